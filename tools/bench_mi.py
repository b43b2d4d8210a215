#!/usr/bin/env python3
"""Time the mutual-information kernels (csrc/mi.hip) with HIP events on the bench's synthetic pair (synthetic.make_pair), all
in one run: the histogram pass (with the min / max pass, and with caller-given ranges: the histogram alone), the finalise and
the backward (both gradients) at 128^3 and 256^3, the histogram of the same pair under a ball mask (radius 0.4 of the side: 73 %
background, as in the centering step), one estimate_translation at 128^3 (median of --est-reps calls), a device copy of the bytes
the forward reads (8 B per voxel), and the fp64 restatement on the host at 128^3 (tests/mi_ref.py: like tools/bench_lc2.py, this
tool takes its host yardstick from the test tree and runs from a checkout).

    python tools/bench_mi.py [--reps 30] [--bins 32] [--out profiles/mi_bench.json]

Each figure is the median over --reps calls; `*_copy_fraction` = the copy's time over the kernel's.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--est-reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keymorph_amd import _lib, ops, synthetic
    from keymorph_amd.io import estimate_translation
    from keymorph_amd.ops import _p, _stream, check
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = args.bins
    res = {"device": torch.cuda.get_device_name(dev), "bins": B, "reps": args.reps, "estimate_translation_reps": args.est_reps}
    for S in args.sizes:
        f, m = synthetic.make_pair(S, 0, dev)
        V = f.numel()
        ws = torch.empty(int(lib.kmh_mi_ws_bytes(1, B)), dtype=torch.uint8, device=dev)
        rng = torch.empty((1, 4), dtype=torch.float32, device=dev)
        mi = torch.empty(1, dtype=torch.float32, device=dev)
        G = torch.empty((1, B, B), dtype=torch.float32, device=dev)
        gout = torch.ones(1, dtype=torch.float32, device=dev)
        dm, df = torch.empty_like(m), torch.empty_like(f)
        both = torch.cat([m.reshape(-1), f.reshape(-1)])
        dst = torch.empty_like(both)

        def hist(given, x=m, y=f):
            check(lib.kmh_mi_hist(_p(x), _p(y), 1, V, B, given, 0.0, 1.0, given, 0.0, 1.0, _p(ws), _p(rng), _stream()), "hist")

        def final():
            check(lib.kmh_mi_final(_p(ws), _p(rng), 1, V, B, _p(mi), _p(G), _stream()), "final")

        def bwd():
            check(lib.kmh_mi_bwd(_p(m), _p(f), _p(rng), _p(G), _p(gout), 1, V, B, _p(dm), _p(df), _stream()), "bwd")

        k = f"mi_{S}"
        res[f"{k}_hist_minmax_ms"] = timed(lambda: hist(0), args.reps)
        res[f"{k}_hist_given_range_ms"] = timed(lambda: hist(1), args.reps)
        ax = torch.linspace(-1, 1, S, device=dev)
        ball = ((ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) <= 0.64).float()[None, None]
        mm, fm = (m * ball).contiguous(), (f * ball).contiguous()
        res[f"{k}_hist_masked_given_range_ms"] = timed(lambda: hist(1, mm, fm), args.reps)
        res[f"{k}_masked_background_fraction"] = 1.0 - float(ball.mean())
        hist(0)
        res[f"{k}_final_ms"] = timed(final, args.reps)
        res[f"{k}_bwd_ms"] = timed(bwd, args.reps)
        res[f"{k}_copy_8B_per_voxel_ms"] = timed(lambda: dst.copy_(both), args.reps)
        res[f"{k}_value"] = float(mi[0])
        res[f"{k}_hist_copy_fraction"] = res[f"{k}_copy_8B_per_voxel_ms"] / res[f"{k}_hist_given_range_ms"]
        res[f"{k}_bwd_read_write_GBps"] = 16.0 * V / (res[f"{k}_bwd_ms"] * 1e6)
        res[f"{k}_fwd_op_ms"] = timed(lambda: ops.mutual_information(m, f, B), args.reps)
        if S == 128:
            res[f"{k}_estimate_translation_ms"] = timed(lambda: estimate_translation(f, m, bins=B), args.est_reps)
            res[f"{k}_estimate_translation_t"] = estimate_translation(f, m, bins=B)[0].tolist()
            from tests import mi_ref
            f64, m64 = f.cpu().double(), m.cpu().double()
            t0 = time.perf_counter()
            ref = float(mi_ref.mutual_information(m64, f64, B)[0])
            res[f"{k}_host_fp64_restatement_ms"] = (time.perf_counter() - t0) * 1e3
            res[f"{k}_value_minus_fp64"] = float(mi[0]) - ref
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
