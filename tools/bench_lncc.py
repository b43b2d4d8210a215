#!/usr/bin/env python3
"""Time the local normalised cross-correlation kernels (csrc/lncc.hip) with HIP events on the bench's synthetic pair
(synthetic.make_pair), all in one run: the forward and the backward (one gradient, as a registration needs, and both) at 128^3
and 256^3 for windows 5 and 9, next to the two other streaming two-volume similarity kernels on the same pair (kmh_mi_hist with
given ranges and kmh_mi_bwd), a device copy of the bytes the forward reads (8 B per voxel), and one
register_bspline(metric="lncc") at 128^3 beside the same call with metric="mi" (median of --reg-reps calls from the identity matrix).

    python tools/bench_lncc.py [--reps 30] [--out profiles/lncc_bench.json]

Each figure is the median over --reps calls.  `*_GBps` = the ALGORITHMIC bytes over the time: the forward reads 8 B per voxel; the
backward reads 8 B and writes five 4 B fields, then reads the fields and the pair (28 B) and writes 4 B per gradient: 60 or 64 B.
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--windows", type=int, nargs="+", default=[5, 9])
    ap.add_argument("--reg-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keymorph_amd import _lib, synthetic
    from keymorph_amd.io import register_bspline, voxel_to_mat
    from keymorph_amd.ops import _p, _stream, check
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    bins = 32
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "register_bspline_reps": args.reg_reps, "bins": bins}
    for S in args.sizes:
        f, m = synthetic.make_pair(S, 0, dev)
        V = f.numel()
        out = torch.empty(1, dtype=torch.float32, device=dev)
        gout = torch.ones(1, dtype=torch.float32, device=dev)
        dm, df = torch.empty_like(m), torch.empty_like(f)
        both = torch.cat([m.reshape(-1), f.reshape(-1)])
        dst = torch.empty_like(both)
        res[f"copy_{S}_8B_per_voxel_ms"] = timed(lambda: dst.copy_(both), args.reps)
        for w in args.windows:
            ws = torch.empty(int(lib.kmh_lncc_ws_bytes(1, S, S, S, w)), dtype=torch.uint8, device=dev)

            def fwd():
                check(lib.kmh_lncc_fwd(_p(m), _p(f), 1, S, S, S, w, 1e-5, _p(out), _p(ws), _stream()), "fwd")

            def bwd(two):
                check(lib.kmh_lncc_bwd(_p(m), _p(f), _p(gout), 1, S, S, S, w, 1e-5, _p(dm), _p(df) if two else None, _p(ws),
                                       _stream()), "bwd")
            k = f"lncc_{S}_w{w}"
            res[f"{k}_fwd_ms"] = timed(fwd, args.reps)
            res[f"{k}_fwd_GBps"] = 8.0 * V / (res[f"{k}_fwd_ms"] * 1e6)
            res[f"{k}_bwd_one_gradient_ms"] = timed(lambda: bwd(False), args.reps)
            res[f"{k}_bwd_one_gradient_GBps"] = 60.0 * V / (res[f"{k}_bwd_one_gradient_ms"] * 1e6)
            res[f"{k}_bwd_both_ms"] = timed(lambda: bwd(True), args.reps)
            res[f"{k}_bwd_both_GBps"] = 64.0 * V / (res[f"{k}_bwd_both_ms"] * 1e6)
            res[f"{k}_value"] = float(out[0])
            res[f"{k}_ws_bytes_over_inputs"] = ws.numel() / (8.0 * V)
            del ws
        # the other two-volume streaming similarity on the same pair, in the same run
        mws = torch.empty(int(lib.kmh_mi_ws_bytes(1, bins)), dtype=torch.uint8, device=dev)
        rng = torch.empty((1, 4), dtype=torch.float32, device=dev)
        mi = torch.empty(1, dtype=torch.float32, device=dev)
        G = torch.empty((1, bins, bins), dtype=torch.float32, device=dev)

        def hist():
            check(lib.kmh_mi_hist(_p(m), _p(f), 1, V, bins, 1, 0.0, 1.0, 1, 0.0, 1.0, _p(mws), _p(rng), _stream()), "hist")

        def mi_bwd():
            check(lib.kmh_mi_bwd(_p(m), _p(f), _p(rng), _p(G), _p(gout), 1, V, bins, _p(dm), _p(df), _stream()), "mi_bwd")
        res[f"mi_{S}_hist_given_range_ms"] = timed(hist, args.reps)
        res[f"mi_{S}_hist_GBps"] = 8.0 * V / (res[f"mi_{S}_hist_given_range_ms"] * 1e6)
        hist()
        check(lib.kmh_mi_final(_p(mws), _p(rng), 1, V, bins, _p(mi), _p(G), _stream()), "final")
        res[f"mi_{S}_bwd_ms"] = timed(mi_bwd, args.reps)
        res[f"mi_{S}_bwd_GBps"] = 16.0 * V / (res[f"mi_{S}_bwd_ms"] * 1e6)
        if S == 128:
            mat = voxel_to_mat(torch.eye(3, device=dev)[None], torch.zeros(1, 3, device=dev), (S, S, S))
            for metric in ("lncc", "mi"):
                res[f"register_bspline_{S}_{metric}_ms"] = timed(lambda: register_bspline(f, m, mat=mat, metric=metric),
                                                                 args.reg_reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
