#!/usr/bin/env python3
"""Time the MIND-SSC kernels (csrc/mind.hip) with HIP events on the bench's synthetic pair (synthetic.make_pair), all in one run:
the bounds, the forward and the backward (one gradient, as a registration needs, and both) at 128^3 and 256^3 for
(radius, dilation) = (1, 2) and (2, 2), next to kmh_lncc_fwd and kmh_lncc_bwd at window 9 on the same pair, a device copy of the
bytes the forward reads (8 B per voxel), and one register_bspline(metric="mind") at 128^3 beside the same call with metric="mi"
(median of --reg-reps calls from the identity matrix).

    python tools/bench_mind.py [--reps 30] [--out profiles/mind_bench.json]

Each figure is the median over --reps calls.  `*_GBps` = the ALGORITHMIC bytes over the time: the forward reads 8 B per voxel;
the backward per gradient reads 8 B, writes and reads the 12 fields of gD (96 B), reads 4 B, writes and reads the 6 fields of G
(48 B) and writes 4 B: 160 B.  `*_lds_reads_per_voxel` = the 4-byte LDS reads of the forward's walk per voxel (both volumes),
counted from the loop bounds: what bounds it, not the 8 B from memory.
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


def lds_reads_per_voxel(r):
    """Per voxel of a 4 x 8 x 32 tile and volume: (4 + 2r) box planes, each (8 + 2r) rows of 32 columns x (2r+1) taps x 6
    neighbours (the x pass), and 12 channels x (2r+1) rows (the y pass) per lane; two volumes."""
    planes, rows, win = 4 + 2 * r, 8 + 2 * r, 2 * r + 1
    return 2 * planes * (rows * 32 * win * 6 + 256 * 12 * win) / (4 * 8 * 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reg-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keymorph_amd import _lib, synthetic
    from keymorph_amd.io import register_bspline, voxel_to_mat
    from keymorph_amd.ops import _p, _stream, check
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "register_bspline_reps": args.reg_reps}
    for S in args.sizes:
        f, m = synthetic.make_pair(S, 0, dev)
        V = f.numel()
        out = torch.empty(1, dtype=torch.float32, device=dev)
        gout = torch.ones(1, dtype=torch.float32, device=dev)
        bounds = torch.empty((1, 2, 2), dtype=torch.float32, device=dev)
        dm, df = torch.empty_like(m), torch.empty_like(f)
        both = torch.cat([m.reshape(-1), f.reshape(-1)])
        dst = torch.empty_like(both)
        res[f"copy_{S}_8B_per_voxel_ms"] = timed(lambda: dst.copy_(both), args.reps)
        for r, d in ((1, 2), (2, 2)):
            ws = torch.empty(int(lib.kmh_mind_ws_bytes(1, S, S, S, r, d)), dtype=torch.uint8, device=dev)

            def bnd():
                check(lib.kmh_mind_bounds(_p(m), _p(f), 1, S, S, S, r, d, _p(bounds), _p(ws), _stream()), "bounds")

            def fwd():
                check(lib.kmh_mind_fwd(_p(m), _p(f), _p(bounds), 1, S, S, S, r, d, _p(out), _p(ws), _stream()), "fwd")

            def bwd(two):
                check(lib.kmh_mind_bwd(_p(m), _p(f), _p(bounds), _p(gout), 1, S, S, S, r, d, _p(dm), _p(df) if two else None,
                                       _p(ws), _stream()), "bwd")
            k = f"mind_{S}_r{r}d{d}"
            res[f"{k}_bounds_ms"] = timed(bnd, args.reps)
            res[f"{k}_fwd_ms"] = timed(fwd, args.reps)
            res[f"{k}_fwd_GBps"] = 8.0 * V / (res[f"{k}_fwd_ms"] * 1e6)
            res[f"{k}_fwd_lds_reads_per_voxel"] = lds_reads_per_voxel(r)
            res[f"{k}_fwd_lds_TBps"] = 4.0 * lds_reads_per_voxel(r) * V / (res[f"{k}_fwd_ms"] * 1e9)
            res[f"{k}_bwd_one_gradient_ms"] = timed(lambda: bwd(False), args.reps)
            res[f"{k}_bwd_one_gradient_GBps"] = 160.0 * V / (res[f"{k}_bwd_one_gradient_ms"] * 1e6)
            res[f"{k}_bwd_both_ms"] = timed(lambda: bwd(True), args.reps)
            res[f"{k}_bwd_both_GBps"] = 320.0 * V / (res[f"{k}_bwd_both_ms"] * 1e6)
            res[f"{k}_value"] = float(out[0])
            res[f"{k}_ws_bytes_over_inputs"] = ws.numel() / (8.0 * V)
            del ws
        # local NCC at window 9 on the same pair, in the same run
        w = 9
        ws = torch.empty(int(lib.kmh_lncc_ws_bytes(1, S, S, S, w)), dtype=torch.uint8, device=dev)

        def lfwd():
            check(lib.kmh_lncc_fwd(_p(m), _p(f), 1, S, S, S, w, 1e-5, _p(out), _p(ws), _stream()), "lncc_fwd")

        def lbwd(two):
            check(lib.kmh_lncc_bwd(_p(m), _p(f), _p(gout), 1, S, S, S, w, 1e-5, _p(dm), _p(df) if two else None, _p(ws), _stream()),
                  "lncc_bwd")
        res[f"lncc_{S}_w9_fwd_ms"] = timed(lfwd, args.reps)
        res[f"lncc_{S}_w9_bwd_one_gradient_ms"] = timed(lambda: lbwd(False), args.reps)
        res[f"lncc_{S}_w9_bwd_both_ms"] = timed(lambda: lbwd(True), args.reps)
        del ws
        if S == 128:
            mat = voxel_to_mat(torch.eye(3, device=dev)[None], torch.zeros(1, 3, device=dev), (S, S, S))
            for metric in ("mind", "mi"):
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
