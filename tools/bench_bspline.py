#!/usr/bin/env python3
"""Time the free-form deformation (csrc/bspline.hip) with HIP events on the bench's synthetic pair (synthetic.make_pair), a
rotation + shear + shift matrix and control spacing 8, at 128^3 and 256^3, all in one process:

  kernels     kmh_bspline_grid_fwd / kmh_bspline_grid_bwd against kmh_affine_grid_fwd / kmh_affine_grid_bwd -- the same 12 B per
              voxel written / read, so the natural yardstick; the four launches alternate inside every repetition, each figure
              is the median over --reps
  step        one optimisation step of io.register_bspline at full size: bspline_grid -> align_img -> mutual_information
              (ranges given) + bending * bspline_bending, backward to the lattice
  register    one io.register_bspline(fixed, moving, mat) with its defaults at 128^3 (median of --est-reps calls)

    python tools/bench_bspline.py [--reps 30] [--out profiles/bspline_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    return float(np.median([event_ms(fn) for _ in range(reps)]))


def alternating(fns, reps, warmup=3):
    """Medians of several arms whose calls alternate inside every repetition."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ts[k].append(event_ms(fn))
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--spacing", type=int, default=8)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--est-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keymorph_amd import _lib, ops, synthetic
    from keymorph_amd.io import register_bspline
    from keymorph_amd.ops import _p, _stream, check
    from keymorph_amd.utils import align_img
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = args.bins
    res = {"device": torch.cuda.get_device_name(dev), "bins": B, "spacing": args.spacing, "reps": args.reps,
           "register_reps": args.est_reps}
    for S in args.sizes:
        f, m = synthetic.make_pair(S, 0, dev)
        dims = (S, S, S)
        lat = ops.bspline_lattice_shape(dims, args.spacing)
        mat = synthetic.random_affine_matrix(3, dev)[:, :3, :].contiguous()
        g = torch.Generator().manual_seed(S)
        ctrl = (0.02 * torch.randn(1, 3, *lat, generator=g)).to(dev)
        grid = torch.empty((1, S, S, S, 3), dtype=torch.float32, device=dev)
        dgrid = torch.randn(1, S, S, S, 3, generator=g).to(dev)
        dctrl, dmat = torch.empty_like(ctrl), torch.empty_like(mat)
        ws = ops.workspace(int(lib.kmh_bspline_grid_ws_bytes(1, S, S, S, *lat)), dev, "bspline_bwd")
        rws = ops._reduce_ws(dev)
        s = _stream()
        k = f"bspline_{S}"
        res[f"{k}_lattice"] = list(lat)
        res[f"{k}_ws_mb"] = lib.kmh_bspline_grid_ws_bytes(1, S, S, S, *lat) / 1e6
        arms = [
            lambda: check(lib.kmh_bspline_grid_fwd(_p(ctrl), _p(mat), _p(grid), 1, S, S, S, *lat, s), "bspline fwd"),
            lambda: check(lib.kmh_affine_grid_fwd(_p(mat), _p(grid), 1, S, S, S, s), "affine fwd"),
            lambda: check(lib.kmh_bspline_grid_bwd(_p(dgrid), _p(dctrl), 1, S, S, S, *lat, _p(ws), s), "bspline bwd"),
            lambda: check(lib.kmh_affine_grid_bwd(_p(dgrid), _p(dmat), 1, S, S, S, _p(rws), s), "affine bwd"),
            lambda: check(lib.kmh_bspline_grid_fwd(_p(ctrl), None, _p(grid), 1, S, S, S, *lat, s), "bspline fwd, no matrix"),
        ]
        (res[f"{k}_fwd_ms"], res[f"{k}_affine_fwd_ms"], res[f"{k}_bwd_ms"], res[f"{k}_affine_bwd_ms"],
         res[f"{k}_fwd_nomat_ms"]) = alternating(arms, args.reps)
        res[f"{k}_fwd_gbps"] = 12.0 * S ** 3 / res[f"{k}_fwd_ms"] / 1e6
        res[f"{k}_bwd_gbps"] = 12.0 * S ** 3 / res[f"{k}_bwd_ms"] / 1e6

        rng = ops.mi_ranges(m, f, B)
        q = (ctrl * (S / 2.0)).requires_grad_(True)

        def step():
            q.grad = None
            warped = align_img(ops.bspline_grid(q * (2.0 / S), dims, mat), m)
            (0.05 * ops.bspline_bending(q) - ops.mutual_information(warped, f, B, ranges=rng)).sum().backward()

        res[f"{k}_step_ms"] = timed(step, args.reps)
        if S == 128:
            res[f"{k}_register_ms"] = timed(lambda: register_bspline(f, m, mat=mat, control_spacing=args.spacing, bins=B),
                                            args.est_reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
