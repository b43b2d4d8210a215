#!/usr/bin/env python3
"""Time the fused warp + mutual-information path (csrc/warp_mi.hip) against the chain of operators it replaces, with HIP events on
the bench's synthetic pair (synthetic.make_pair) and a rotation + shear + shift matrix, at 128^3 and 256^3, all in one process:

  step        one forward + backward to `mat` of ops.warp_mutual_information (ranges given), against
              affine_grid -> align_img -> mutual_information(range_a, range_b) -> backward to `mat`; the two arms alternate inside
              every repetition, each figure is the median over --reps
  kernels     each launch on its own: fused kmh_warp_mi_hist, kmh_mi_final, kmh_warp_mi_bwd, kmh_mi_range; unfused
              kmh_affine_grid_fwd, kmh_grid_sample3d_fwd, kmh_mi_hist (given ranges), kmh_mi_bwd (da only),
              kmh_grid_sample3d_bwd_grid, kmh_affine_grid_bwd
  register    one io.register_intensity(fixed, moving, "rigid") at 128^3 (median of --est-reps calls)

    python tools/bench_warp_mi.py [--reps 30] [--bins 32] [--out profiles/warp_mi_bench.json]

`*_equal` records that the two arms returned the same MI bit for bit on the timed inputs.
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


def alternating(fns, reps):
    """Medians of several arms whose calls alternate inside every repetition."""
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--est-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keymorph_amd import _lib, ops, synthetic
    from keymorph_amd.io import register_intensity
    from keymorph_amd.ops import _p, _stream, check
    from keymorph_amd.utils import align_img
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = args.bins
    res = {"device": torch.cuda.get_device_name(dev), "bins": B, "reps": args.reps, "register_reps": args.est_reps}
    for S in args.sizes:
        f, m = synthetic.make_pair(S, 0, dev)
        dims, V = (S, S, S), S ** 3
        mat = synthetic.random_affine_matrix(3, dev)[:, :3, :].contiguous().requires_grad_(True)
        rng = ops.mi_ranges(m, f, B)
        ra, rb = (float(m.min()), float(m.max())), (float(f.min()), float(f.max()))

        def fused_step():
            mat.grad = None
            ops.warp_mutual_information(m, f, mat, B, rng).sum().backward()

        def chain_step():
            mat.grad = None
            ops.mutual_information(align_img(ops.affine_grid(mat, dims), m), f, B, ra, rb).sum().backward()

        k = f"warp_mi_{S}"
        res[f"{k}_step_fused_ms"], res[f"{k}_step_chain_ms"] = alternating([fused_step, chain_step], args.reps)
        with torch.no_grad():
            a = ops.warp_mutual_information(m, f, mat, B, rng)
            b = ops.mutual_information(align_img(ops.affine_grid(mat, dims), m), f, B, ra, rb)
        res[f"{k}_value"], res[f"{k}_equal"] = float(a[0]), bool(torch.equal(a, b))
        fused_step()
        g_fused = mat.grad.clone()
        chain_step()
        res[f"{k}_dmat_rel_diff"] = float((g_fused - mat.grad).norm() / mat.grad.norm())

        # every launch on its own
        md = mat.detach()
        ws = torch.empty(int(lib.kmh_warp_mi_ws_bytes(1, B, S, S, S)), dtype=torch.uint8, device=dev)
        mi = torch.empty(1, dtype=torch.float32, device=dev)
        G = torch.empty((1, B, B), dtype=torch.float32, device=dev)
        gout = torch.ones(1, dtype=torch.float32, device=dev)
        dmat = torch.empty_like(md)
        rng2 = torch.empty_like(rng)
        grid = torch.empty((1, S, S, S, 3), dtype=torch.float32, device=dev)
        warped, da, dgrid = torch.empty_like(m), torch.empty_like(m), torch.empty_like(grid)
        rws = ops._reduce_ws(dev)
        s = _stream()
        launches = {
            "fused_hist": lambda: check(lib.kmh_warp_mi_hist(_p(m), _p(f), _p(md), _p(rng), 1, S, S, S, B, _p(ws), s), "hist"),
            "final": lambda: check(lib.kmh_mi_final(_p(ws), _p(rng), 1, V, B, _p(mi), _p(G), s), "final"),
            "fused_bwd": lambda: check(lib.kmh_warp_mi_bwd(_p(m), _p(f), _p(md), _p(rng), _p(G), _p(gout), 1, S, S, S, B, _p(ws),
                                                          _p(dmat), s), "bwd"),
            "range": lambda: check(lib.kmh_mi_range(_p(m), _p(f), 1, V, B, 0, 0.0, 0.0, 0, 0.0, 0.0, _p(ws), _p(rng2), s), "range"),
            "chain_affine_grid": lambda: check(lib.kmh_affine_grid_fwd(_p(md), _p(grid), 1, S, S, S, s), "grid"),
            "chain_sample": lambda: check(lib.kmh_grid_sample3d_fwd(_p(m), _p(grid), _p(warped), 1, 1, S, S, S, S, S, S, 0, s),
                                          "sample"),
            "chain_hist": lambda: check(lib.kmh_mi_hist(_p(warped), _p(f), 1, V, B, 1, ra[0], ra[1], 1, rb[0], rb[1], _p(ws),
                                                        _p(rng2), s), "mi_hist"),
            "chain_mi_bwd": lambda: check(lib.kmh_mi_bwd(_p(warped), _p(f), _p(rng2), _p(G), _p(gout), 1, V, B, _p(da), None, s),
                                          "mi_bwd"),
            "chain_sample_bwd": lambda: check(lib.kmh_grid_sample3d_bwd_grid(_p(m), _p(grid), _p(da), _p(dgrid), 1, 1, S, S, S, S,
                                                                            S, S, s), "sample_bwd"),
            "chain_affine_grid_bwd": lambda: check(lib.kmh_affine_grid_bwd(_p(dgrid), _p(dmat), 1, S, S, S, _p(rws), s),
                                                   "grid_bwd"),
        }
        for name, fn in launches.items():       # in this order: every launch finds its inputs written by the ones before it
            res[f"{k}_{name}_ms"] = timed(fn, args.reps)
        res[f"{k}_fused_kernels_ms"] = sum(res[f"{k}_{n}_ms"] for n in ("fused_hist", "final", "fused_bwd"))
        res[f"{k}_chain_kernels_ms"] = sum(res[f"{k}_{n}_ms"] for n in launches if n.startswith("chain_")) + res[f"{k}_final_ms"]
        if S == 128:
            res[f"{k}_register_rigid_ms"] = timed(lambda: register_intensity(f, m, "rigid", bins=B), args.est_reps)
            out = register_intensity(f, m, "rigid", bins=B)
            with torch.no_grad():
                res[f"{k}_register_rigid_mi"] = float(ops.warp_mutual_information(m, f, out, B)[0])
                res[f"{k}_unregistered_mi"] = float(ops.mutual_information(m, f, B)[0])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
