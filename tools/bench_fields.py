#!/usr/bin/env python3
"""Time keymorph_amd.fields (csrc/fields.hip) with HIP events at 128^3 and 256^3, n = 1, on two inputs built on the device: a
rotated, zoomed affine grid (ops.affine_grid) and a thin-plate-spline grid (ops.tps_fit + ops.tps_grid on seeded keypoints).

    python tools/bench_fields.py [--reps 30] [--sizes 128 256] [--out profiles/fields_bench.json]

compose(first = TPS grid, then = affine grid) is timed against the only route there was before it -- permute().contiguous()
of `then`, ops.grid_sample3d, permute().contiguous() of the result -- in the SAME loop, alternating the two, and the two results
are compared bit for bit.  Bytes are the algorithmic ones, computed from the shapes: compose reads first and then once and writes
the result, 36 B per voxel; the old route moves 24 + 36 + 24 = 84 B per voxel.  invert: time, unconverged voxels and the mean
number of Newton steps per voxel on both inputs.  to_displacement / from_displacement: 24 B per voxel.  A device copy of a grid
(24 B per voxel) is timed alongside as the streaming yardstick.  Every time is the median over --reps calls."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_interleaved(fns, reps):
    """Median ms of every callable, measured in one loop that alternates them."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in ts]


def rotation(deg_z, deg_x, deg_y, scale):
    def rot(axis, deg):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        i, j = [(0, 1), (1, 2), (0, 2)][axis]
        m = torch.eye(3, dtype=torch.float64)
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return m
    return scale * rot(0, deg_z) @ rot(1, deg_x) @ rot(2, deg_y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--keypoints", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keymorph_amd import fields, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "n": 1, "keypoints": args.keypoints}
    gen = torch.Generator().manual_seed(0)
    ctrl = (torch.rand(1, args.keypoints, 3, generator=gen) * 1.6 - 0.8).to(dev)
    tgt = (1.2 * ctrl.cpu() + 0.03 * torch.randn(1, args.keypoints, 3, generator=gen)).to(dev)
    theta = ops.tps_fit(ctrl, tgt, torch.ones(1, device=dev))
    mat = torch.cat([rotation(12.0, 7.0, -5.0, 1.35), torch.tensor([[0.03], [-0.02], [0.02]], dtype=torch.float64)], dim=1)
    mat = mat.float().unsqueeze(0).to(dev)
    for S in args.sizes:
        V = S ** 3
        k = f"fields_{S}"
        g_aff = ops.affine_grid(mat, (S, S, S))
        g_tps = ops.tps_grid(theta, ctrl, (S, S, S))

        def old_route():
            x = g_aff.permute(0, 4, 1, 2, 3).contiguous()
            return ops.grid_sample3d(x, g_tps).permute(0, 2, 3, 4, 1).contiguous()

        new, old = fields.compose(g_tps, g_aff), old_route()
        res[f"{k}_compose_equals_old_route"] = bool(torch.equal(new, old))
        del new, old
        dst = torch.empty_like(g_aff)
        t_new, t_old, t_copy = timed_interleaved([lambda: fields.compose(g_tps, g_aff), old_route, lambda: dst.copy_(g_aff)],
                                                 args.reps)
        res[f"{k}_compose_ms"], res[f"{k}_old_route_ms"], res[f"{k}_copy_24B_per_voxel_ms"] = t_new, t_old, t_copy
        res[f"{k}_compose_speedup"] = t_old / t_new
        res[f"{k}_compose_GBps"] = 36.0 * V / (t_new * 1e6)
        res[f"{k}_old_route_GBps"] = 84.0 * V / (t_old * 1e6)
        res[f"{k}_copy_GBps"] = 24.0 * V / (t_copy * 1e6)
        for name, g in (("affine", g_aff), ("tps", g_tps)):
            res[f"{k}_invert_{name}_ms"] = timed_interleaved([lambda: fields.invert(g)], args.reps)[0]
            res[f"{k}_invert_{name}_kernel_ms"] = timed_interleaved([_kernel_only(fields, ops, g)], args.reps)[0]
            _, conv, unconv, maxres, iters = fields._invert(g, 1e-5, 20)
            res[f"{k}_invert_{name}_unconverged"] = int(unconv[0])
            res[f"{k}_invert_{name}_max_residual"] = float(maxres[0])
            res[f"{k}_invert_{name}_mean_newton_steps"] = float(iters[0]) / V
        disp = fields.to_displacement(g_tps)
        t_to, t_from = timed_interleaved([lambda: fields.to_displacement(g_tps), lambda: fields.from_displacement(disp)],
                                         args.reps)
        res[f"{k}_to_displacement_ms"], res[f"{k}_from_displacement_ms"] = t_to, t_from
        res[f"{k}_to_displacement_GBps"] = 24.0 * V / (t_to * 1e6)
        res[f"{k}_from_displacement_GBps"] = 24.0 * V / (t_from * 1e6)
        del g_aff, g_tps, disp, dst
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def _kernel_only(fields, ops, g):
    """The Newton kernel and its statistics pass alone (fields.invert without the affine start and the allocations)."""
    from keymorph_amd import _lib
    from keymorph_amd.ops import _p, _stream, check
    lib = _lib.load()
    n, D, H, W, _ = g.shape
    start = fields._affine_start(g)
    out = torch.empty_like(g)
    conv = torch.empty((n, D, H, W), dtype=torch.uint8, device=g.device)
    unconv = torch.empty(n, dtype=torch.int64, device=g.device)
    maxres = torch.empty(n, dtype=torch.float32, device=g.device)
    ws = ops.workspace(int(lib.kmh_field_invert_ws_bytes(n, D, H, W)), g.device, "fields")

    def run():
        check(lib.kmh_field_invert(_p(g), _p(start), _p(out), _p(conv), _p(unconv), _p(maxres), None, n, D, H, W, 1e-5, 20,
                                   _p(ws), _stream()), "kmh_field_invert")
    return run


if __name__ == "__main__":
    main()
