#!/usr/bin/env python3
"""Time the cubic B-spline kernels (csrc/cubic.hip) with HIP events beside the trilinear sampler's, all in one run: at 128^3 and
256^3, single channel and 14 channels, the prefilter, kmh_cubic_sample_fwd and kmh_cubic_sample_bwd_grid next to
kmh_grid_sample3d_fwd and kmh_grid_sample3d_bwd_grid on the same grid -- bench.py's three-axis affine grid
(synthetic.random_affine_matrix(3)).

    python tools/bench_cubic.py [--reps 30] [--window-ms 1.0] [--out profiles/cubic_bench.json]

The five arms of a configuration alternate (one timed window of each per round, --reps rounds) and each figure is the median
over the rounds.  A window is a number of back-to-back calls between two events, chosen per arm from a first timing so that the
window lasts at least --window-ms (`*_calls_per_window` records it): the shortest kernel is timed over a millisecond, not over the
events.  Every call of an arm runs on the same buffers, and the one-channel volumes (8 and 67 MB) and the 128^3 14-channel
one (117 MB) fit the 256 MB Infinity Cache: the figures are WARM-CACHE times, not reads from HBM.  `*_GBps` = the ALGORITHMIC bytes over the time: the prefilter 8 B per voxel and pass (its
floor: every pass reads and writes each voxel once; the y and z passes as written move 16), a sampler forward 12 + 8 C per voxel
(grid, volume once, output), a grid backward 24 + 8 C (cotangent, grid, volume once, grid gradient) -- the same count for the
cubic and the trilinear kernels, so the ratio of their times is the ratio of their rates.  `*_over_trilinear` = cubic time over
trilinear time.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, calls):
    """ms per call over `calls` back-to-back calls between two events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternate(arms, reps, window_ms):
    """{name: fn} -> ({name: median ms per call}, {name: 10th - 90th percentile spread}, {name: calls per window}); every round
    times one window of each arm, in turn"""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    calls = {k: max(4, min(1024, math.ceil(window_ms / max(window(fn, 4), 1e-4)))) for k, fn in arms.items()}
    ts = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ts[k].append(window(fn, calls[k]))
    return ({k: float(np.median(v)) for k, v in ts.items()},
            {k: float(np.percentile(v, 90) - np.percentile(v, 10)) for k, v in ts.items()}, calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window-ms", type=float, default=1.0)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 14])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cubic_bench.json"))
    args = ap.parse_args()
    from keymorph_amd import _lib, synthetic
    from keymorph_amd.ops import _p, _stream, check
    from keymorph_amd.transformations import AffineTransform
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "window_ms": args.window_ms,
           "cache": "warm: every call of an arm reuses the same buffers (256 MB Infinity Cache)",
           "grid": "synthetic.random_affine_matrix(3): rotations about all three axes, shear, scale"}
    gen = torch.Generator(device=dev).manual_seed(0)
    for S in args.sizes:
        grid = AffineTransform(matrix=synthetic.random_affine_matrix(3, dev), dim=3).get_flow_field((1, 1, S, S, S)).contiguous()
        dgrid = torch.empty_like(grid)
        V = S ** 3
        for C in args.channels:
            x = torch.rand(1, C, S, S, S, device=dev, generator=gen)
            coef, out = torch.empty_like(x), torch.empty_like(x)
            gout = torch.randn(1, C, S, S, S, device=dev, generator=gen)
            dims = (1, C, S, S, S, S, S, S)
            arms = {
                "prefilter": lambda: check(lib.kmh_cubic_prefilter(_p(x), _p(coef), 1, C, S, S, S, _stream()), "prefilter"),
                "cubic_fwd": lambda: check(lib.kmh_cubic_sample_fwd(_p(coef), _p(grid), _p(out), *dims, _stream()), "cubic_fwd"),
                "trilinear_fwd": lambda: check(lib.kmh_grid_sample3d_fwd(_p(x), _p(grid), _p(out), *dims, 0, _stream()), "fwd"),
                "cubic_bwd_grid": lambda: check(lib.kmh_cubic_sample_bwd_grid(_p(coef), _p(grid), _p(gout), _p(dgrid), *dims,
                                                                              _stream()), "cubic_bwd"),
                "trilinear_bwd_grid": lambda: check(lib.kmh_grid_sample3d_bwd_grid(_p(x), _p(grid), _p(gout), _p(dgrid), *dims,
                                                                                   _stream()), "bwd"),
            }
            ms, spread, calls = alternate(arms, args.reps, args.window_ms)
            k = f"{S}_C{C}"
            nbytes = {"prefilter": 3 * 8.0 * C * V, "cubic_fwd": (12.0 + 8 * C) * V, "trilinear_fwd": (12.0 + 8 * C) * V,
                      "cubic_bwd_grid": (24.0 + 8 * C) * V, "trilinear_bwd_grid": (24.0 + 8 * C) * V}
            for name, t in ms.items():
                res[f"{name}_{k}_ms"] = t
                res[f"{name}_{k}_p10_p90_spread_ms"] = spread[name]
                res[f"{name}_{k}_calls_per_window"] = calls[name]
                res[f"{name}_{k}_GBps"] = nbytes[name] / (t * 1e6)
            res[f"prefilter_{k}_over_floor_at_6.29TBps"] = ms["prefilter"] / (nbytes["prefilter"] / 6.29e9)      # the measured copy rate
            res[f"cubic_fwd_{k}_over_trilinear"] = ms["cubic_fwd"] / ms["trilinear_fwd"]
            res[f"cubic_bwd_grid_{k}_over_trilinear"] = ms["cubic_bwd_grid"] / ms["trilinear_bwd_grid"]
            res[f"checksum_{k}"] = float(out.double().sum()) + float(dgrid.double().abs().sum())
            del x, coef, out, gout
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
