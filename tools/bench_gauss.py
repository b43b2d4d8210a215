#!/usr/bin/env python3
"""Time Gaussian smoothing (csrc/gauss.hip) with HIP events beside a device copy of the same bytes and the cubic prefilter, all in
one run: forward and transpose at 128^3 and 256^3, one and three channels, sigma 1, 2 and 4 (R = 4, 8, 16), on all three axes
and on one axis only (x, y, z each) -- then one io.estimate_translation and one io.register_bspline at 128^3 with and without
smoothing_sigmas="auto".

    python tools/bench_gauss.py [--reps 30] [--window-ms 1.0] [--out profiles/gauss_bench.json]

The arms of a configuration alternate (one timed window of each per round, --reps rounds) and each figure is the median over the
rounds.  A window is a number of back-to-back calls between two events, chosen per arm from a first timing so that the window
lasts at least --window-ms (`*_calls_per_window` records it).  Every call of an arm runs on the same buffers, and the one-channel
volumes (8 and 67 MB) and the 128^3 three-channel one fit the 256 MB Infinity Cache: those figures are WARM-CACHE times, not reads
from HBM; 256^3 with three channels (201 MB in, 201 MB out, 201 MB workspace) does not fit.

`copy` is out.copy_(x): 4 B in and 4 B out per voxel, the operator's floor (8 B per voxel for the WHOLE operator) at the rate this
device reaches in this run.  `*_over_floor` = an arm's time over the copy's time: for a one-axis arm that is the pass against its
own floor; an all-axes arm makes three passes, so its figure is three trips against the one a fused operator would need.
`*_over_pass_floor` = the all-axes time over three copies.  `prefilter` is kmh_cubic_prefilter on the same volume (three recursive
passes; its y and z passes move 16 B per voxel).
The driver timings are host clocks around a call that ends in a synchronise, medians of --driver-reps alternating runs after one
warm-up of each.
"""
import argparse
import json
import math
import os
import sys
import time

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


def driver_pair(size, dev):
    """a smooth multi-modal-looking pair with voxel noise, on the device: fixed = smoothed noise rescaled to [0, 1], moving = a
    non-monotone remap of it shifted by (2.3, -1.6, 0.8) voxels; 0.1 randn noise on both"""
    from keymorph_amd import ops
    from keymorph_amd.io import translate
    gen = torch.Generator(device=dev).manual_seed(7)
    f = ops.gaussian_smooth(torch.randn(1, 1, size, size, size, device=dev, generator=gen), 6.0)
    f = (f - f.min()) / (f.max() - f.min())
    m = translate(0.8 * (1 - f) ** 2 + 0.2 * torch.sin(6 * f) ** 2, torch.tensor([[-2.3, 1.6, -0.8]], device=dev))
    return (f + 0.1 * torch.randn(f.shape, device=dev, generator=gen)).contiguous(), \
        (m + 0.1 * torch.randn(f.shape, device=dev, generator=gen)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window-ms", type=float, default=1.0)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--sigmas", type=float, nargs="+", default=[1.0, 2.0, 4.0])
    ap.add_argument("--driver-size", type=int, default=128)
    ap.add_argument("--driver-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gauss: no GPU: timings are taken on the device or not at all")
    from keymorph_amd import _lib, ops
    from keymorph_amd.ops import _p, _stream, check
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "window_ms": args.window_ms,
           "cache": "warm: every call of an arm reuses the same buffers (256 MB Infinity Cache)",
           "floor": "copy = out.copy_(x), 8 B per voxel, timed in the same rounds"}
    gen = torch.Generator(device=dev).manual_seed(0)
    for S in args.sizes:
        V = S ** 3
        for C in args.channels:
            x = torch.randn(1, C, S, S, S, device=dev, generator=gen)
            out = torch.empty_like(x)
            arms = {"copy": lambda: out.copy_(x),
                    "prefilter": lambda: check(lib.kmh_cubic_prefilter(_p(x), _p(out), 1, C, S, S, S, _stream()), "prefilter")}
            for sg in args.sigmas:
                for axes, sigma in (("zyx", (sg, sg, sg)), ("x", (0.0, 0.0, sg)), ("y", (0.0, sg, 0.0)), ("z", (sg, 0.0, 0.0))):
                    plan = ops._gauss_plan("bench_gauss", x, sigma, 4.0)
                    for name, transpose in (("fwd", False), ("bwd", True)):
                        arms[f"{name}_s{sg:g}_{axes}"] = (lambda p=plan, t=transpose: ops._gauss_call(x, p, t))
            ms, spread, calls = alternate(arms, args.reps, args.window_ms)
            k = f"{S}_C{C}"
            for name, t in ms.items():
                res[f"{name}_{k}_ms"] = t
                res[f"{name}_{k}_p10_p90_spread_ms"] = spread[name]
                res[f"{name}_{k}_calls_per_window"] = calls[name]
                if name not in ("copy", "prefilter"):
                    res[f"{name}_{k}_over_floor"] = t / ms["copy"]
                    if name.endswith("_zyx"):
                        res[f"{name}_{k}_over_pass_floor"] = t / (3 * ms["copy"])
            res[f"copy_{k}_GBps"] = 8.0 * C * V / (ms["copy"] * 1e6)
            res[f"prefilter_{k}_over_floor"] = ms["prefilter"] / ms["copy"]
            res[f"checksum_{k}"] = float(ops._gauss_call(x, ops._gauss_plan("bench_gauss", x, 2.0, 4.0), False).double().sum())
            del x, out
    # the drivers, with and without the smoothed pyramid
    from keymorph_amd.io import estimate_translation, register_bspline, register_intensity
    f, m = driver_pair(args.driver_size, dev)
    mat = register_intensity(f, m, "translation")
    runs = {"estimate_translation": lambda sm: estimate_translation(f, m, smoothing_sigmas=sm),
            "register_bspline": lambda sm: register_bspline(f, m, mat, smoothing_sigmas=sm)}
    for name, run in runs.items():
        ts = {None: [], "auto": []}
        for sm in ts:
            run(sm)
        torch.cuda.synchronize()
        for _ in range(args.driver_reps):
            for sm in ts:
                t0 = time.perf_counter()
                ans = run(sm)
                torch.cuda.synchronize()
                ts[sm].append(time.perf_counter() - t0)
        k = f"{name}_{args.driver_size}"
        res[f"{k}_s"] = float(np.median(ts[None]))
        res[f"{k}_auto_s"] = float(np.median(ts["auto"]))
        res[f"{k}_auto_over_plain"] = res[f"{k}_auto_s"] / res[f"{k}_s"]
        if name == "estimate_translation":
            res[f"{k}_auto_answer"] = [float(v) for v in ans[0].tolist()]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
