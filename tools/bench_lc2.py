#!/usr/bin/env python3
"""Time LC2 / ImageLC2 on the GPU with HIP events: ImageLC2() (51^3 patches, radius 5, mean) on a 256^3 pair and LC2()
(radii 3, 5, 7) on a 255^3 pair, forward and backward separately (gradients for both inputs).

    python tools/bench_lc2.py [--reps 50] [--out FILE]

Each figure is the median over --reps calls.  The backward writes d/d(us) and d/d(mr) for every voxel (two dense fp32
volumes); `bwd_write_TBps` is those bytes over the backward's median time.
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
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keymorph_amd.loss_ops import LC2, ImageLC2
    from tests.test_lc2_cpu import lc2_pair
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev)}
    for key, S, mod in (("imagelc2_256", 256, ImageLC2()), ("lc2_255", 255, LC2())):
        us, mr = lc2_pair(21, 1, S, ("plain",))
        u = torch.tensor(us, device=dev, requires_grad=True)
        m = torch.tensor(mr, device=dev, requires_grad=True)
        out = mod(u, m)
        cot = torch.ones_like(out)
        res[f"{key}_value"] = out.detach().cpu().tolist()
        res[f"{key}_fwd_ms_median"], res[f"{key}_fwd_ms_min"] = timed(lambda: mod(u, m), args.reps)
        res[f"{key}_bwd_ms_median"], res[f"{key}_bwd_ms_min"] = timed(
            lambda: torch.autograd.grad(out, (u, m), cot, retain_graph=True), args.reps)
        res[f"{key}_bwd_write_TBps"] = 2 * u.numel() * 4 / (res[f"{key}_bwd_ms_median"] * 1e9)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
