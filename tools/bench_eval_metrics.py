#!/usr/bin/env python3
"""Time the evaluation metrics on the GPU with HIP events: hausdorff_distance (bs = 1, 256^3, the brain256 volumes of
tests/golden/eval_metrics.npz) and fast_dice (256^3, C = 14, the class count of the align_img legs).

    python tools/bench_eval_metrics.py [--reps 20] [--out FILE]

Each figure is the median over --reps calls of the public function, host work and the result copy included; the
kernel-only time of kmh_hausdorff3d is reported next to it.
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keymorph_amd import _lib, loss_ops
    from keymorph_amd.ops import _p, _stream
    from tests.test_eval_metrics_gpu import param_volume
    g = np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))
    dev = torch.device("cuda", torch.cuda.current_device())
    S = 256
    A = param_volume((S, S, S), g["big::brain256::boxes_a"], g["big::brain256::ell_a"])[None, None].float()
    B = param_volume((S, S, S), g["big::brain256::boxes_b"], g["big::brain256::ell_b"])[None, None].float()
    res = {"device": torch.cuda.get_device_name(dev), "shape": [1, 1, S, S, S]}
    hd = loss_ops.hausdorff_distance(A, B)
    res["hausdorff_value"] = hd
    res["hausdorff_equals_reference"] = hd == float(g["big::brain256::value"])
    res["hausdorff_ms_median"], res["hausdorff_ms_min"] = timed(lambda: loss_ops.hausdorff_distance(A, B), args.reps)
    lib = _lib.load()
    ws = torch.empty(int(lib.kmh_hausdorff3d_ws_bytes(S, S, S)), dtype=torch.uint8, device=dev)
    out = torch.empty(1, dtype=torch.float64, device=dev)
    res["kmh_hausdorff3d_ms_median"], res["kmh_hausdorff3d_ms_min"] = timed(
        lambda: lib.kmh_hausdorff3d(_p(A), _p(B), 0, 0, A.stride(0), B.stride(0), 1, S, S, S, 1.25, 1.25, 10.0, _p(ws),
                                    _p(out), _stream()), args.reps)
    res["hausdorff_ws_bytes"] = int(ws.numel())
    # fast_dice: 14-class soft maps (C = 14, the align_img legs' class count)
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.rand((1, 14, S, S, S), device=dev, generator=gen)
    y = torch.rand((1, 14, S, S, S), device=dev, generator=gen)
    res["fast_dice_value"] = loss_ops.fast_dice(x, y)
    res["fast_dice_ms_median"], res["fast_dice_ms_min"] = timed(lambda: loss_ops.fast_dice(x, y), args.reps)
    res["fast_dice_GBps"] = 2 * x.numel() * 4 / (res["fast_dice_ms_median"] * 1e6)
    res["host_scipy_hausdorff_256_s"] = 12.9     # the reference on the build host's CPU (scipy 1.15.3), not measured here
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
