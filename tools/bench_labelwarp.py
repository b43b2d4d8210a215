#!/usr/bin/env python3
"""Time the trilinear label vote (csrc/label_warp.hip) and Dice on label maps (csrc/label_dice.hip) with HIP events beside what
they replace, all in one run, at 128^3 and 256^3 on a map of 14 labels through bench.py's three-axis affine grid
(synthetic.random_affine_matrix(3)):

    warp_labels_u8, warp_labels_i64   kmh_warp_labels on the uint8 / the int64 map (labels only, no weight output)
    nearest_f32                       kmh_grid_sample3d_fwd, mode nearest, on the float32 copy of the map
    chain                             utils.one_hot (14 int64 channels) -> .float() -> align_img -> argmax(1): the reference's route
    label_dice                        loss_ops.label_dice(warped uint8 map, map)
    fast_dice                         loss_ops.fast_dice on the two 14-channel float32 one-hot tensors

    python tools/bench_labelwarp.py [--reps 30] [--window-ms 1.0] [--out profiles/labelwarp_bench.json]

The arms of a size alternate (one timed window of each per round, --reps rounds) and each figure is the median over the rounds.
A window is a number of back-to-back calls between two events, chosen per arm from a first timing so that the window lasts at
least --window-ms (`*_calls_per_window` records it).  Every call of an arm runs on the same buffers: the label maps (2 / 17 MB as
uint8, 17 / 134 MB as int64) and the grid (25 / 201 MB) fit or nearly fit the 256 MB Infinity Cache, so these are WARM-CACHE
times; the chain's tensors at 256^3 (1.9 GB int64, 0.94 GB float32 twice) do not.  chain, label_dice and fast_dice each copy a
few flags or counts to the host inside the call (that is how they are used), so their windows include that wait.
The map: 16^3-voxel blocks with a label drawn per block, so most output voxels see one label at all 8 corners (as in an anatomical
map) and block faces, edges and corners supply the mixed ones.  `*_GBps` = the ALGORITHMIC bytes over the time: 12 B of grid, the
map once and one label out per voxel for the warps.  `warp_labels_*_over_chain` = time over the chain's time."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NLAB = 14


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


def block_map(S, dev, gen):
    """(1, 1, S, S, S) int64: 16^3 blocks, one of NLAB labels per block, every label present"""
    nb = S // 16
    blocks = torch.randint(0, NLAB, (nb, nb, nb), device=dev, generator=gen)
    blocks.view(-1)[:NLAB] = torch.arange(NLAB, device=dev)
    return blocks.repeat_interleave(16, 0).repeat_interleave(16, 1).repeat_interleave(16, 2)[None, None].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window-ms", type=float, default=1.0)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labelwarp_bench.json"))
    args = ap.parse_args()
    from keymorph_amd import _lib, synthetic
    from keymorph_amd.loss_ops import fast_dice, label_dice
    from keymorph_amd.ops import _p, _stream, check
    from keymorph_amd.transformations import AffineTransform
    from keymorph_amd.utils import _encode, align_img, one_hot
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "window_ms": args.window_ms, "labels": NLAB,
           "cache": "warm: every call of an arm reuses the same buffers (256 MB Infinity Cache)",
           "grid": "synthetic.random_affine_matrix(3): rotations about all three axes, shear, scale",
           "map": "16^3 blocks, one label per block"}
    gen = torch.Generator(device=dev).manual_seed(0)
    for S in args.sizes:
        grid = AffineTransform(matrix=synthetic.random_affine_matrix(3, dev), dim=3).get_flow_field((1, 1, S, S, S)).contiguous()
        V = S ** 3
        seg64 = block_map(S, dev, gen)
        seg8, segf = seg64.to(torch.uint8), seg64.float()
        out8, out64, outf = torch.empty_like(seg8), torch.empty_like(seg64), torch.empty_like(segf)
        dims = (1, 1, S, S, S, S, S, S)
        kept = {}

        def chain():
            kept["chain"] = torch.argmax(align_img(grid, one_hot(seg64).float()), 1, keepdim=True)

        check(lib.kmh_warp_labels(_p(seg8), 1, 0, _p(grid), _p(out8), None, *dims, _stream()), "warp_labels")
        warped8 = out8.clone()
        oh_a, oh_b = (_encode(s.contiguous(), np.arange(NLAB), False) for s in (warped8.long(), seg64))     # 14 float32 channels
        arms = {
            "warp_labels_u8": lambda: check(lib.kmh_warp_labels(_p(seg8), 1, 0, _p(grid), _p(out8), None, *dims, _stream()),
                                            "warp_labels"),
            "warp_labels_i64": lambda: check(lib.kmh_warp_labels(_p(seg64), 8, 1, _p(grid), _p(out64), None, *dims, _stream()),
                                             "warp_labels"),
            "nearest_f32": lambda: check(lib.kmh_grid_sample3d_fwd(_p(segf), _p(grid), _p(outf), *dims, 1, _stream()), "nearest"),
            "chain": chain,
            "label_dice": lambda: kept.__setitem__("label_dice", label_dice(warped8, seg8)),
            "fast_dice": lambda: kept.__setitem__("fast_dice", fast_dice(oh_a, oh_b)),
        }
        ms, spread, calls = alternate(arms, args.reps, args.window_ms)
        nbytes = {"warp_labels_u8": (12.0 + 2) * V, "warp_labels_i64": (12.0 + 16) * V, "nearest_f32": (12.0 + 8) * V}
        for name, t in ms.items():
            res[f"{name}_{S}_ms"] = t
            res[f"{name}_{S}_p10_p90_spread_ms"] = spread[name]
            res[f"{name}_{S}_calls_per_window"] = calls[name]
            if name in nbytes:
                res[f"{name}_{S}_GBps"] = nbytes[name] / (t * 1e6)
        for name in ("warp_labels_u8", "warp_labels_i64"):
            res[f"{name}_{S}_over_chain"] = ms[name] / ms["chain"]
            res[f"{name}_{S}_over_nearest"] = ms[name] / ms["nearest_f32"]
        res[f"label_dice_{S}_over_fast_dice"] = ms["label_dice"] / ms["fast_dice"]
        res[f"warp_equals_chain_{S}"] = bool(torch.equal(out8.long(), kept["chain"]) and torch.equal(out64, kept["chain"]))
        res[f"label_dice_equals_fast_dice_{S}"] = bool(kept["label_dice"] == kept["fast_dice"])
        res[f"label_dice_value_{S}"] = kept["label_dice"]
        res[f"share_of_voxels_unlike_nearest_{S}"] = float((out8 != outf.to(torch.uint8)).float().mean())
        res[f"chain_peak_bytes_{S}"] = int(V) * NLAB * (8 + 4 + 4)
        del seg64, seg8, segf, out8, out64, outf, oh_a, oh_b, warped8, kept
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
