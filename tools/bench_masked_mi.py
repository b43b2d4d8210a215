#!/usr/bin/env python3
"""Time the masked mutual-information kernels (csrc/mi.hip, csrc/warp_mi.hip) against the unmasked ones they stand beside, with
HIP events on the bench's synthetic pair (synthetic.make_pair) and a rotation + shear + shift matrix, at 128^3 and 256^3, all
in one process.  Per size, each launch on its own, the arms of one group alternating inside every repetition, medians over
--reps (the 10th and 90th percentiles are kept beside them as `_p10` / `_p90`):

  hist        kmh_mi_hist_ranges                      against kmh_mi_hist_masked       with mask = ones | ball
  warp_hist   kmh_warp_mi_hist                        against kmh_warp_mi_hist_masked  with ones (fixed) | ball (fixed) | ball (both)
  warp_bwd    kmh_warp_mi_bwd                         against kmh_warp_mi_bwd_masked   with the same three

ball = the centred ball of radius 0.4 size (about 27 % of the box).  `*_counted` is the share of voxels the masked pass counted,
`*_ones_equal` records that the mask of ones returned the unmasked MI bit for bit on the timed inputs.

    python tools/bench_masked_mi.py [--reps 30] [--bins 32] [--out profiles/masked_mi_bench.json]
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


def alternating(fns, reps):
    """Per arm (median, p10, p90) in ms; the arms' calls alternate inside every repetition, after three warm-up rounds."""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(event_ms(fn))
    return {k: tuple(float(np.percentile(t, q)) for q in (50, 10, 90)) for k, t in ts.items()}


def ball_mask(S, dev):
    ax = torch.arange(S, dtype=torch.float32, device=dev) - (S - 1) / 2
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    return ((z * z + y * y + x * x) <= (0.4 * S) ** 2).to(torch.uint8)[None, None].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keymorph_amd import _lib, ops, synthetic
    from keymorph_amd.ops import _p, _stream, check
    from keymorph_amd.utils import align_img
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = args.bins
    res = {"device": torch.cuda.get_device_name(dev), "bins": B, "reps": args.reps}
    for S in args.sizes:
        f, m = synthetic.make_pair(S, 0, dev)
        V = S ** 3
        mat = synthetic.random_affine_matrix(3, dev)[:, :3, :].contiguous()
        rng = ops.mi_ranges(m, f, B)
        warped = align_img(ops.affine_grid(mat, (S, S, S)), m)
        ones, ball = torch.ones_like(ball_mask(S, dev)), ball_mask(S, dev)
        ws = torch.empty(int(lib.kmh_warp_mi_ws_bytes(1, B, S, S, S)), dtype=torch.uint8, device=dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        mi = torch.empty(1, dtype=torch.float32, device=dev)
        G = torch.empty((1, B, B), dtype=torch.float32, device=dev)
        gout = torch.ones(1, dtype=torch.float32, device=dev)
        dmat = torch.empty_like(mat)
        s = _stream()
        k = f"masked_mi_{S}"
        res[f"{k}_ball_share"] = float(ball.float().mean())

        def hist(mask):
            return lambda: check(lib.kmh_mi_hist_masked(_p(warped), _p(f), _p(mask), _p(rng), 1, V, B, _p(ws), _p(cnt), s), "hist_masked")

        def warp_hist(fm, mm):
            return lambda: check(lib.kmh_warp_mi_hist_masked(_p(m), _p(f), _p(fm), _p(mm), _p(mat), _p(rng), 1, S, S, S, B, 0, _p(ws),
                                                             _p(cnt), s), "warp_hist_masked")

        def final(masked):
            if masked:
                check(lib.kmh_mi_final_masked(_p(ws), _p(rng), _p(cnt), 1, B, _p(mi), _p(G), s), "final_masked")
            else:
                check(lib.kmh_mi_final(_p(ws), _p(rng), 1, V, B, _p(mi), _p(G), s), "final")
            return mi.clone()

        groups = {
            "hist": {"unmasked": lambda: check(lib.kmh_mi_hist_ranges(_p(warped), _p(f), _p(rng), 1, V, B, _p(ws), s), "hist"),
                     "ones": hist(ones), "ball": hist(ball)},
            "warp_hist": {"unmasked": lambda: check(lib.kmh_warp_mi_hist(_p(m), _p(f), _p(mat), _p(rng), 1, S, S, S, B, _p(ws), s),
                                                    "warp_hist"),
                          "ones": warp_hist(ones, None), "ball": warp_hist(ball, None), "ball_both": warp_hist(ball, ball)},
        }
        for group, arms in groups.items():
            for arm, (med, lo, hi) in alternating(arms, args.reps).items():
                res[f"{k}_{group}_{arm}_ms"], res[f"{k}_{group}_{arm}_p10"], res[f"{k}_{group}_{arm}_p90"] = med, lo, hi
            arms["unmasked"]()
            plain = final(False)
            arms["ones"]()
            res[f"{k}_{group}_ones_equal"] = bool(torch.equal(plain, final(True)))
            for arm in arms:
                if arm not in ("unmasked", "ones"):
                    arms[arm]()
                    torch.cuda.synchronize()
                    res[f"{k}_{group}_{arm}_counted"] = int(cnt[0]) / V
        # the backward passes read G and the count of their own histogram pass: G of the unmasked table serves all arms (the time
        # does not depend on its values); the count is set by a histogram pass with the arm's masks right before the arm is timed
        groups["warp_hist"]["unmasked"]()
        final(False)
        bwd = {"unmasked": (None, lambda: check(lib.kmh_warp_mi_bwd(_p(m), _p(f), _p(mat), _p(rng), _p(G), _p(gout), 1, S, S, S, B,
                                                                     _p(ws), _p(dmat), s), "warp_bwd")),
               "ones": (ones, None), "ball": (ball, None), "ball_both": (ball, ball)}
        cnts = {}
        for arm, masks in bwd.items():
            if arm != "unmasked":
                warp_hist(*masks)()
                cnts[arm] = cnt.clone()
        arms = {"unmasked": bwd["unmasked"][1]}
        for arm, masks in bwd.items():
            if arm != "unmasked":
                def run(masks=masks, c=cnts[arm]):
                    check(lib.kmh_warp_mi_bwd_masked(_p(m), _p(f), _p(masks[0]), _p(masks[1]), _p(mat), _p(rng), _p(G), _p(gout), _p(c),
                                                     1, S, S, S, B, 0, _p(ws), _p(dmat), s), "warp_bwd_masked")
                arms[arm] = run
        for arm, (med, lo, hi) in alternating(arms, args.reps).items():
            res[f"{k}_warp_bwd_{arm}_ms"], res[f"{k}_warp_bwd_{arm}_p10"], res[f"{k}_warp_bwd_{arm}_p90"] = med, lo, hi
        arms["unmasked"]()
        plain = dmat.clone()
        arms["ones"]()
        res[f"{k}_warp_bwd_ones_equal"] = bool(torch.equal(plain, dmat))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
