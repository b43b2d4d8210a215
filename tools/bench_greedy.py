#!/usr/bin/env python3
"""Time the dense displacement model (csrc/dense.hip) and the greedy iteration built on it with HIP events on the bench's synthetic
pair (synthetic.make_pair) at 128^3 and 256^3, all in one process.  Every figure is the median of --windows windows; a window
repeats its call until it lasts at least a millisecond, and the arms of a comparison alternate inside every repetition.

  kernels     ops.displacement_grid forward (with a matrix) and backward, ops.displacement_step_scale, ops.displacement_update, each
              with the bytes it has to move (24, 24, 12 and 24 B per voxel; the update's 24 gathered values come on top) and the rate
  iteration   one iteration of io.register_greedy at full size with mutual information (ranges given), no matrix:
                  displacement_grid -> align_img -> mutual_information -> autograd -> gaussian_smooth -> displacement_step_scale
                  -> displacement_update -> gaussian_smooth
              beside the same iteration as the chain of the operators that existed before: the grid from torch's permute / flip /
              add of fields.identity_grid (fields.from_displacement carries no gradient), a host-side amax of the norms for the
              step, and  d + align_img(fields.from_displacement(d), disp)  with C = 3 for the composition
  register    one io.register_greedy(fixed, moving, mat) with its defaults at 128^3 (median of --est-reps calls), beside
              io.register_bspline

    python tools/bench_greedy.py [--windows 30] [--out profiles/greedy_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternating(fns, windows, warmup=3, min_ms=1.0):
    """Medians (ms per call) of several arms whose windows alternate inside every repetition; an arm's window repeats its call
    until it lasts min_ms."""
    calls = []
    for fn in fns:
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        once = max(window_ms(fn, 1), 1e-3)
        calls.append(max(1, int(np.ceil(min_ms / once))))
    ts = [[] for _ in fns]
    for _ in range(windows):
        for k, fn in enumerate(fns):
            ts[k].append(window_ms(fn, calls[k]))
    return [float(np.median(t)) for t in ts]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    return float(np.median([window_ms(fn, 1) for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--est-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_greedy.py: no GPU")
    from keymorph_amd import fields, ops, synthetic
    from keymorph_amd.io import register_bspline, register_greedy
    from keymorph_amd.utils import align_img
    dev = torch.device("cuda", torch.cuda.current_device())
    B, step, su, st = args.bins, 0.5, 3 ** 0.5, 0.5 ** 0.5
    res = {"device": torch.cuda.get_device_name(dev), "bins": B, "windows": args.windows, "window_min_ms": 1.0, "step": step,
           "sigma_update": su, "sigma_total": st, "register_reps": args.est_reps}
    for S in args.sizes:
        f, m = synthetic.make_pair(S, 0, dev)
        V = S ** 3
        mat = synthetic.random_affine_matrix(3, dev)[:, :3, :].contiguous()
        g = torch.Generator().manual_seed(S)
        disp = ops.gaussian_smooth((3.0 * torch.randn(1, 3, S, S, S, generator=g)).to(dev), 2.0) * 4
        delta = ops.gaussian_smooth(torch.randn(1, 3, S, S, S, generator=g).to(dev), su)
        dgrid = torch.randn(1, S, S, S, 3, generator=g).to(dev)
        scale = ops.displacement_step_scale(delta, step)
        k = f"greedy_{S}"
        res[f"{k}_max_disp_vox"] = float(disp.abs().max())

        # ---- the kernels ---------------------------------------------------------------------------------------------------
        dg = disp.clone().requires_grad_()
        grid = ops.displacement_grid(dg, mat)
        with torch.no_grad():
            fwd = lambda: ops.displacement_grid(disp, mat)                                    # noqa: E731
            fwd0 = lambda: ops.displacement_grid(disp)                                        # noqa: E731
            old0 = lambda: fields.from_displacement(disp)                                     # noqa: E731
            bwd = lambda: torch.autograd.grad(grid, dg, dgrid, retain_graph=True)             # noqa: E731
            ssc = lambda: ops.displacement_step_scale(delta, step)                            # noqa: E731
            upd = lambda: ops.displacement_update(disp, delta, scale)                         # noqa: E731
            d1 = delta * scale[:, None, None, None, None]
            upd_chain = lambda: d1 + align_img(fields.from_displacement(d1), disp)            # noqa: E731
            names = ["grid_fwd", "grid_fwd_nomat", "from_displacement", "grid_bwd", "step_scale", "update", "update_chain"]
            nbytes = [24, 24, 24, 24, 12, 24, None]
            for name, t, nb in zip(names, alternating([fwd, fwd0, old0, bwd, ssc, upd, upd_chain], args.windows), nbytes):
                res[f"{k}_{name}_ms"] = t
                if nb:
                    res[f"{k}_{name}_gbps"] = nb * V / t / 1e6
            assert torch.equal(upd(), upd_chain()) and torch.equal(fwd0(), old0())
        del grid, dg

        # ---- one iteration -------------------------------------------------------------------------------------------------
        rng = ops.mi_ranges(m, f, B)
        ids = fields.identity_grid((1, 1, S, S, S), dev)
        d0 = (0.25 * disp).contiguous()

        def iteration(mt):
            def run():
                d = d0.detach().requires_grad_(True)
                warped = align_img(ops.displacement_grid(d, mt), m)
                (gr,) = torch.autograd.grad(ops.mutual_information(warped, f, B, ranges=rng).sum(), d)
                with torch.no_grad():
                    gr = ops.gaussian_smooth(gr, su)
                    return ops.gaussian_smooth(ops.displacement_update(d0, gr, ops.displacement_step_scale(gr, step)), st)
            return run

        def chain():
            d = d0.detach().requires_grad_(True)
            u = torch.stack([d[:, 2] * (2.0 / S), d[:, 1] * (2.0 / S), d[:, 0] * (2.0 / S)], dim=-1)
            warped = align_img(ids + u, m)
            (gr,) = torch.autograd.grad(ops.mutual_information(warped, f, B, ranges=rng).sum(), d)
            with torch.no_grad():
                gr = ops.gaussian_smooth(gr, su)
                longest = float(gr.pow(2).sum(dim=1).amax().sqrt())                           # the host waits here
                dl = gr * (step / longest if longest > 0 else 0.0)
                return ops.gaussian_smooth(dl + align_img(fields.from_displacement(dl), d0), st)

        res[f"{k}_iteration_ms"], res[f"{k}_iteration_mat_ms"], res[f"{k}_chain_iteration_ms"] = alternating(
            [iteration(None), iteration(mat), chain], args.windows)
        res[f"{k}_iteration_vs_chain_max_abs_vox"] = float((iteration(None)() - chain()).abs().max())

        if S == 128:
            res[f"{k}_register_ms"] = timed(lambda: register_greedy(f, m, mat=mat, bins=B), args.est_reps)
            res[f"{k}_bspline_register_ms"] = timed(lambda: register_bspline(f, m, mat=mat, bins=B), args.est_reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
