#!/usr/bin/env python3
"""Time the velocity-field exponential (csrc/svf.hip, ops.svf_grid) with HIP events on the bench's synthetic pair
(synthetic.make_pair), a rotation + shear + shift matrix, control spacing 8 and K = 6 squarings, at 128^3 and 256^3, all in one
process, each beside two baselines whose calls alternate with its own inside every repetition:

  forward     ops.svf_grid | ops.bspline_grid | the chain of existing operators, K times
                  u + align_img(identity_grid + u, u.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)
  backward    the same three graphs, backward alone (the graph is kept between repetitions), from one cotangent of the grid; the
              chain's is torch autograd through grid_sample3d, whose volume gradient is a float-atomic scatter -- the only way to
              this gradient before ops.svf_grid, and not reproducible bit for bit
  entries     the library calls of one svf_grid forward + backward, by entry point (the library's own event profiler)
  step        one optimisation step of io.register_svf at full size: svf_grid -> align_img -> mutual_information (ranges given)
              + bending * bspline_bending, backward to the lattice; beside register_bspline's step
  register    one io.register_svf(fixed, moving, mat) with its defaults at 128^3 (median of --est-reps calls), beside
              io.register_bspline

    python tools/bench_svf.py [--reps 20] [--out profiles/svf_bench.json]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--spacing", type=int, default=8)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--est-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keymorph_amd import _lib, fields, ops, synthetic
    from keymorph_amd.io import register_bspline, register_svf
    from keymorph_amd.utils import align_img
    dev = torch.device("cuda", torch.cuda.current_device())
    B, K = args.bins, args.steps
    res = {"device": torch.cuda.get_device_name(dev), "bins": B, "spacing": args.spacing, "steps": K, "reps": args.reps,
           "register_reps": args.est_reps}
    for S in args.sizes:
        f, m = synthetic.make_pair(S, 0, dev)
        dims = (S, S, S)
        lat = ops.bspline_lattice_shape(dims, args.spacing)
        mat = synthetic.random_affine_matrix(3, dev)[:, :3, :].contiguous()
        g = torch.Generator().manual_seed(S)
        ctrl = (0.02 * torch.randn(1, 3, *lat, generator=g)).to(dev)
        dgrid = torch.randn(1, S, S, S, 3, generator=g).to(dev)
        ids = fields.identity_grid((1, 1, *dims), dev)
        k = f"svf_{S}"
        res[f"{k}_lattice"] = list(lat)
        res[f"{k}_saved_mb"] = 12.0 * S ** 3 * K / 1e6
        res[f"{k}_ws_mb"] = 32.0 * S ** 3 / 1e6

        def chain(u):
            for _ in range(K):
                u = u + align_img(ids + u, u.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)
            return ids + u

        with torch.no_grad():
            u0 = ops.svf_displacement(ctrl * 2.0 ** -K, dims, 0)
            arms = [lambda: ops.svf_grid(ctrl, dims, K, mat), lambda: ops.svf_grid(ctrl, dims, K),
                    lambda: ops.bspline_grid(ctrl, dims, mat), lambda: chain(u0)]
            (res[f"{k}_fwd_ms"], res[f"{k}_fwd_nomat_ms"], res[f"{k}_bspline_fwd_ms"], res[f"{k}_chain_fwd_ms"]) = \
                alternating(arms, args.reps)
            assert torch.equal(ops.svf_grid(ctrl, dims, K), chain(u0))

        c1, c2, u1 = ctrl.clone().requires_grad_(), ctrl.clone().requires_grad_(), u0.clone().requires_grad_()
        g_svf, g_ffd, g_chain = ops.svf_grid(c1, dims, K, mat), ops.bspline_grid(c2, dims, mat), chain(u1)
        arms = [lambda: torch.autograd.grad(g_svf, c1, dgrid, retain_graph=True),
                lambda: torch.autograd.grad(g_ffd, c2, dgrid, retain_graph=True),
                lambda: torch.autograd.grad(g_chain, u1, dgrid, retain_graph=True)]
        res[f"{k}_bwd_ms"], res[f"{k}_bspline_bwd_ms"], res[f"{k}_chain_bwd_ms"] = alternating(arms, args.reps)
        # two backward passes of each: bit-identical, or not
        a, b = arms[0]()[0], arms[0]()[0]
        res[f"{k}_bwd_repeats_bitwise"] = bool(torch.equal(a, b))
        a, b = arms[2]()[0], arms[2]()[0]
        res[f"{k}_chain_bwd_repeats_bitwise"] = bool(torch.equal(a, b))
        del g_svf, g_ffd, g_chain, a, b

        _lib.profiler.reset()
        _lib.profiler.enabled = True
        cp = ctrl.clone().requires_grad_()
        ops.svf_grid(cp, dims, K, mat).backward(dgrid)
        _lib.profiler.enabled = False
        res[f"{k}_entries_ms"] = {n: {"calls": d["calls"], "ms": round(d["ms"], 4)} for n, d in _lib.profiler.summary().items()}
        _lib.profiler.reset()

        rng = ops.mi_ranges(m, f, B)
        q = (ctrl * (S / 2.0)).requires_grad_(True)

        def step(grid_of):
            def run():
                q.grad = None
                warped = align_img(grid_of(q * (2.0 / S)), m)
                (0.05 * ops.bspline_bending(q) - ops.mutual_information(warped, f, B, ranges=rng)).sum().backward()
            return run

        res[f"{k}_step_ms"], res[f"{k}_bspline_step_ms"] = alternating(
            [step(lambda c: ops.svf_grid(c, dims, K, mat)), step(lambda c: ops.bspline_grid(c, dims, mat))], args.reps)
        if S == 128:
            res[f"{k}_register_ms"] = timed(lambda: register_svf(f, m, mat=mat, control_spacing=args.spacing, steps=K, bins=B),
                                            args.est_reps)
            res[f"{k}_bspline_register_ms"] = timed(lambda: register_bspline(f, m, mat=mat, control_spacing=args.spacing, bins=B),
                                                    args.est_reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
