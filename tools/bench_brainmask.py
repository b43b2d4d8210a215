#!/usr/bin/env python3
"""Time the brain-extraction step (notebooks/[B] Brain Extraction.ipynb of the reference) on the GPU with HIP events, and the
same four steps on the host in the same run:

    resize 256^3 -> 128^3 | Simple_Unet forward at 128^3 (the notebook's channel lists) | x2 upsampling to 256^3 |
    clean_mask at 256^3 on a blob-plus-islands mask

    python tools/bench_brainmask.py [--reps 20] [--host-reps 3] [--out profiles/brainmask_bench.json]

GPU figures: median / minimum over --reps calls of the public function after one warm-up call, HIP events around each call,
a synchronisation after each (clean_mask's includes its own result read-back).  Host figures: torch CPU (F.interpolate, the
network as F.conv3d / F.max_pool3d / F.interpolate) and scipy.ndimage.label + the reference's arithmetic, median over
--host-reps, with the thread count printed.  The resize also reports its achieved bytes/s next to a device copy of the same
number of bytes measured here and the copy rate DESIGN.md quotes (5.1 TB/s).  Recorded, not gated.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENC_NF, DEC_NF = [4, 8, 16, 32], [32, 16, 8, 4]


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


def host_timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def host_unet(sd, x):
    """keymorph/model.py:568-595 with use_in=False on the host"""
    def blk(i, t):
        return F.relu(F.conv3d(t, sd[f"block{i}.conv1.weight"], sd[f"block{i}.conv1.bias"], padding=1))
    skips = []
    for i in range(4):
        x = blk(i, x if i == 0 else F.max_pool3d(x, 2, 2))
        skips.append(x)
    x = blk(4, F.max_pool3d(x, 2, 2))
    for i, s in zip(range(5, 9), skips[::-1]):
        x = blk(i, torch.cat([F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=False), s], 1))
    return F.conv3d(x, sd["conv.weight"], sd["conv.bias"], padding=1)


def blob_mask(S=256):
    """a ball of radius S/4 plus 40 islands of 1 .. 10^3 voxels"""
    z, y, x = np.ogrid[:S, :S, :S]
    m = ((z - S // 2) ** 2 + (y - S // 2) ** 2 + (x - S // 2) ** 2 <= (S // 4) ** 2).astype(np.uint8)
    rng = np.random.RandomState(0)
    for k in range(40):
        e = 1 + k % 10
        c = rng.randint(0, S // 8, size=3) + np.array([(k % 2) * (S - S // 8 - 12), ((k // 2) % 2) * (S - S // 8 - 12), 0])
        m[c[0]:c[0] + e, c[1]:c[1] + e, c[2]:c[2] + e] = 1
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keymorph_amd.model import Simple_Unet, clean_mask
    from keymorph_amd.utils import resize_trilinear
    from tests.brainmask_ref import clean_mask_oracle
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "host_threads": torch.get_num_threads()}
    print("host threads:", res["host_threads"], file=sys.stderr)
    torch.manual_seed(0)
    net = Simple_Unet(1, 1, False, ENC_NF, DEC_NF).eval()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.to(dev)
    img = torch.rand(1, 1, 256, 256, 256)
    x256 = img.to(dev)
    mask = blob_mask(256)
    md = torch.from_numpy(mask).to(dev)

    with torch.no_grad():
        x128 = resize_trilinear(x256, size=(128, 128, 128))
        prob = net(x128)
        # GPU
        res["resize_256_to_128_ms_median"], res["resize_256_to_128_ms_min"] = timed(
            lambda: resize_trilinear(x256, size=(128, 128, 128)), args.reps)
        nbytes = 4 * (x256.numel() + x128.numel())
        res["resize_bytes"] = nbytes
        res["resize_TBps"] = nbytes / (res["resize_256_to_128_ms_median"] * 1e9)
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)
        cp, _ = timed(lambda: dst.copy_(src), args.reps)
        res["copy_same_bytes_TBps"] = nbytes / (cp * 1e9)
        res["copy_rate_quoted_TBps"] = 5.1
        res["unet_fwd_128_ms_median"], res["unet_fwd_128_ms_min"] = timed(lambda: net(x128), args.reps)
        res["upsample_128_to_256_ms_median"], res["upsample_128_to_256_ms_min"] = timed(
            lambda: resize_trilinear(prob, scale_factor=2), args.reps)
        up_bytes = 4 * (prob.numel() * 9)
        res["upsample_TBps"] = up_bytes / (res["upsample_128_to_256_ms_median"] * 1e9)
        res["clean_mask_256_ms_median"], res["clean_mask_256_ms_min"] = timed(lambda: clean_mask(md, 0.2), args.reps)
        out = clean_mask(md, 0.2)
        # host, same run
        res["host_resize_ms"] = host_timed(
            lambda: F.interpolate(img, size=(128, 128, 128), mode="trilinear", align_corners=False), args.host_reps)
        h128 = F.interpolate(img, size=(128, 128, 128), mode="trilinear", align_corners=False)
        res["host_unet_fwd_128_ms"] = host_timed(lambda: host_unet(sd, h128), args.host_reps)
        hprob = host_unet(sd, h128)
        res["host_upsample_ms"] = host_timed(
            lambda: F.interpolate(hprob, scale_factor=2, mode="trilinear", align_corners=False), args.host_reps)
        res["host_clean_mask_ms"] = host_timed(lambda: clean_mask_oracle(mask, 0.2), args.host_reps)
        res["clean_mask_equals_host"] = bool(np.array_equal(out.cpu().numpy(), clean_mask_oracle(mask, 0.2)))
        res["unet_max_abs_diff_vs_host"] = float((prob.cpu() - hprob).abs().max())
        res["mask_voxels_set"] = int(mask.sum())
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
