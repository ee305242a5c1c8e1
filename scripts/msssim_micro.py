"""Time the fused MS-SSIM kernel against the same computation in torch ops on the same GPU and
against the bytes it must move, and the file path with and without --msssim.

  python scripts/msssim_micro.py [--out DIR] [--iters N] [--frames N] [--skip-file]

Device events around N calls after warm-up; the torch formulation (grouped F.conv2d + avg_pool2d in
float32, a direct restatement of the reference) is the path a user would otherwise take. The byte
count is both inputs once per scale plus the pooled planes written once, over the project's measured
6.29 TB/s copy rate. Fails without a GPU. Writes msssim_micro.json and prints a markdown table."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from fastvideocodec_amd import metrics as MT  # noqa: E402
from fastvideocodec_amd import video_io as VIO  # noqa: E402

COPY_TBS = 6.29


def torch_ms_ssim(x, y, data_range):
    C = x.shape[1]
    win = torch.tensor(MT.TAPS, dtype=torch.float32, device=x.device).reshape(1, 1, 1, 11).repeat(C, 1, 1, 1)
    w = torch.tensor(MT.WEIGHTS, device=x.device)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    blur = lambda t: F.conv2d(F.conv2d(t, win, groups=C), win.transpose(2, 3), groups=C)  # noqa: E731
    mcs = []
    for _ in range(5):
        mu1, mu2 = blur(x), blur(y)
        m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        s1, s2, s12 = blur(x * x) - m11, blur(y * y) - m22, blur(x * y) - m12
        cs = (2 * s12 + c2) / (s1 + s2 + c2)
        ss = ((2 * m12 + c1) / (m11 + m22 + c1)) * cs
        mcs.append(cs.mean((1, 2, 3)))
        pad = (x.shape[2] % 2, x.shape[3] % 2)
        x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
    return torch.prod(torch.stack(mcs[:-1]) ** w[:-1, None], 0) * ss.mean((1, 2, 3)) ** (4 * w[-1])


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def min_bytes(planes, h, w, esize):
    n, total = planes * h * w, 0
    for l in range(5):
        total += 2 * n * (esize if l == 0 else 4)          # both inputs of this scale, once
        h, w = (h + 1) // 2, (w + 1) // 2
        n = planes * h * w
        if l < 4:
            total += 2 * n * 4                               # the pooled planes, written
    return total


def kernel_cases(iters):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1)
    rows = []
    for name, shape, dtype in (("12 x 3x1080x1920 float32", (12, 3, 1080, 1920), torch.float32),
                               ("12 x 1x1080x1920 uint8 (Y planes)", (12, 1, 1080, 1920), torch.uint8)):
        x8 = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        y8 = (x8.int() + torch.randint(-4, 5, shape, generator=g)).clamp(0, 255).to(torch.uint8)
        if dtype == torch.float32:
            x, y, dr = (x8.float() / 255).to(dev), (y8.float() / 255).to(dev), 1.0
            xt, yt = x, y
        else:
            x, y, dr = x8.to(dev), y8.to(dev), 255.0
            xt, yt = x.float(), y.float()                    # torch ops have no uint8 conv: conversion not timed
        q = MT.ms_ssim(x, y, dr)
        qt = torch_ms_ssim(xt, yt, dr)
        fused = timed(lambda: MT.ms_ssim(x, y, dr), iters)
        ops = timed(lambda: torch_ms_ssim(xt, yt, dr), max(2, iters // 4), warmup=1)
        planes = shape[0] * shape[1]
        nb = min_bytes(planes, shape[2], shape[3], x.element_size())
        rows.append({"case": name, "fused_ms": fused, "torch_ops_ms": ops, "min_bytes": nb,
                     "bytes_floor_ms": nb / (COPY_TBS * 1e12) * 1e3, "fused_gbs": nb / fused / 1e6,
                     "max_abs_diff_vs_torch_f32": float((q - qt.double()).abs().max())})
    return rows


def file_case(nframes):
    from fastvideocodec_amd.models import get_codec_model
    from fastvideocodec_amd.transcode import encode_file
    dev = torch.device("cuda:0")
    model = get_codec_model("DVC-pretrained", compression_level=2, device=dev)
    rng = np.random.Generator(np.random.PCG64(3))
    base = rng.integers(16, 236, size=(1080 // 8 + 1, 1920 // 8 + 1), dtype=np.uint8)
    y0 = np.repeat(np.repeat(base, 8, 0), 8, 1)[:1080, :1920]
    buf = io.BytesIO()
    wr = VIO.Y4MWriter(buf, 1920, 1080)
    for t in range(nframes):
        wr.write(np.roll(y0, 2 * t, axis=1), np.full((540, 960), 128, np.uint8), np.full((540, 960), 128, np.uint8))
    src = buf.getvalue()
    out = {}
    for rep in range(3):  # alternate the two on the same tree; the first pair is warm-up
        for flag in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            encode_file(model, VIO.Y4MReader(io.BytesIO(src)), io.BytesIO(), gop=12, msssim=flag)
            torch.cuda.synchronize()
            if rep:
                out.setdefault(flag, []).append(nframes / (time.perf_counter() - t0))
    return {"frames": nframes, "fps_without": out[False], "fps_with_msssim": out[True]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "bench_out"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--skip-file", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msssim_micro needs a GPU: nothing is measured without one")
    res = {"kernel": kernel_cases(a.iters), "file": None if a.skip_file else file_case(a.frames)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "msssim_micro.json"), "w") as f:
        json.dump(res, f, indent=1)
    print("| case | fused kernel, ms | torch ops, ms | bytes floor at 6.29 TB/s, ms | fused, GB/s of the needed bytes |")
    print("|---|---|---|---|---|")
    for r in res["kernel"]:
        print(f"| {r['case']} | {r['fused_ms']:.3f} | {r['torch_ops_ms']:.3f} | {r['bytes_floor_ms']:.3f} | "
              f"{r['fused_gbs']:.0f} |")
    if res["file"]:
        print(json.dumps(res["file"]))


if __name__ == "__main__":
    main()
