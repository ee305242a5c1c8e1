"""Time the frame digest kernel and what stamping / self-checking costs the file-encode path.

  python scripts/digest_bench.py [--height 1080 --width 1920] [--gops 2 --gop 12] [--json-out PATH]

Kernel: HIP events around `iters` back-to-back fvc_frame_digest_f32 launches after a warm-up
(event_ms of pixfmt_bench.py), over B frames of the coded size per launch; it reads 4 * n bytes per
frame once, so GB/s is achieved bandwidth, to be read against the device's measured float4 copy rate
(6.29 TB/s). The time includes the call's 8 * B byte hipMemsetAsync.
File path: transcode.encode_file from an in-memory Y4M, plain / digest / digest + self_check taken
in turn, `repeats` times, after a warm-up of each; host clock around work that ends in a device
synchronise.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fastvideocodec_amd import digest as DG  # noqa: E402
from fastvideocodec_amd import pixfmt as PF  # noqa: E402
from fastvideocodec_amd import video_io as VIO  # noqa: E402
from fastvideocodec_amd.models import get_codec_model  # noqa: E402
from fastvideocodec_amd.synthetic import gop_seed, make_gop  # noqa: E402
from fastvideocodec_amd.transcode import encode_file  # noqa: E402
from pixfmt_bench import COPY_RATE_GBS, event_ms  # noqa: E402

VARIANTS = {"plain": {}, "digest": {"digest": True}, "digest_self_check": {"digest": True, "self_check": True}}


def kernel(h, w, dev, batches, iters):
    Hp, Wp = -(-h // 64) * 64, -(-w // 64) * 64
    rows = []
    for B in batches:
        x = torch.rand((B, 3, Hp, Wp), dtype=torch.float32, device=dev, generator=torch.Generator(dev).manual_seed(B))
        ms = event_ms(lambda: DG.frame_digest(x), iters)
        nbytes = x.numel() * 4
        gbs = nbytes / ms / 1e6
        rows.append({"batch": B, "coded": [Hp, Wp], "ms": round(ms, 4), "us_per_frame": round(1e3 * ms / B, 2),
                     "bytes": nbytes, "GBps": round(gbs, 1), "share_of_copy_rate": round(gbs / COPY_RATE_GBS, 3)})
    return rows


def file_path(h, w, dev, gops, gop, repeats):
    model = get_codec_model("DVC-pretrained", compression_level=2, device=dev)
    x0 = torch.from_numpy(make_gop(h, w, gop, gop_seed(0))).to(dev)
    y, u, v = (p.cpu().numpy() for p in PF.rgb_to_yuv420(x0, h, w))
    buf = io.BytesIO()
    wr = VIO.Y4MWriter(buf, w, h)
    for _ in range(gops):
        for t in range(gop):
            wr.write(y[t], u[t], v[t])
    src = buf.getvalue()
    n = gops * gop

    def wall(kw):
        out = io.BytesIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        encode_file(model, VIO.Y4MReader(io.BytesIO(src)), out, gop=gop, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out.getvalue()

    sizes = {name: len(wall(kw)[1]) for name, kw in VARIANTS.items()}  # warm-up of every variant
    times = {name: [] for name in VARIANTS}
    for _ in range(repeats):
        for name, kw in VARIANTS.items():
            times[name].append(wall(kw)[0])
    out = {"frames": n, "gop": gop, "bytes": sizes,
           "encode_file_fps": {name: [round(n / t, 2) for t in ts] for name, ts in times.items()}}
    best = {name: min(ts) for name, ts in times.items()}
    out["ms_per_frame_over_plain"] = {name: round(1e3 * (best[name] - best["plain"]) / n, 3)
                                      for name in VARIANTS if name != "plain"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--gops", type=int, default=2)
    ap.add_argument("--gop", type=int, default=12)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 12])
    ap.add_argument("--skip-file", action="store_true")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("digest_bench needs a GPU: timings taken elsewhere say nothing")
    dev = torch.device("cuda:0")
    res = {"height": a.height, "width": a.width, "copy_rate_GBps": COPY_RATE_GBS,
           "kernel": kernel(a.height, a.width, dev, a.batches, a.iters)}
    if not a.skip_file:
        res["file"] = file_path(a.height, a.width, dev, a.gops, a.gop, a.repeats)
    line = json.dumps(res)
    print(line)
    if a.json_out:
        with open(a.json_out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
