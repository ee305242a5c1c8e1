"""Time the 8-bit YUV 4:2:0 ingest / egress kernels and the file-encode path at 1920x1080.

  python scripts/pixfmt_bench.py [--height 1080 --width 1920] [--gops 2 --gop 12] [--json-out PATH]

Kernels: HIP events around `iters` back-to-back launches after a warm-up, per batch size; the bytes
are what the algorithm must move (ingest: 1.5 B/px read of the display area, 12 B/px written of the
coded area; egress: 12 B/px read and 1.5 B/px written of the display area), so GB/s is achieved
bandwidth, to be read against the device's measured float4 copy rate (6.29 TB/s).
File path: encode_file from an in-memory Y4M against container.encode_video (I-frame, compress
chain, payloads: the float-tensor path) and a bare model.compress loop, both over the same frames
already converted to padded float RGB; host clock around work that ends in a device synchronise.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fastvideocodec_amd import container as CT  # noqa: E402
from fastvideocodec_amd import pixfmt as PF  # noqa: E402
from fastvideocodec_amd import video_io as VIO  # noqa: E402
from fastvideocodec_amd.models import get_codec_model  # noqa: E402
from fastvideocodec_amd.synthetic import gop_seed, make_gop  # noqa: E402
from fastvideocodec_amd.transcode import encode_file  # noqa: E402

COPY_RATE_GBS = 6290.0


def event_ms(fn, iters, warmup=5):
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


def kernels(h, w, dev, batches, iters):
    rows = []
    ch, cw = PF.chroma_size(h, w)
    for B in batches:
        g = torch.Generator(device="cpu").manual_seed(B)
        y = torch.randint(0, 256, (B, h, w), dtype=torch.uint8, generator=g).to(dev)
        u = torch.randint(0, 256, (B, ch, cw), dtype=torch.uint8, generator=g).to(dev)
        v = torch.randint(0, 256, (B, ch, cw), dtype=torch.uint8, generator=g).to(dev)
        y2 = torch.randint(0, 256, (B, h, w), dtype=torch.uint8, generator=g).to(dev)
        x, _ = PF.yuv420_to_rgb(y, u, v)
        Hp, Wp = x.shape[2:]
        yuv_bytes = B * (h * w + 2 * ch * cw)
        ms_in = event_ms(lambda: PF.yuv420_to_rgb(y, u, v), iters)
        ms_out = event_ms(lambda: PF.rgb_to_yuv420(x, h, w), iters)
        ms_sse = event_ms(lambda: PF.sse_u8_device(y, y2), iters)
        b_in = yuv_bytes + B * 12 * Hp * Wp
        b_out = yuv_bytes + B * 12 * h * w
        for name, ms, nbytes in (("ingest", ms_in, b_in), ("egress", ms_out, b_out), ("sse_y", ms_sse, 2 * B * h * w)):
            gbs = nbytes / ms / 1e6
            rows.append({"kernel": name, "batch": B, "ms": round(ms, 4), "us_per_frame": round(1e3 * ms / B, 2),
                         "bytes": nbytes, "GBps": round(gbs, 1), "share_of_copy_rate": round(gbs / COPY_RATE_GBS, 3)})
    return rows


def file_path(h, w, dev, gops, gop):
    model = get_codec_model("DVC-pretrained", compression_level=2, device=dev)
    rgb = make_gop(h, w, gop, gop_seed(0))
    x0 = torch.from_numpy(rgb).to(dev)
    y, u, v = (p.cpu().numpy() for p in PF.rgb_to_yuv420(x0, h, w))
    buf = io.BytesIO()
    wr = VIO.Y4MWriter(buf, w, h)
    for _ in range(gops):
        for t in range(gop):
            wr.write(y[t], u[t], v[t])
    src = buf.getvalue()
    n = gops * gop
    # the same frames, already converted: what the float-tensor path is handed
    yd, ud, vd = (torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in (y, u, v))
    x, _ = PF.yuv420_to_rgb(yd, ud, vd)
    video = x[None].expand(gops, *x.shape).contiguous()

    def run_file(batch=1):
        return encode_file(model, VIO.Y4MReader(io.BytesIO(src)), io.BytesIO(), gop=gop, batch=batch)

    def run_tensor():
        CT.encode_video(model, video, io.BytesIO())

    def run_compress():
        for g in range(gops):
            ref = video[g, 0:1]
            for t in range(1, gop):
                _, ref = model.compress(video[g, t:t + 1], ref)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    run_file(), run_tensor(), run_compress()  # warm-up: every shape the timed runs use
    out = {"frames": n, "gop": gop}
    t_file = [wall(run_file) for _ in range(3)]
    t_tensor = [wall(run_tensor) for _ in range(3)]
    t_comp = [wall(run_compress) for _ in range(3)]
    out["encode_file_fps"] = [round(n / t, 2) for t in t_file]
    out["encode_video_fps"] = [round(n / t, 2) for t in t_tensor]
    out["compress_loop_pframes_per_s"] = [round(gops * (gop - 1) / t, 2) for t in t_comp]
    out["conversion_overhead_ms_per_frame"] = round(1e3 * (min(t_file) - min(t_tensor)) / n, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--gops", type=int, default=2)
    ap.add_argument("--gop", type=int, default=12)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 12, 32])
    ap.add_argument("--skip-file", action="store_true")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixfmt_bench needs a GPU: timings taken elsewhere say nothing")
    dev = torch.device("cuda:0")
    res = {"height": a.height, "width": a.width, "copy_rate_GBps": COPY_RATE_GBS,
           "kernels": kernels(a.height, a.width, dev, a.batches, a.iters)}
    if not a.skip_file:
        res["file"] = file_path(a.height, a.width, dev, a.gops, a.gop)
    line = json.dumps(res)
    print(line)
    if a.json_out:
        with open(a.json_out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
