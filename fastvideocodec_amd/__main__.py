"""Command line: python -m fastvideocodec_amd encode | decode | verify | info | compare.

  encode IN.y4m|IN.yuv OUT.fvc [--size WxH] [--gop N] [--level L] [--checkpoint PATH]
         [--matrix bt601|bt709] [--range limited|full] [--batch G]
         [--digest] [--self-check] [--msssim]                          prints one JSON line of stats
  decode IN.fvc OUT.y4m [--checkpoint PATH] [--no-verify]              prints one JSON line
  verify IN.fvc [--checkpoint PATH]                                    decodes without writing; one JSON line
  info   IN.fvc                                                        header and record counts (no GPU)
  compare A.y4m|A.yuv B.y4m|B.yuv [--size WxH]                         per-frame psnr_y/u/v and msssim_y of two files

--digest stamps every record with a digest of the encoder's reconstruction; decode checks each frame
against it unless --no-verify, and fails at the first frame that differs. --self-check makes the
encoder decode the bytes it has just serialised and compare (the file does not change).
verify exits 0 when every frame matches, 1 at a mismatch, 2 when the file carries no digests.
--msssim adds msssim_y, the per-frame MS-SSIM of the Y planes (8-bit, data range 255, display size).
compare measures two files of equal geometry frame by frame (the shorter one sets the count) and
exits 2 when their sizes differ; msssim_y is null for frames smaller than 176 on a side.
"""
from __future__ import annotations

import argparse
import json
import sys


def _model(level, checkpoint):
    import torch

    from .models import get_codec_model
    if not torch.cuda.is_available():
        raise SystemExit("encode / decode need a GPU (the codec has no CPU path)")
    return get_codec_model("DVC-pretrained", compression_level=level, checkpoint=checkpoint,
                           device=torch.device("cuda:0"))


def _size(s):
    try:
        w, h = s.lower().split("x")
        return int(w), int(h)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected WxH, got {s!r}")


def _compare(a) -> int:
    """Two files of equal geometry, frame by frame: the exact 8-bit PSNR of each plane and the
    MS-SSIM of the Y planes. With a GPU both are queued on the device and read once at the end;
    without one the squared errors are integer sums on the host and the MS-SSIM is the float64
    restatement (metrics.ms_ssim_reference)."""
    import numpy as np
    import torch

    from . import metrics as MT
    from . import pixfmt as PF
    from .video_io import open_video
    with open_video(a.a, a.size) as ra, open_video(a.b, a.size) as rb:
        if (ra.width, ra.height) != (rb.width, rb.height):
            print(f"geometry mismatch: {a.a} is {ra.width}x{ra.height}, {a.b} is {rb.width}x{rb.height}",
                  file=sys.stderr)
            return 2
        gpu = torch.cuda.is_available()
        dev = torch.device("cuda:0" if gpu else "cpu")
        h, w = ra.height, ra.width
        ms = min(h, w) >= MT.min_side(5)
        rows = []
        for fa, fb in zip(ra, rb):
            pa = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in fa]
            pb = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in fb]
            if gpu:
                m = [PF.sse_u8_device(x, y) for x, y in zip(pa, pb)]
            else:
                m = [((x.long() - y.long()) ** 2).sum().reshape(1) for x, y in zip(pa, pb)]
            if ms:
                m.append(MT.ms_ssim(pa[0][None, None], pb[0][None, None], data_range=255).view(torch.int64))
            rows.append(torch.cat(m))
    if not rows:
        raise SystemExit("no frame to compare")
    s = torch.stack(rows).cpu().numpy()  # the one host wait
    ch, cw = PF.chroma_size(h, w)
    res = {"frames": len(rows), "height": h, "width": w}
    for k, (key, npx) in enumerate((("psnr_y", h * w), ("psnr_u", ch * cw), ("psnr_v", ch * cw))):
        res[key] = [PF.psnr_from_sse(int(v), npx) for v in s[:, k]]
    res["msssim_y"] = np.ascontiguousarray(s[:, 3]).view(np.float64).tolist() if ms else None
    print(json.dumps(res, sort_keys=True))
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m fastvideocodec_amd", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("encode", help="8-bit 4:2:0 Y4M / raw I420 -> FVC1 container")
    e.add_argument("src")
    e.add_argument("dst")
    e.add_argument("--size", type=_size, default=None, help="WxH of a raw .yuv source")
    e.add_argument("--gop", type=int, default=12)
    e.add_argument("--level", type=int, default=2)
    e.add_argument("--checkpoint", default=None)
    e.add_argument("--matrix", choices=("bt601", "bt709"), default="bt709")
    e.add_argument("--range", choices=("limited", "full"), default="limited")
    e.add_argument("--batch", type=int, default=1)
    e.add_argument("--digest", action="store_true", help="stamp every record with its reconstruction digest")
    e.add_argument("--self-check", action="store_true",
                   help="decode every serialised payload and compare its digest with the encoder's")
    e.add_argument("--msssim", action="store_true", help="also report the per-frame MS-SSIM of the Y planes")
    d = sub.add_parser("decode", help="FVC1 container -> Y4M")
    d.add_argument("src")
    d.add_argument("dst")
    d.add_argument("--checkpoint", default=None)
    d.add_argument("--no-verify", action="store_true", help="do not check the frame digests the file carries")
    v = sub.add_parser("verify", help="decode without writing and check every frame digest")
    v.add_argument("src")
    v.add_argument("--checkpoint", default=None)
    i = sub.add_parser("info", help="print a container's header and record counts")
    i.add_argument("src")
    c = sub.add_parser("compare", help="per-frame PSNR and MS-SSIM of two 8-bit 4:2:0 files")
    c.add_argument("a")
    c.add_argument("b")
    c.add_argument("--size", type=_size, default=None, help="WxH of raw .yuv sources")
    a = ap.parse_args(argv)

    if a.cmd == "info":
        from .container import info
        with open(a.src, "rb") as f:
            print(json.dumps(info(f.read()), sort_keys=True))
        return 0
    if a.cmd == "compare":
        return _compare(a)
    if a.cmd == "encode":
        from .transcode import encode_file
        from .video_io import open_video
        model = _model(a.level, a.checkpoint)
        with open_video(a.src, a.size) as reader, open(a.dst, "wb") as f:
            stats = encode_file(model, reader, f, gop=a.gop, batch=a.batch,
                                pixfmt={"matrix": a.matrix, "range": a.range}, digest=a.digest,
                                self_check=a.self_check, msssim=a.msssim)
        print(json.dumps(stats, sort_keys=True))
        return 0
    from .container import ContainerReader, display_size
    from .transcode import decode_file
    from .video_io import Y4MWriter
    with open(a.src, "rb") as f:
        data = f.read()
    reader = ContainerReader(data)
    header = reader.header
    if a.cmd == "verify":
        from .digest import DigestMismatch
        order = [(e[1], e[2], e[3]) for vg in reader.gops() for e in reader.gop_records(*vg)]
        if header.get("frame_digest") is None:
            print(json.dumps({"frames": len(order), "verified": 0, "first_mismatch": None}, sort_keys=True))
            return 2
        model = _model(header["level"], a.checkpoint)
        try:
            stats = decode_file(model, data, None)
            res = {"frames": stats["frames"], "verified": stats["verified"], "first_mismatch": None}
        except DigestMismatch as m:
            print(m, file=sys.stderr)
            at = order.index((m.view, m.gop, m.frame))  # frames decoded and verified before it
            res = {"frames": at, "verified": at, "first_mismatch": [m.view, m.gop, m.frame]}
        print(json.dumps(res, sort_keys=True))
        return 0 if res["first_mismatch"] is None else 1
    h, w = display_size(header)
    model = _model(header["level"], a.checkpoint)
    with Y4MWriter(a.dst, w, h, fps=header.get("fps", (25, 1))) as writer:
        stats = decode_file(model, data, writer, verify=not a.no_verify)
    print(json.dumps(stats, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
