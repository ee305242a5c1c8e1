"""Command line: python -m fastvideocodec_amd encode | decode | info.

  encode IN.y4m|IN.yuv OUT.fvc [--size WxH] [--gop N] [--level L] [--checkpoint PATH]
         [--matrix bt601|bt709] [--range limited|full] [--batch G]     prints one JSON line of stats
  decode IN.fvc OUT.y4m                                                prints one JSON line
  info   IN.fvc                                                        header and record counts (no GPU)
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
    d = sub.add_parser("decode", help="FVC1 container -> Y4M")
    d.add_argument("src")
    d.add_argument("dst")
    d.add_argument("--checkpoint", default=None)
    i = sub.add_parser("info", help="print a container's header and record counts")
    i.add_argument("src")
    a = ap.parse_args(argv)

    if a.cmd == "info":
        from .container import info
        with open(a.src, "rb") as f:
            print(json.dumps(info(f.read()), sort_keys=True))
        return 0
    if a.cmd == "encode":
        from .transcode import encode_file
        from .video_io import open_video
        model = _model(a.level, a.checkpoint)
        with open_video(a.src, a.size) as reader, open(a.dst, "wb") as f:
            stats = encode_file(model, reader, f, gop=a.gop, batch=a.batch,
                                pixfmt={"matrix": a.matrix, "range": a.range})
        print(json.dumps(stats, sort_keys=True))
        return 0
    from .container import ContainerReader, display_size
    from .transcode import decode_file
    from .video_io import Y4MWriter
    with open(a.src, "rb") as f:
        data = f.read()
    header = ContainerReader(data).header
    h, w = display_size(header)
    model = _model(header["level"], a.checkpoint)
    with Y4MWriter(a.dst, w, h, fps=header.get("fps", (25, 1))) as writer:
        stats = decode_file(model, data, writer)
    print(json.dumps(stats, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
