"""CPU: the Y4M / raw I420 readers and writer, the container's display-geometry header keys and
`info`, and the colour coefficient tables' row-sum rule."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from fastvideocodec_amd import container as CT
from fastvideocodec_amd import video_io as VIO
from test_gpu_pixfmt import PAIRS, ref_coefficients, ref_egress, ref_ingest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(n, w, h, seed=0):
    rng = np.random.default_rng(seed)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
             rng.integers(0, 256, (ch, cw), dtype=np.uint8)) for _ in range(n)]


def _y4m(frames, w, h, **kw):
    buf = io.BytesIO()
    wr = VIO.Y4MWriter(buf, w, h, **kw)
    for f in frames:
        wr.write(*f)
    return buf.getvalue()


@pytest.mark.parametrize("w,h,fps", [(64, 64, (25, 1)), (51, 37, (30000, 1001)), (3, 2, (24, 1)), (1, 1, (60, 1))])
def test_y4m_round_trip_is_byte_identical(w, h, fps):
    frames = _frames(3, w, h, seed=w + h)
    data = _y4m(frames, w, h, fps=fps, aspect="1:1")
    assert data.startswith(f"YUV4MPEG2 W{w} H{h} F{fps[0]}:{fps[1]} Ip A1:1 C420jpeg\n".encode())
    r = VIO.Y4MReader(io.BytesIO(data))
    assert (r.width, r.height, r.fps, r.chroma, r.aspect) == (w, h, fps, "420jpeg", "1:1")
    got = list(r)
    assert len(got) == 3 and r.frames_read == 3
    for a, b in zip(got, frames):
        for p, q in zip(a, b):
            assert p.dtype == np.uint8 and np.array_equal(p, q)
    assert _y4m(got, r.width, r.height, fps=r.fps, chroma=r.chroma, aspect=r.aspect) == data


def test_y4m_reads_from_a_path_frame_by_frame(tmp_path):
    frames = _frames(2, 10, 6)
    path = tmp_path / "a.y4m"
    with VIO.Y4MWriter(str(path), 10, 6) as wr:
        for f in frames:
            wr.write(*f)
    with VIO.open_video(str(path)) as r:
        first = next(r)
        assert r.f.tell() < path.stat().st_size  # the second frame has not been read yet
        assert np.array_equal(first[0], frames[0][0])
        assert np.array_equal(next(r)[2], frames[1][2])
        with pytest.raises(StopIteration):
            next(r)


@pytest.mark.parametrize("head", [b"YUV4MPEG2 W4 H4 F25:1 Ip C420\n", b"YUV4MPEG2 W4 H4 F25:1\n",
                                  b"YUV4MPEG2 H4 W4 C420mpeg2 XYSCSS=420\n", b"YUV4MPEG2 W4 H4 A1:1 C420paldv\n"])
def test_y4m_accepted_headers(head):
    body = bytes(range(24))
    r = VIO.Y4MReader(io.BytesIO(head + b"FRAME\n" + body))
    y, u, v = next(r)
    assert (r.width, r.height) == (4, 4) and y.tobytes() + u.tobytes() + v.tobytes() == body


@pytest.mark.parametrize("tag", ["C422", "C444", "Cmono", "C420p10", "C444p16", "It", "Ib", "Im"])
def test_y4m_rejected_tags_are_named(tag):
    with pytest.raises(ValueError, match=tag):
        VIO.Y4MReader(io.BytesIO(f"YUV4MPEG2 W4 H4 F25:1 {tag}\n".encode()))
    if tag.startswith("C"):
        with pytest.raises(ValueError, match=tag):
            VIO.Y4MWriter(io.BytesIO(), 4, 4, chroma=tag[1:])


def test_bad_streams_raise():
    with pytest.raises(ValueError):
        VIO.Y4MReader(io.BytesIO(b"RIFF W4 H4\n"))
    with pytest.raises(ValueError):
        VIO.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 F25:1\n"))  # no height
    data = _y4m(_frames(2, 5, 3), 5, 3)
    r = VIO.Y4MReader(io.BytesIO(data[:-1]))
    next(r)
    with pytest.raises(ValueError, match="truncated"):
        next(r)
    r = VIO.Y4MReader(io.BytesIO(data.replace(b"FRAME\n", b"FRANE\n")))
    with pytest.raises(ValueError):
        next(r)
    with pytest.raises(ValueError):
        VIO.Y4MWriter(io.BytesIO(), 5, 3).write(*_frames(1, 4, 3)[0])


def test_raw_i420_reader():
    frames = _frames(3, 7, 5)
    raw = b"".join(p.tobytes() for f in frames for p in f)
    got = list(VIO.RawYUVReader(io.BytesIO(raw), 7, 5))
    assert len(got) == 3 and all(np.array_equal(p, q) for a, b in zip(got, frames) for p, q in zip(a, b))
    r = VIO.RawYUVReader(io.BytesIO(raw[:-3]), 7, 5)
    next(r), next(r)
    with pytest.raises(ValueError, match="truncated"):
        next(r)
    with pytest.raises(ValueError):
        VIO.open_video("clip.yuv")  # a raw file needs its size


def _container(header):
    buf = io.BytesIO()
    w = CT.ContainerWriter(buf, header)
    for g in range(2):
        w.write_payload(b"I", 0, g, 0, b"i" * 5)
        for t in (1, 2):
            w.write_payload(b"P", 0, g, t, b"p" * (3 + t))
    w.close()
    return buf.getvalue()


def test_info_with_and_without_display_geometry(tmp_path):
    old = {"codec": "DVC-pretrained", "level": 2, "height": 128, "width": 192, "gop": 3, "gops": 2}
    new = dict(old, display_height=66, display_width=130, fps=[30000, 1001], frames=6,
               pixfmt={"chroma": "420", "matrix": "bt709", "range": "limited"})
    a, b = CT.info(_container(old)), CT.info(_container(new))
    assert a["display"] == a["coded"] == [128, 192] and b["display"] == [66, 130] and b["coded"] == [128, 192]
    for i in (a, b):
        assert (i["gops"], i["records"], i["iframes"], i["pframes"]) == (2, 6, 2, 4)
    assert a["header"] == old and b["header"] == new
    assert CT.display_size(old) == (128, 192) and CT.display_size(new) == (66, 130)
    with pytest.raises(ValueError):
        CT.display_size(dict(old, display_height=129))
    with pytest.raises(ValueError):
        CT.ContainerWriter(io.BytesIO(), old).write_payload(b"X", 0, 0, 0, b"")
    # the command line prints the same thing, and needs no GPU for it
    path = tmp_path / "a.fvc"
    path.write_bytes(_container(new))
    out = subprocess.run([sys.executable, "-m", "fastvideocodec_amd", "info", str(path)], capture_output=True,
                         text=True, timeout=120, check=True, cwd=REPO)
    assert json.loads(out.stdout) == json.loads(json.dumps(b))


def test_make_header_keys():
    class M:
        name, compression_level = "DVC-pretrained", 2
    import unittest.mock as mock
    with mock.patch.object(CT, "tables_crc", lambda m: "00000000"):
        base = CT.make_header(M, 128, 192, 3, 2, "segment", 4)
        full = CT.make_header(M, 128, 192, 3, 2, "segment", 4, display=(66, 130), fps=(30000, 1001), frames=5,
                              pixfmt={"matrix": "bt601", "range": "full"})
    assert not {"display_height", "display_width", "pixfmt", "fps", "frames"} & set(base)
    assert {k: full[k] for k in base} == base
    assert (full["display_height"], full["display_width"], full["fps"], full["frames"]) == (66, 130, [30000, 1001], 5)
    assert full["pixfmt"] == {"chroma": "420", "matrix": "bt601", "range": "full"}


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_coefficient_tables_obey_the_row_sum_rule(pair):
    """The library's tables equal the rule restated in numpy, and the rule keeps grey exact."""
    from fastvideocodec_amd import pixfmt as PF
    fwd, (yoff, coff), inv = PF.coefficients(*pair)
    Q, ref_yoff = ref_coefficients(*pair)
    assert np.array_equal(fwd.astype(np.int64), Q) and (yoff, coff) == (ref_yoff, 128)
    sy = 219.0 / 255.0 if pair[1] == "limited" else 1.0
    assert fwd.sum(axis=1).tolist() == [int(np.rint(sy * 65536.0)), 0, 0]
    if pair == ("bt709", "limited"):
        assert fwd.tolist() == [[11966, 40254, 4064], [-6596, -22189, 28785], [28784, -26145, -2639]]
    assert inv.dtype == np.float32 and inv.shape == (5,)
    # grey through the restated conversions: every legal Y returns, chroma stays 128
    legal = np.arange(16, 236) if pair[1] == "limited" else np.arange(0, 256)
    y = np.resize(legal, (1, 16, 16)).astype(np.uint8)
    u = np.full((1, 8, 8), 128, np.uint8)
    y2, u2, v2 = ref_egress(ref_ingest(y, u, u, *pair).astype(np.float32), 16, 16, *pair)
    assert np.array_equal(y2, y) and (u2 == 128).all() and (v2 == 128).all()
    with pytest.raises(ValueError):
        PF.coefficients("bt2020", "limited")
