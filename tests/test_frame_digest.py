"""CPU: the frame digest's definition (pinned vectors), its host implementation, the C entry point's
argument validation (no device touched) and the digest's place in the container."""
import io
import os
import struct

import numpy as np
import pytest

from fastvideocodec_amd import _lib
from fastvideocodec_amd import container as CT
from fastvideocodec_amd import digest as DG

M64 = (1 << 64) - 1
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pframe_segment_256x1024.fvc")


def scalar_digest(words):
    """The definition, one word at a time in Python integers."""
    d = 0
    for i, w in enumerate(words):
        z = ((i << 32 | int(w)) + 0x9e3779b97f4a7c15) & M64
        z ^= z >> 30
        z = z * 0xbf58476d1ce4e5b9 & M64
        z ^= z >> 27
        z = z * 0x94d049bb133111eb & M64
        z ^= z >> 31
        d = (d + z) & M64
    return d


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pinned():
    ramp = (np.arange(8) / 8).astype(np.float32)
    swapped = ramp.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    return [(np.zeros(1, np.uint32), 0xe220a8397b1dcdaf),
            (bits(ramp), 0x933fcf021ccce414),
            (bits(swapped), 0x7bb61f9c33785910),
            (bits(np.random.default_rng(0).random(3 * 128 * 192, dtype=np.float32)), 0x2d460e97f6934bed)]


def test_scalar_definition_reproduces_the_pinned_vectors():
    for w, want in pinned():
        assert scalar_digest(w.tolist()) == want


def test_host_digest_equals_the_scalar_definition():
    for w, want in pinned():
        assert DG.frame_digest_host(w) == want
        assert DG.frame_digest_host(w.view(np.float32)) == want  # float32 in, same words
    w = np.random.default_rng(1).integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)
    assert DG.frame_digest_host(w) == scalar_digest(w.tolist())
    assert DG.frame_digest_host(w.reshape(10, 100)) == scalar_digest(w.tolist())  # C order
    with pytest.raises(ValueError):
        DG.frame_digest_host(np.zeros(4, np.float64))
    with pytest.raises(ValueError):
        DG.frame_digest_host(np.zeros(0, np.float32))


def test_digest_mismatch_carries_where_and_what():
    e = DG.DigestMismatch(0, 3, 7, 5, -1)
    assert isinstance(e, ValueError)
    assert (e.view, e.gop, e.frame, e.expected, e.got) == (0, 3, 7, 5, M64)  # int64 bit pattern -> uint64


_BUF = np.zeros(16, dtype=np.float32)
_P = _BUF.ctypes.data


@pytest.mark.parametrize("args", [(None, 1, 16, _P), (_P, 1, 16, None), (_P, 0, 16, _P), (_P, 1, 0, _P),
                                  (_P, 1, 2 ** 32, _P)],
                         ids=["null-x", "null-out", "batch=0", "n=0", "n=2**32"])
def test_entry_point_rejects_bad_arguments(args):
    """FVC_EINVAL from the argument validation, before the memset and the launch: the dummy host
    pointers are never used and no device is touched."""
    assert _lib.load().fvc_frame_digest_f32(*args, None) == -1000


def test_writer_appends_digests_and_record_digest_reads_them():
    header = {"codec": "DVC-pretrained", "gop": 3, "frame_digest": "splitmix64-f32"}
    recs = [(b"I", 0, 0, 0, b"intra-payload", 0x0123456789abcdef), (b"P", 0, 0, 1, b"p1", 0),
            (b"P", 0, 0, 2, b"p2-longer", M64)]
    buf = io.BytesIO()
    w = CT.ContainerWriter(buf, header)
    for kind, v, g, t, payload, d in recs[:2]:
        w.write_payload(kind, v, g, t, payload, digest=d)
    w.write_pframe(*recs[2][1:5], digest=recs[2][5])
    with pytest.raises(ValueError):  # a file's records all carry a digest, or none does
        w.write_payload(b"P", 0, 0, 3, b"p3")
    w.close()
    r = CT.ContainerReader(buf.getvalue())
    assert r.header["frame_digest"] == "splitmix64-f32"
    for e, (kind, v, g, t, payload, d) in zip(r.gop_records(0, 0), recs):
        got = r.record(e)
        assert got[:-8] == payload and got[-8:] == struct.pack("<Q", d)
        assert CT.record_digest(r.header, got) == d
    with pytest.raises(ValueError):
        CT.record_digest({"frame_digest": "crc32"}, b"x" * 16)  # a scheme this reader does not know


def test_a_file_without_the_key_reads_as_before():
    header = {"codec": "DVC-pretrained", "gop": 3}
    payload = b"some payload whose last 8 bytes are not a digest"
    buf = io.BytesIO()
    w = CT.ContainerWriter(buf, header)
    w.write_payload(b"P", 0, 0, 1, payload)
    w.write_pframe(0, 0, 2, payload)
    with pytest.raises(ValueError):
        w.write_payload(b"P", 0, 0, 3, payload, digest=1)
    w.close()
    data = buf.getvalue()
    r = CT.ContainerReader(data)
    for e in r.gop_records(0, 0):
        assert r.record(e) == payload and CT.record_digest(r.header, r.record(e)) is None
    # byte for byte what the format's layout says, which is what the writer produced before digests
    hb = b'{"codec": "DVC-pretrained", "gop": 3}'
    body = b"".join(struct.pack("<cHIHI", b"P", 0, 0, t, len(payload)) + payload for t in (1, 2))
    off = 10 + len(hb)
    index = struct.pack("<I", 2) + b"".join(struct.pack("<cHIHQ", b"P", 0, 0, t, off + k * (13 + len(payload)))
                                            for k, t in enumerate((1, 2)))
    assert data == b"FVC1" + struct.pack("<HI", 1, len(hb)) + hb + body + index + \
        struct.pack("<Q", off + len(body)) + b"FVCX"


def test_the_golden_container_reports_no_digests():
    r = CT.ContainerReader(open(GOLDEN, "rb").read())
    assert "frame_digest" not in r.header
    assert all(CT.record_digest(r.header, r.record(e)) is None for e in r.index)
