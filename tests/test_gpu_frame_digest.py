"""GPU: the frame digest kernel against its host definition, and the digest through the file path
(transcode.encode_file / decode_file), the tensor path (container.encode_video / decode_video) and
the command line, on the small case of test_gpu_transcode.py: a 66x130 Y4M of 5 frames, gop=3,
coded size 128x192. Mismatches are made by two benign means only: editing the stored digest, and
decoding a valid P record against another GOP's I-frame."""
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fastvideocodec_amd import container as CT
from fastvideocodec_amd import digest as DG
from fastvideocodec_amd import iframe as IF
from fastvideocodec_amd import video_io as VIO
from fastvideocodec_amd.synthetic import gop_seed, make_gop
from test_gpu_transcode import GOP, H, W, synthetic_y4m

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPS = (30000, 1001)
NAN_BITS = 0x7fc01234


def frame_words(n, seed):
    """Seeded float32 in [-1, 1) with -0.0, +inf and a NaN bit pattern planted where n allows."""
    a = (np.random.default_rng(seed).random(n, dtype=np.float32) * 2 - 1).astype(np.float32)
    if n >= 3:
        a[0], a[n // 2] = -0.0, np.inf
        a.view(np.uint32)[n - 1] = NAN_BITS
    return a


def device_digests(a, dev):
    """frame_digest of a host array [B, n] -> list of uint64."""
    return [DG.to_uint64(v) for v in DG.frame_digest(torch.from_numpy(a).to(dev)).tolist()]


# ---------------------------------------------------------------------------------------- kernel
@pytest.mark.gpu
def test_single_words(dev):
    for k, bits in enumerate((0, 0x80000000, 0x7f800000, NAN_BITS, 0x3f000001)):
        a = np.array([[bits]], np.uint32).view(np.float32)
        assert device_digests(a, dev) == [DG.frame_digest_host(a[0])], hex(bits)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 4 * 256 + 3], ids=["tail-only", "body-and-tail"])
def test_kernel_equals_host(dev, n):
    a = frame_words(n, n)
    assert device_digests(a[None], dev) == [DG.frame_digest_host(a)]


@pytest.mark.gpu
def test_base_misaligned_by_one_word(dev):
    a = frame_words(1028, 7)
    buf = torch.from_numpy(a).to(dev)
    assert buf.data_ptr() % 16 == 0
    x = buf[1:][None]  # [1, 1027] starting 4 bytes past a 16-byte boundary: a 3-word head
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    assert DG.to_uint64(DG.frame_digest(x).item()) == DG.frame_digest_host(a[1:])


@pytest.mark.gpu
def test_batch_frames_are_digested_on_their_own(dev):
    n = 3 * 64 * 64
    a = np.stack([frame_words(n, s) for s in (1, 2, 3)])
    x = torch.from_numpy(a).to(dev).view(3, 3, 64, 64)
    got = device_digests(a, dev)
    assert got == [DG.frame_digest_host(f) for f in a]
    assert [DG.to_uint64(DG.frame_digest(x[b:b + 1]).item()) for b in range(3)] == got  # single-frame calls
    order = [2, 0, 1]
    assert [DG.to_uint64(v) for v in DG.frame_digest(x[order].contiguous()).tolist()] == [got[b] for b in order]
    assert len(set(got)) == 3
    # frames of n % 4 != 0 words start at different alignments inside one batch
    b = np.stack([frame_words(1027, s) for s in (4, 5, 6)])
    assert device_digests(b, dev) == [DG.frame_digest_host(f) for f in b]


@pytest.mark.gpu
def test_grid_stride_loop_and_scalar_tail(dev):
    """The grid is capped at kMaxBlocks blocks of kBlk lanes over a call's frames, so for one frame
    that is the cap (both read from the source here), one 16-byte word per lane and pass: this n
    takes every lane through the loop at least twice, some a third time, and leaves three single
    words."""
    src = open(os.path.join(REPO, "fastvideocodec_amd", "csrc", "fvc_digest.hip")).read()
    cap = int(re.search(r"constexpr unsigned kMaxBlocks = (\d+);", src).group(1))
    blk = int(re.search(r"constexpr int kBlk = (\d+);", src).group(1))
    n = 2 * cap * blk * 4 + 4 * 777 + 3
    assert n <= 8 << 20
    a = frame_words(n, 11)
    assert device_digests(a[None], dev) == [DG.frame_digest_host(a)]


@pytest.mark.gpu
def test_sensitivity(dev):
    a = frame_words(1027, 13)
    a[100], a[200], a[300] = 0.25, 0.5, 0.0
    base = device_digests(a[None], dev)[0]
    flipped, swapped, negzero = a.copy(), a.copy(), a.copy()
    flipped.view(np.uint32)[100] ^= 1
    swapped[[100, 200]] = swapped[[200, 100]]
    negzero[300] = -0.0
    assert negzero[300] == a[300]  # equal as floats, different words
    for b in (flipped, swapped, negzero):
        d = device_digests(b[None], dev)[0]
        assert d != base and d == DG.frame_digest_host(b)


# ------------------------------------------------------------------------------------- file path
@pytest.fixture(scope="module")
def model(dev):
    from fastvideocodec_amd.models import get_codec_model
    return get_codec_model("DVC-pretrained", compression_level=2, device=dev)


def encode(model, src, **kw):
    from fastvideocodec_amd.transcode import encode_file
    f = io.BytesIO()
    stats = encode_file(model, VIO.Y4MReader(io.BytesIO(src)), f, gop=GOP, **kw)
    return f.getvalue(), stats


@pytest.fixture(scope="module")
def coded(model):
    """One stamped encode, one plain encode and one decode shared by the tests below."""
    from fastvideocodec_amd.transcode import decode_file
    src, _ = synthetic_y4m(5, gop_seed(3))
    recon = io.BytesIO()
    data, stats = encode(model, src, digest=True, recon_writer=VIO.Y4MWriter(recon, W, H, fps=FPS))
    plain, _ = encode(model, src)
    dec = io.BytesIO()
    dstats = decode_file(model, data, VIO.Y4MWriter(dec, W, H, fps=FPS))
    return dict(src=src, data=data, stats=stats, plain=plain, recon=recon.getvalue(), decoded=dec.getvalue(),
                dstats=dstats)


def invert_stored_digest(data, key=(0, 0, 1)):
    """A copy of the file with the 8 digest bytes of record (view, gop, frame) inverted."""
    r = CT.ContainerReader(data)
    (e,) = [e for e in r.index if tuple(e[1:4]) == key]
    end = e[4] + CT._REC.size + CT._REC.unpack_from(data, e[4])[4]
    out = bytearray(data)
    out[end - 8:end] = bytes(b ^ 0xff for b in out[end - 8:end])
    return bytes(out)


@pytest.mark.gpu
def test_decode_verifies_every_frame(coded):
    assert coded["dstats"] == {"frames": 5, "height": H, "width": W, "verified": 5}
    assert coded["decoded"] == coded["recon"]


@pytest.mark.gpu
def test_stamped_file_is_the_plain_file_plus_digests(coded):
    a, b = CT.ContainerReader(coded["data"]), CT.ContainerReader(coded["plain"])
    assert a.header["frame_digest"] == "splitmix64-f32" and "frame_digest" not in b.header
    assert {k: v for k, v in a.header.items() if k != "frame_digest"} == b.header
    assert [e[:4] for e in a.index] == [e[:4] for e in b.index] and len(a.index) == 5
    for ea, eb in zip(a.index, b.index):
        assert a.record(ea)[:-8] == b.record(eb)
    assert len({CT.record_digest(a.header, a.record(e)) for e in a.index}) == 5


@pytest.mark.gpu
def test_stamped_bytes_do_not_depend_on_batch_or_self_check(model, coded):
    assert encode(model, coded["src"], digest=True, batch=2)[0] == coded["data"]
    assert encode(model, coded["src"], digest=True, self_check=True)[0] == coded["data"]
    assert encode(model, coded["src"], digest=True, self_check=True, batch=2)[0] == coded["data"]
    assert encode(model, coded["src"], self_check=True)[0] == coded["plain"]  # works without digest


@pytest.mark.gpu
def test_edited_digest_is_reported_at_its_frame(model, coded):
    from fastvideocodec_amd.transcode import decode_file
    bad = invert_stored_digest(coded["data"])
    dec = io.BytesIO()
    with pytest.raises(DG.DigestMismatch) as ei:
        decode_file(model, bad, VIO.Y4MWriter(dec, W, H, fps=FPS))
    e = ei.value
    assert (e.view, e.gop, e.frame) == (0, 0, 1) and e.expected != e.got
    assert e.expected == e.got ^ ((1 << 64) - 1)  # the decoded frame is the right one: only the stamp was inverted
    assert len(list(VIO.Y4MReader(io.BytesIO(dec.getvalue())))) == 1  # frame (0,0,0) was checked and written
    dec = io.BytesIO()
    st = decode_file(model, bad, VIO.Y4MWriter(dec, W, H, fps=FPS), verify=False)
    assert st == {"frames": 5, "height": H, "width": W, "verified": 0}
    assert dec.getvalue() == coded["decoded"]


@pytest.mark.gpu
def test_drift_against_another_reference_changes_the_digest(model, coded, dev):
    """The P record (0,0,1) decoded against GOP 1's I-frame instead of GOP 0's: a valid stream and a
    wrong reference frame, which is what a desynchronised decoder holds."""
    r = CT.ContainerReader(coded["data"])
    iframes = [IF.decode(CT.iframe_from_payload(r.record(r.gop_records(0, g)[0]), dev)) for g in (0, 1)]
    assert not torch.equal(iframes[0], iframes[1])
    payload = r.record(r.gop_records(0, 0)[1])
    want = CT.record_digest(r.header, payload)
    got = [DG.to_uint64(DG.frame_digest(model.decompress(CT.pframe_from_payload(payload, dev), ref)).item())
           for ref in iframes]
    assert got[0] == want and got[1] != want


@pytest.mark.gpu
def test_tensor_path_stamps_and_verifies(model, dev):
    video = torch.from_numpy(make_gop(64, 64, 3, gop_seed(1)).copy()).to(dev)[None]
    data, recons = CT.encode_video_bytes(model, video, digest=True)
    plain, _ = CT.encode_video_bytes(model, video)
    r = CT.ContainerReader(data)
    assert r.header == dict(CT.ContainerReader(plain).header, frame_digest="splitmix64-f32")
    assert [CT.record_digest(r.header, r.record(e)) for e in r.gop_records(0, 0)] == \
        [DG.frame_digest_host(recons[0, t].cpu().numpy()) for t in range(3)]
    out = CT.decode_video(model, data)
    assert torch.equal(out[(0, 0)], recons[0])
    bad = invert_stored_digest(data, (0, 0, 2))
    with pytest.raises(DG.DigestMismatch) as ei:
        CT.decode_video(model, bad)
    assert (ei.value.view, ei.value.gop, ei.value.frame) == (0, 0, 2)
    assert torch.equal(CT.decode_video(model, bad, verify=False)[(0, 0)], recons[0])


@pytest.mark.gpu
def test_command_line(coded, tmp_path):
    """Each step is a fresh child process under its own time limit; the first unexpected status ends
    the test."""
    src, fvc, bad, plain = (tmp_path / n for n in ("src.y4m", "out.fvc", "bad.fvc", "plain.fvc"))
    src.write_bytes(coded["src"])
    run = lambda *a: subprocess.run([sys.executable, "-m", "fastvideocodec_amd", *a], capture_output=True,  # noqa: E731
                                    text=True, timeout=300, cwd=REPO)
    last = lambda p: json.loads(p.stdout.strip().splitlines()[-1])  # noqa: E731
    enc = run("encode", str(src), str(fvc), "--gop", str(GOP), "--digest", "--self-check")
    assert enc.returncode == 0, enc.stderr[-2000:]
    assert fvc.read_bytes() == coded["data"]
    assert last(enc) == json.loads(json.dumps(coded["stats"]))
    ok = run("verify", str(fvc))
    assert ok.returncode == 0, ok.stderr[-2000:]
    assert last(ok) == {"frames": 5, "verified": 5, "first_mismatch": None}
    bad.write_bytes(invert_stored_digest(coded["data"]))
    mis = run("verify", str(bad))
    assert mis.returncode == 1, mis.stderr[-2000:]
    assert last(mis) == {"frames": 1, "verified": 1, "first_mismatch": [0, 0, 1]}
    plain.write_bytes(coded["plain"])
    none = run("verify", str(plain))
    assert none.returncode == 2, none.stderr[-2000:]
    assert last(none) == {"frames": 5, "verified": 0, "first_mismatch": None}
