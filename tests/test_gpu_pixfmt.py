"""GPU: the 8-bit YUV 4:2:0 ingest / egress kernels and the exact u8 SSE (csrc/fvc_pixfmt.hip)
against numpy restatements kept here: float64 for ingest, int64 for egress. The restatements are
also what the transcode tests use to make their YUV sources (module import needs no GPU)."""
import math

import numpy as np
import pytest
import torch

from fastvideocodec_amd.synthetic import pad_to_multiple

KRKB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
PAIRS = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
SIZES = [(64, 64), (37, 51), (66, 130), (1, 1), (2, 3)]
FVC_EINVAL = -1000


# ------------------------------------------------------------------ numpy restatements
def ref_coefficients(matrix, rng):
    """RGB8 -> YUV8 rows with 16 fractional bits: rint(M * 65536), then the largest-magnitude entry
    of each row adjusted so the luma row sums to rint(s_y * 65536) and the chroma rows to 0."""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (219.0 / 255.0, 224.0 / 255.0) if rng == "limited" else (1.0, 1.0)
    M = np.array([[sy * kr, sy * kg, sy * kb],
                  [-sc * kr / (2 * (1 - kb)), -sc * kg / (2 * (1 - kb)), sc * 0.5],
                  [sc * 0.5, -sc * kg / (2 * (1 - kr)), -sc * kb / (2 * (1 - kr))]], np.float64)
    Q = np.rint(M * 65536.0).astype(np.int64)
    want = [int(np.rint(sy * 65536.0)), 0, 0]
    for r in range(3):
        Q[r, int(np.argmax(np.abs(M[r])))] += want[r] - int(Q[r].sum())
    return Q, (16 if rng == "limited" else 0)


def _near_far(n_luma, n_chroma):
    """Per luma index: its chroma sample and the clamped neighbour towards it (centre siting)."""
    i = np.arange(n_luma)
    near = i >> 1
    far = np.clip(near + np.where(i & 1, 1, -1), 0, n_chroma - 1)
    return near, far


def ref_upsample16(c, h, w):
    """Chroma plane [B,ch,cw] u8 -> [B,h,w] int64 in 1/16 units (bilinear 9/3/3/1)."""
    c = c.astype(np.int64)
    rn, rf = _near_far(h, c.shape[1])
    cn, cf = _near_far(w, c.shape[2])
    return (9 * c[:, rn][:, :, cn] + 3 * c[:, rn][:, :, cf] + 3 * c[:, rf][:, :, cn] + c[:, rf][:, :, cf])


def ref_ingest(y, u, v, matrix, rng):
    """Planes u8 -> float64 RGB [B,3,h,w] in [0,1] (unpadded)."""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    B, h, w = y.shape
    yoff, ys, cs = (16, 219.0, 224.0) if rng == "limited" else (0, 255.0, 255.0)
    yy = (y.astype(np.float64) - yoff) / ys
    cb = (ref_upsample16(u, h, w) - 2048) / (16.0 * cs)
    cr = (ref_upsample16(v, h, w) - 2048) / (16.0 * cs)
    r = yy + 2 * (1 - kr) * cr
    g = yy - (2 * kb * (1 - kb) / kg) * cb - (2 * kr * (1 - kr) / kg) * cr
    b = yy + 2 * (1 - kb) * cb
    return np.clip(np.stack([r, g, b], 1), 0.0, 1.0)


def ref_egress(x, h, w, matrix, rng):
    """float32 RGB [B,3,Hp,Wp] -> u8 planes of the top-left h x w, integer arithmetic."""
    Q, yoff = ref_coefficients(matrix, rng)
    x = np.asarray(x, np.float32)[:, :, :h, :w]
    c8 = np.rint(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.int64)
    offs = [yoff, 128, 128]
    px = [np.clip((Q[k, 0] * c8[:, 0] + Q[k, 1] * c8[:, 1] + Q[k, 2] * c8[:, 2] + (offs[k] << 16) + 32768) >> 16,
                  0, 255) for k in range(3)]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    r0, r1 = 2 * np.arange(ch), np.minimum(2 * np.arange(ch) + 1, h - 1)
    c0, c1 = 2 * np.arange(cw), np.minimum(2 * np.arange(cw) + 1, w - 1)
    sub = lambda p: (p[:, r0][:, :, c0] + p[:, r0][:, :, c1] + p[:, r1][:, :, c0] + p[:, r1][:, :, c1] + 2) >> 2  # noqa: E731
    return px[0].astype(np.uint8), sub(px[1]).astype(np.uint8), sub(px[2]).astype(np.uint8)


# ------------------------------------------------------------------ inputs
def make_planes(kind, B, h, w, seed=0):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if kind == "random":
        rng = np.random.default_rng(1000 * h + w + seed)
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((B, h, w), (B, ch, cw), (B, ch, cw)))
    val = 0 if kind == "zeros" else 255
    return tuple(np.full(s, val, np.uint8) for s in ((B, h, w), (B, ch, cw), (B, ch, cw)))


def make_rgb(B, Hp, Wp, seed):
    """Floats that hold exact k/255, exact 0 and 1, and values outside [0,1] (pad region too)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.25, 1.25, (B, 3, Hp, Wp)).astype(np.float32)
    k255 = (rng.integers(0, 256, x.shape).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    pick = rng.integers(0, 8, x.shape)
    x = np.where(pick < 3, k255, x)
    x = np.where(pick == 3, np.float32(0.0), x)
    x = np.where(pick == 4, np.float32(1.0), x)
    return np.ascontiguousarray(x, np.float32)


def _dev(planes, dev):
    return tuple(torch.from_numpy(p).to(dev) for p in planes)


def _coded(h, w):
    return -(-h // 64) * 64, -(-w // 64) * 64


# ------------------------------------------------------------------ tests
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "zeros", "full"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ingest_matches_float64_and_pads_by_replication(dev, size, B, pair, kind):
    """Bound 1e-6: the output is in [0,1], the integer chroma interpolation is exact, and the
    float32 matrix step is a handful of 2^-24-relative roundings on magnitudes below 2."""
    from fastvideocodec_amd import pixfmt as PF
    h, w = size
    planes = make_planes(kind, B, h, w)
    x, hw = PF.yuv420_to_rgb(*_dev(planes, dev), matrix=pair[0], range=pair[1])
    assert hw == (h, w) and tuple(x.shape) == (B, 3) + _coded(h, w) and x.dtype == torch.float32
    got = x.cpu()
    ref = ref_ingest(*planes, *pair)
    err = float(np.abs(got[:, :, :h, :w].numpy().astype(np.float64) - ref).max())
    print(f"ingest {size} B={B} {pair} {kind}: max|err| = {err:.3e}")
    assert err <= 1e-6
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    padded = torch.from_numpy(pad_to_multiple(got[:, :, :h, :w].numpy().copy(), 64))
    assert torch.equal(got, padded)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_egress_is_bit_exact(dev, size, B, pair):
    from fastvideocodec_amd import pixfmt as PF
    h, w = size
    Hp, Wp = _coded(h, w)
    x = make_rgb(B, Hp, Wp, seed=h * 131 + w)
    got = PF.rgb_to_yuv420(torch.from_numpy(x).to(dev), h, w, *pair)
    ref = ref_egress(x, h, w, *pair)
    for name, g, r in zip("yuv", got, ref):
        assert g.dtype == torch.uint8 and tuple(g.shape) == r.shape, name
        assert torch.equal(g.cpu(), torch.from_numpy(r)), name


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_grey_survives_ingest_then_egress(dev, pair):
    """U = V = 128 and every legal Y: Y -> RGB -> Y is the identity and chroma stays 128."""
    from fastvideocodec_amd import pixfmt as PF
    h, w = 37, 51
    legal = np.arange(16, 236) if pair[1] == "limited" else np.arange(0, 256)
    y = legal[np.arange(h * w) % len(legal)].astype(np.uint8).reshape(1, h, w)
    u = np.full((1, (h + 1) // 2, (w + 1) // 2), 128, np.uint8)
    x, _ = PF.yuv420_to_rgb(*_dev((y, u, u.copy()), dev), *pair)
    assert torch.equal(x[:, 0], x[:, 1]) and torch.equal(x[:, 0], x[:, 2])
    y2, u2, v2 = PF.rgb_to_yuv420(x, h, w, *pair)
    assert torch.equal(y2.cpu(), torch.from_numpy(y))
    assert int(u2.min()) == int(u2.max()) == int(v2.min()) == int(v2.max()) == 128


@pytest.mark.gpu
@pytest.mark.parametrize("n,offset", [(1, 0), (63, 0), (64, 0), (65, 0), ((1 << 20) + 3, 0), (65, 1), (4099, 3)])
def test_sse_u8_is_exact(dev, n, offset):
    """offset > 0 starts both buffers off a 16-byte boundary (the kernel's byte path)."""
    from fastvideocodec_amd import pixfmt as PF
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, n + offset, dtype=np.uint8)
    b = rng.integers(0, 256, n + offset, dtype=np.uint8)
    ref = int(((a[offset:].astype(np.int64) - b[offset:].astype(np.int64)) ** 2).sum())
    da, db = torch.from_numpy(a).to(dev)[offset:], torch.from_numpy(b).to(dev)[offset:]
    assert PF.sse_u8(da, db) == ref
    assert PF.plane_psnr(da, db) == 10.0 * math.log10(255.0 ** 2 * n / ref)
    assert PF.sse_u8(da, da) == 0 and PF.plane_psnr(da, da) == math.inf


@pytest.mark.gpu
def test_all_extremes_sse(dev):
    from fastvideocodec_amd import pixfmt as PF
    n = 100003
    a = torch.zeros(n, dtype=torch.uint8, device=dev)
    b = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    assert PF.sse_u8(a, b) == n * 255 * 255


@pytest.mark.gpu
def test_bad_arguments_return_einval(dev):
    from fastvideocodec_amd import _lib, pixfmt as PF
    lib = _lib.load()
    h, w = 37, 51
    y, u, v = _dev(make_planes("random", 1, h, w), dev)
    x = torch.zeros((1, 3, 64, 64), dtype=torch.float32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def ingest(geom, y_=y, u_=u, v_=v, x_=x):
        return lib.fvc_yuv420_to_rgb_pad(p(y_), p(u_), p(v_), p(x_), *geom, None)

    def egress(geom, y_=y, u_=u, v_=v, x_=x):
        return lib.fvc_rgb_to_yuv420_crop(p(x_), p(y_), p(u_), p(v_), *geom, None)

    ok = (1, h, w, 64, 64, 1, 0)  # batch, h, w, Hp, Wp, matrix, range
    for call in (ingest, egress):
        assert call((1, 65, w, 64, 64, 1, 0)) == FVC_EINVAL       # Hp < h
        assert call((1, h, 65, 64, 64, 1, 0)) == FVC_EINVAL       # Wp < w
        assert call((1, h, w, 96, 64, 1, 0)) == FVC_EINVAL        # Hp % 64 != 0
        assert call((1, h, w, 64, 100, 1, 0)) == FVC_EINVAL       # Wp % 64 != 0
        assert call((0, h, w, 64, 64, 1, 0)) == FVC_EINVAL        # empty batch
        assert call((1, h, w, 64, 64, 2, 0)) == FVC_EINVAL        # unknown matrix
        assert call((1, h, w, 64, 64, 1, 2)) == FVC_EINVAL        # unknown range
        for null in ("y_", "u_", "v_", "x_"):
            assert call(ok, **{null: None}) == FVC_EINVAL, (call.__name__, null)
        assert call(ok) == 0
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    assert lib.fvc_sse_u8(None, p(y), 4, p(out), None) == FVC_EINVAL
    assert lib.fvc_sse_u8(p(y), p(y), 4, None, None) == FVC_EINVAL
    assert lib.fvc_sse_u8(p(y), p(y), 0, p(out), None) == FVC_EINVAL
    torch.cuda.synchronize()
    # the Python layer refuses what the kernels cannot take
    with pytest.raises(ValueError):
        PF.yuv420_to_rgb(y.cpu(), u, v)
    with pytest.raises(ValueError):
        PF.yuv420_to_rgb(y, u[:, :, :-1].contiguous(), v)
    with pytest.raises(ValueError):
        PF.yuv420_to_rgb(y.float(), u, v)
    with pytest.raises(ValueError):
        PF.yuv420_to_rgb(y, u, v, matrix="bt2020")
    with pytest.raises(ValueError):
        PF.yuv420_to_rgb(y, u, v, multiple=32)
    with pytest.raises(ValueError):
        PF.rgb_to_yuv420(x, 65, 10)
    with pytest.raises(ValueError):
        PF.rgb_to_yuv420(x.transpose(2, 3), 10, 10)
