"""GPU: the fused SSIM / MS-SSIM kernel (csrc/fvc_msssim.hip) through metrics.py, models.MSSSIM,
encode_file(msssim=True) and the compare command.

Tolerance (set before any GPU run, from the reference alone): a value passes within twice the
reference's own |float32 - float64| recorded for that quantity in tests/golden/msssim_ref.json,
with a floor of 4 float32 ulps of 1.0 where the reference happened to round exactly."""
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _msssim_cases as MC
from fastvideocodec_amd import metrics as MT
from fastvideocodec_amd import video_io as VIO
from fastvideocodec_amd.synthetic import gop_seed, make_gop
from test_gpu_pixfmt import ref_egress

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(REPO, "tests", "golden", "msssim_ref.json")))
FLOOR = 4 * 2.0 ** -23
H, W, GOP = 184, 200, 2  # display size of the file tests; coded 192 x 256


def on(dev, case):
    x, y, dr = MC.make_case(case)
    return torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), dr


def case_named(name):
    return next(c for c in MC.CASES if c[0] == name)


def within(got, want, env, what):
    got, want, env = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(env, np.float64)
    err, tol = np.abs(got - want), np.maximum(2 * env, FLOOR)
    print(f"{what}: max err {err.max():.3e}, least tolerance {tol.min():.3e}")
    assert not np.isnan(got).any() and (err <= tol).all(), (what, err.max(), tol[err > tol])


@pytest.mark.gpu
@pytest.mark.parametrize("case", MC.CASES, ids=[c[0] for c in MC.CASES])
def test_against_the_reference_fixture(dev, case):
    g = GOLD["cases"][case[0]]
    x, y, dr = on(dev, case)
    x0, y0 = x.clone(), y.clone()
    s = MT.ms_ssim_scales(x, y, dr, case[1])
    assert s.dtype == torch.float64 and s.device == x.device and tuple(s.shape) == (case[1], case[2], 2)
    within(s.cpu().numpy(), g["scales"], g["env_scales"], case[0] + " scales")
    q = MT.ms_ssim(x, y, dr) if case[1] == 5 else MT.ssim(x, y, dr)
    within(q.cpu().numpy(), g["quality"], g["env_quality"], case[0] + " quality")
    assert torch.equal(x, x0) and torch.equal(y, y0)  # read only


@pytest.mark.gpu
def test_exact_properties(dev):
    x8, y8, _ = on(dev, case_named("ms_177x203_b2c3_u8"))
    xf, yf = x8.float(), y8.float()
    assert MT.ms_ssim(xf, xf, 255.0).tolist() == [1.0, 1.0]
    assert MT.ms_ssim(x8, x8, 255.0).tolist() == [1.0, 1.0]
    a = MT.ms_ssim_scales(x8, y8, 255.0)
    assert torch.equal(a, MT.ms_ssim_scales(xf, yf, 255.0))      # uint8 and the same values as float32
    assert torch.equal(a, MT.ms_ssim_scales(x8, y8, 255.0))      # call to call
    assert torch.equal(a[:, 1:], MT.ms_ssim_scales(x8[1:].contiguous(), y8[1:].contiguous(), 255.0))  # alone
    s1 = MT.ssim(xf, yf, 255.0)
    assert torch.equal(s1, a[0, :, 1])                           # levels == 1 is scale 0 of five


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,fill", [(torch.float32, float("nan")), (torch.uint8, 255)])
def test_no_read_outside_the_planes(dev, dtype, fill):
    """The planes are a batch slice from the middle of a larger buffer whose other entries would
    poison (NaN) or change (255) any sum they leaked into."""
    x8, y8, _ = on(dev, case_named("ms_177x203_b1c1_u8"))
    x, y = x8.to(dtype), y8.to(dtype)
    bx = torch.full((3, 1, 177, 203), fill, dtype=dtype, device=dev)
    by = torch.full((3, 1, 177, 203), fill, dtype=dtype, device=dev)
    bx[1], by[1] = x[0], y[0]
    got = MT.ms_ssim_scales(bx[1:2], by[1:2], 255.0)
    assert torch.equal(got, MT.ms_ssim_scales(x, y, 255.0))
    # one window exactly: an 11 x 11 plane between two poisoned ones
    sx = torch.full((3, 1, 11, 11), fill, dtype=dtype, device=dev)
    sy = sx.clone()
    sx[1], sy[1] = x[0, :, :11, :11], y[0, :, :11, :11]
    assert torch.equal(MT.ssim(sx[1:2], sy[1:2], 255.0),
                       MT.ssim(x[:, :, :11, :11].contiguous(), y[:, :, :11, :11].contiguous(), 255.0))


@pytest.mark.gpu
def test_negative_terms_are_clamped(dev):
    x, _, _ = on(dev, case_named("ms_176x176_b2c3_f32"))
    q = MT.ms_ssim(x, (1 - x).contiguous(), 1.0)
    assert bool(torch.isfinite(q).all()) and bool((q >= 0).all()) and bool((q < 1).all())


@pytest.mark.gpu
def test_models_msssim(dev):
    """models.MSSSIM calls the metric at data range 255: frames that hold the byte values as
    float32 then reproduce the fixture's q of the uint8 case."""
    from fastvideocodec_amd.models import MSSSIM
    case = case_named("ms_192x320_b2c3_u8")
    g = GOLD["cases"][case[0]]
    x8, y8, _ = on(dev, case)
    x, y = x8.float(), y8.float()
    q = MT.ms_ssim(x, y, 255.0)
    within(q.cpu().numpy(), g["quality"], g["env_quality"], "MSSSIM q")
    got = MSSSIM(x, y)
    assert got.dim() == 0 and float(got) == float(-10 * torch.log(1 - q.mean()) / math.log(10.0))
    lst = MSSSIM(x, y, use_list=True)
    assert [float(v) for v in lst] == [float(-10 * torch.log(1 - v) / math.log(10.0)) for v in q]


def synthetic_y4m(nframes, seed):
    rgb = make_gop(192, 256, nframes, seed)[:, :, :H, :W]
    y, u, v = ref_egress(rgb, H, W, "bt709", "limited")
    frames = [(y[t], u[t], v[t]) for t in range(nframes)]
    buf = io.BytesIO()
    wr = VIO.Y4MWriter(buf, W, H)
    for f in frames:
        wr.write(*f)
    return buf.getvalue(), frames


@pytest.fixture(scope="module")
def model(dev):
    from fastvideocodec_amd.models import get_codec_model
    return get_codec_model("DVC-pretrained", compression_level=2, device=dev)


@pytest.fixture(scope="module")
def coded(model):
    """Two GOPs of two frames at 200 x 184, coded once with and once without the flag."""
    from fastvideocodec_amd.transcode import decode_file, encode_file
    src, frames = synthetic_y4m(4, gop_seed(7))
    plain, flagged, recon, dec = io.BytesIO(), io.BytesIO(), io.BytesIO(), io.BytesIO()
    st0 = encode_file(model, VIO.Y4MReader(io.BytesIO(src)), plain, gop=GOP)
    st1 = encode_file(model, VIO.Y4MReader(io.BytesIO(src)), flagged, gop=GOP, msssim=True,
                      recon_writer=VIO.Y4MWriter(recon, W, H))
    decode_file(model, flagged.getvalue(), VIO.Y4MWriter(dec, W, H))
    return dict(src=src, frames=frames, plain=plain.getvalue(), flagged=flagged.getvalue(), st0=st0, st1=st1,
                recon=recon.getvalue(), decoded=dec.getvalue())


@pytest.mark.gpu
def test_encode_file_msssim(coded, dev):
    st0, st1 = coded["st0"], coded["st1"]
    assert coded["plain"] == coded["flagged"]                      # the file does not depend on the flag
    assert "msssim_y" not in st0 and {k: v for k, v in st1.items() if k != "msssim_y"} == st0
    assert (st1["coded_height"], st1["coded_width"], st1["frames"], st1["gops"]) == (192, 256, 4, 2)
    rec = list(VIO.Y4MReader(io.BytesIO(coded["recon"])))
    assert len(st1["msssim_y"]) == len(rec) == 4
    for t, (r, s) in enumerate(zip(rec, coded["frames"])):
        a = torch.from_numpy(np.ascontiguousarray(s[0])).to(dev)[None, None]
        b = torch.from_numpy(np.ascontiguousarray(r[0])).to(dev)[None, None]
        assert st1["msssim_y"][t] == float(MT.ms_ssim(a, b, 255.0)), t
        assert 0.0 < st1["msssim_y"][t] <= 1.0
    json.dumps(st1)


@pytest.mark.gpu
def test_encode_file_msssim_refuses_a_small_display_size(model):
    from fastvideocodec_amd.transcode import encode_file

    class Small:
        width, height, fps = 200, 175, (25, 1)

        def __iter__(self):
            raise AssertionError("no frame may be read")

    with pytest.raises(ValueError, match="smaller side is 175, the minimum is 176"):
        encode_file(model, Small(), io.BytesIO(), msssim=True)


@pytest.mark.gpu
def test_compare_reproduces_what_encode_printed(coded, tmp_path):
    """A fresh child process under its own time limit."""
    a, b = tmp_path / "src.y4m", tmp_path / "dec.y4m"
    a.write_bytes(coded["src"])
    b.write_bytes(coded["decoded"])
    r = subprocess.run([sys.executable, "-m", "fastvideocodec_amd", "compare", str(a), str(b)], capture_output=True,
                       text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("psnr_y", "psnr_u", "psnr_v", "msssim_y"):
        assert got[key] == coded["st1"][key], key
    assert (got["frames"], got["height"], got["width"]) == (4, H, W)
