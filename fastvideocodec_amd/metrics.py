"""SSIM and MS-SSIM of image batches on the GPU (csrc/fvc_msssim.hip), as the reference's vendored
`DVC/subnet/ms_ssim_torch.py` defines them: the 11-tap Gaussian window (sigma 1.5, float32 taps)
applied separably and valid, (cs, ssim) averaged per image over C, H, W at each of five scales,
the next scale a 2x2 average with a zero row / column in front of an odd side.

Combination (`combine="reference"`, the default) is what that file computes:

  q = prod_{l<5} cs_l^w_l * ssim_5^(4 w_5),   w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) in float32

Its line `prod(mcs[:-1] ** w[:-1] * ssim ** w[-1], dim=0)` broadcasts ssim_5^w_5 into each of the
four cs factors, so the last scale enters with exponent 4 w_5; the published definition (and the
current pip `pytorch_msssim`) has exponent w_5, which `combine="standard"` gives. The pinned oracle
of this module is the vendored file; parity with the pip package is unpinned (it is not installed
where the fixtures are generated).

One decided deviation: every cs and the last ssim are clamped at 0 before the power, as the current
`pytorch_msssim` does; the vendored file returns NaN for a negative base. The two agree whenever
every term is positive.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib
from . import kernels as K

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WIN = 11
# exp(-(k-5)^2 / (2 * 1.5^2)) / sum, formed in float32 by torch as the reference forms them; the
# library holds the same constants (fvc_ms_ssim_window)
TAPS = tuple(float.fromhex(v) for v in (
    "0x1.0d957p-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.10656p-2",
    "0x1.b43c3ep-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d957p-10"))
_DTYPES = {torch.float32: 0, torch.uint8: 1}  # FVC_DTYPE_F32, FVC_DTYPE_U8


def min_side(levels: int) -> int:
    """The smallest height / width that `levels` scales accept: the last scale holds one window
    after floor halving (176 for five scales)."""
    return WIN << (levels - 1)


def _check(x, y, levels):
    if not (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor)):
        raise ValueError("x and y must be tensors")
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"expected two [B,C,H,W] tensors of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.dtype != y.dtype or x.dtype not in _DTYPES:
        raise ValueError(f"x and y must both be float32 or both uint8, got {x.dtype} and {y.dtype}")
    if x.device != y.device:
        raise ValueError(f"x and y must be on one device, got {x.device} and {y.device}")
    if not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError("x and y must be contiguous")
    if not 1 <= levels <= 5:
        raise ValueError(f"levels must be in 1..5, got {levels}")
    B, C, H, W = x.shape
    if B < 1 or C < 1:
        raise ValueError(f"empty batch {tuple(x.shape)}")
    if min(H, W) < min_side(levels):
        raise ValueError(f"frames of {H}x{W} are too small for {levels} scales: the smaller side is {min(H, W)}, "
                         f"the minimum is {min_side(levels)}")


def _weights(weights):
    w = torch.tensor(WEIGHTS if weights is None else [float(v) for v in weights], dtype=torch.float32)
    if w.dim() != 1 or not 1 <= w.numel() <= 5:
        raise ValueError("weights: expected 1 to 5 values")
    return w.double()  # the reference holds them in float32 and widens with the data


def ms_ssim_scales_reference(x, y, data_range=1.0, levels=5):
    """ms_ssim_scales in float64 torch ops for CPU tensors (a restatement of the reference)."""
    _check(x, y, levels)
    X, Y = x.double(), y.double()
    C = X.shape[1]
    win = torch.tensor(TAPS, dtype=torch.float64).reshape(1, 1, 1, WIN).repeat(C, 1, 1, 1)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2

    def blur(t):
        return F.conv2d(F.conv2d(t, win, groups=C), win.transpose(2, 3), groups=C)

    out = []
    for _ in range(levels):
        mu1, mu2 = blur(X), blur(Y)
        m11, m22, m12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s1, s2, s12 = blur(X * X) - m11, blur(Y * Y) - m22, blur(X * Y) - m12
        cs = (2 * s12 + c2) / (s1 + s2 + c2)
        ss = ((2 * m12 + c1) / (m11 + m22 + c1)) * cs
        out.append(torch.stack([cs.mean(-1).mean(-1).mean(-1), ss.mean(-1).mean(-1).mean(-1)], dim=-1))
        pad = (X.shape[2] % 2, X.shape[3] % 2)
        X, Y = F.avg_pool2d(X, kernel_size=2, padding=pad), F.avg_pool2d(Y, kernel_size=2, padding=pad)
    return torch.stack(out)


def ms_ssim_scales(x, y, data_range=1.0, levels=5):
    """x, y [B,C,H,W], float32 or uint8, contiguous -> float64 [levels,B,2]: each image's (cs, ssim)
    means over C, H, W at each scale. Device tensors run the HIP kernel (stream-ordered, no host
    wait); CPU tensors the float64 restatement."""
    _check(x, y, levels)
    if not x.is_cuda:
        return ms_ssim_scales_reference(x, y, data_range, levels)
    B, C, H, W = x.shape
    planes = B * C
    nbytes = _lib.load().fvc_ms_ssim_workspace_bytes(planes, H, W, levels)
    if nbytes == 0:
        raise ValueError(f"unsupported geometry: {planes} planes of {H}x{W} at {levels} scales")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty((levels, B, C, 2), dtype=torch.float64, device=x.device)
    _lib.call("fvc_ms_ssim_planes", x.data_ptr(), y.data_ptr(), _DTYPES[x.dtype], planes, H, W, levels,
              float(data_range), ws.data_ptr(), nbytes, out.data_ptr(), K.stream_handle(x.device))
    return out.mean(dim=2)


def combine_scales(scales, weights=None, combine="reference"):
    """float64 [levels,B,2] -> [B]: prod cs_l^w_l over all but the last scale times ssim_last^(k w_last),
    every base clamped at 0; k = levels - 1 for "reference" (the vendored file's broadcast), 1 for
    "standard"."""
    if combine not in ("reference", "standard"):
        raise ValueError(f"combine must be 'reference' or 'standard', got {combine!r}")
    w = _weights(weights).to(scales.device)
    L = scales.shape[0]
    if w.numel() != L:
        raise ValueError(f"{L} scales need {L} weights, got {w.numel()}")
    cs = scales[:-1, :, 0].clamp_min(0)
    last = scales[-1, :, 1].clamp_min(0)
    k = (L - 1) if combine == "reference" and L > 1 else 1
    return torch.prod(cs ** w[:-1, None], dim=0) * last ** (k * w[-1])


def ssim(x, y, data_range=1.0):
    """Mean SSIM of each image: float64 [B] on the inputs' device."""
    return ms_ssim_scales(x, y, data_range, 1)[0, :, 1]


def ms_ssim(x, y, data_range=1.0, weights=None, combine="reference"):
    """MS-SSIM of each image (module docstring): float64 [B] on the inputs' device. weights: one per
    scale (default: the five of the reference)."""
    L = 5 if weights is None else len(weights)
    return combine_scales(ms_ssim_scales(x, y, data_range, L), weights, combine)


def ms_ssim_reference(x, y, data_range, weights=None, combine="reference"):
    """ms_ssim in float64 torch ops for CPU tensors."""
    L = 5 if weights is None else len(weights)
    return combine_scales(ms_ssim_scales_reference(x, y, data_range, L), weights, combine)
