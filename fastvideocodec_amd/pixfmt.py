"""8-bit planar YUV 4:2:0 <-> the codec's float RGB frames, on the GPU (csrc/fvc_pixfmt.hip).

Ingest converts and replicate-pads in one kernel (same placement as synthetic.pad_to_multiple),
egress crops to the display size and converts back with integer arithmetic, and plane_psnr is the
exact 8-bit PSNR from an integer sum of squared differences. Chroma is treated as centre-sited.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from . import kernels as K

MATRICES = ("bt601", "bt709")
RANGES = ("limited", "full")


def _enum(matrix, range):
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {MATRICES}, got {matrix!r}")
    if range not in RANGES:
        raise ValueError(f"range must be one of {RANGES}, got {range!r}")
    return MATRICES.index(matrix), RANGES.index(range)


def coefficients(matrix="bt709", range="limited"):
    """The kernels' tables (host call, no GPU): (fwd [3,3] int32 RGB8 -> YUV8 rows with 16
    fractional bits, offsets (luma, chroma), inv float32 [ky, rv, gu, gv, bu])."""
    m, r = _enum(matrix, range)
    fwd = np.zeros(9, np.int32)
    offs = np.zeros(2, np.int32)
    inv = np.zeros(5, np.float32)
    _lib.call("fvc_pixfmt_coeffs", m, r, fwd.ctypes.data, offs.ctypes.data, inv.ctypes.data)
    return fwd.reshape(3, 3), (int(offs[0]), int(offs[1])), inv


def chroma_size(h, w):
    return (h + 1) // 2, (w + 1) // 2


def _check_planes(y, u, v):
    if y.dim() != 3:
        raise ValueError(f"y: expected [B,h,w], got {tuple(y.shape)}")
    B, h, w = y.shape
    if B < 1 or h < 1 or w < 1:
        raise ValueError(f"y: empty plane {tuple(y.shape)}")
    K._chk(y, dtype=torch.uint8, name="y")
    ch, cw = chroma_size(h, w)
    K._chk(u, (B, ch, cw), torch.uint8, "u")
    K._chk(v, (B, ch, cw), torch.uint8, "v")
    if u.device != y.device or v.device != y.device:
        raise ValueError("y, u, v must be on one device")
    return B, h, w


def yuv420_to_rgb(y, u, v, matrix="bt709", range="limited", multiple=64):
    """Planes y [B,h,w], u / v [B,(h+1)/2,(w+1)/2] (uint8, device) -> (x, (h, w)): x float32
    [B,3,Hp,Wp] in [0,1] with Hp, Wp = h, w rounded up to `multiple` (a multiple of 64) and the
    padding replicated from the last row / column."""
    m, r = _enum(matrix, range)
    if multiple < 64 or multiple % 64:
        raise ValueError(f"multiple must be a positive multiple of 64, got {multiple}")
    B, h, w = _check_planes(y, u, v)
    Hp, Wp = -(-h // multiple) * multiple, -(-w // multiple) * multiple
    x = torch.empty((B, 3, Hp, Wp), dtype=torch.float32, device=y.device)
    _lib.call("fvc_yuv420_to_rgb_pad", y.data_ptr(), u.data_ptr(), v.data_ptr(), x.data_ptr(), B, h, w, Hp, Wp,
              m, r, K.stream_handle(y.device))
    return x, (h, w)


def rgb_to_yuv420(x, h, w, matrix="bt709", range="limited"):
    """x float32 [B,3,Hp,Wp] (device; Hp, Wp multiples of 64) -> uint8 planes (y, u, v) of its
    top-left h x w."""
    m, r = _enum(matrix, range)
    K._chk(x, name="x")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"x: expected [B,3,Hp,Wp], got {tuple(x.shape)}")
    B, _, Hp, Wp = x.shape
    if Hp % 64 or Wp % 64:
        raise ValueError(f"x: Hp and Wp must be multiples of 64, got {Hp}x{Wp}")
    if not (1 <= h <= Hp and 1 <= w <= Wp):
        raise ValueError(f"display size {h}x{w} does not fit the coded size {Hp}x{Wp}")
    ch, cw = chroma_size(h, w)
    y = torch.empty((B, h, w), dtype=torch.uint8, device=x.device)
    u = torch.empty((B, ch, cw), dtype=torch.uint8, device=x.device)
    v = torch.empty((B, ch, cw), dtype=torch.uint8, device=x.device)
    _lib.call("fvc_rgb_to_yuv420_crop", x.data_ptr(), y.data_ptr(), u.data_ptr(), v.data_ptr(), B, h, w, Hp, Wp,
              m, r, K.stream_handle(x.device))
    return y, u, v


def sse_u8(a, b) -> int:
    """Exact sum of squared differences of two uint8 device tensors of equal shape."""
    return int(sse_u8_device(a, b).item())


def sse_u8_device(a, b) -> torch.Tensor:
    """sse_u8 left on the device (int64 [1], stream-ordered): no host wait."""
    K._chk(a, dtype=torch.uint8, name="a")
    K._chk(b, tuple(a.shape), torch.uint8, "b")
    if a.device != b.device:
        raise ValueError("a and b must be on one device")
    if a.numel() == 0:
        raise ValueError("empty planes")
    out = torch.empty(1, dtype=torch.int64, device=a.device)
    _lib.call("fvc_sse_u8", a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), K.stream_handle(a.device))
    return out


def psnr_from_sse(sse: int, n: int) -> float:
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 * n / sse)


def plane_psnr(a, b) -> float:
    """10 log10(255^2 N / SSE) of two uint8 device planes, from the exact SSE; inf when equal."""
    return psnr_from_sse(sse_u8(a, b), a.numel())
