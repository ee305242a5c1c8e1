"""Per-frame reconstruction digest (csrc/fvc_digest.hip): what an encoder stamps on every coded
frame and a decoder checks, so that the two cannot hold different reference frames unnoticed.

A frame is its n float32 bit patterns w[0..n-1] (the NCHW reconstruction [3, Hp, Wp] at the coded
size, n < 2^32):

  D = sum_i mix( (i << 32 | w[i]) + 0x9e3779b97f4a7c15 )  mod 2^64,   mix = the splitmix64 finaliser

Position-dependent, and a sum of integers: exact, and independent of the order of addition.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import kernels as K

NAME = "splitmix64-f32"  # the container header's "frame_digest" value
MASK = (1 << 64) - 1


class DigestMismatch(ValueError):
    """A decoded frame's digest differs from the one its record carries."""

    def __init__(self, view, gop, frame, expected, got):
        self.view, self.gop, self.frame = int(view), int(gop), int(frame)
        self.expected, self.got = int(expected) & MASK, int(got) & MASK
        super().__init__(f"frame digest mismatch at view {self.view} gop {self.gop} frame {self.frame}: the file says "
                         f"{self.expected:#018x}, the decoded frame has {self.got:#018x} (the decoder does not "
                         "reproduce the encoder's reconstruction)")


def frame_digest(x: torch.Tensor) -> torch.Tensor:
    """x float32 [B, ...] (device, contiguous) -> int64 [B] on the device: each frame's digest as
    the uint64 bit pattern. Stream-ordered, no host wait."""
    K._chk(x, name="x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: expected a non-empty [B, ...], got {tuple(x.shape)}")
    B = x.shape[0]
    n = x.numel() // B
    if n >= 1 << 32:
        raise ValueError(f"x: a frame of {n} words does not fit the digest's 32-bit index")
    out = torch.empty(B, dtype=torch.int64, device=x.device)
    _lib.call("fvc_frame_digest_f32", x.data_ptr(), B, n, out.data_ptr(), K.stream_handle(x.device))
    return out


def to_uint64(v) -> int:
    """The digest as a Python int in [0, 2^64) from an int64 element of frame_digest's result."""
    return int(v) & MASK


def frame_digest_host(a: np.ndarray) -> int:
    """The digest of one frame on the host (vectorised numpy, no GPU): a is float32, or uint32
    holding the bit patterns; any shape, read in C order."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        a = a.view(np.uint32)
    elif a.dtype != np.uint32:
        raise ValueError(f"expected float32 or uint32, got {a.dtype}")
    w = a.reshape(-1)
    if not 0 < w.size < 1 << 32:
        raise ValueError(f"a frame holds 1 .. 2^32 - 1 words, got {w.size}")
    z = (np.arange(w.size, dtype=np.uint64) << np.uint64(32)) | w.astype(np.uint64)
    z += np.uint64(0x9e3779b97f4a7c15)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xbf58476d1ce4e5b9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94d049bb133111eb)
    z ^= z >> np.uint64(31)
    return int(np.add.reduce(z, dtype=np.uint64))
