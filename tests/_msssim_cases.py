"""Seeded inputs of the MS-SSIM tests, shared by tests/golden/gen_msssim_golden.py (which runs the
reference on them) and the tests (which run this package on them). Integer arithmetic on PCG64
draws only, so the bytes are the same on every machine: a smooth field (a bilinearly interpolated
coarse grid) plus texture at two grains, and y = x plus noise of a few grey levels at four grains
(the coarse grains keep cs away from 1 at the pooled scales).

A case is (name, levels, B, C, h, w, kind): kind "u8" is the uint8 pair at data range 255, kind
"f32" the same bytes / 255 as float32 at data range 1."""
import numpy as np

TILE = 32  # the SSIM kernel's output tile; a tile reads TILE + 10 input rows and columns

SINGLE_SIZES = [(11, 11), (11, 75), (12, 45), (TILE + 9, TILE + 9), (TILE + 10, TILE + 10), (TILE + 11, TILE + 11)]
MULTI_SIZES = [(176, 176), (177, 203), (192, 320)]

CASES = []
for _h, _w in SINGLE_SIZES:
    for _k in ("f32", "u8"):
        CASES.append((f"ssim_{_h}x{_w}_{_k}", 1, 1, 2, _h, _w, _k))
for _h, _w in MULTI_SIZES:
    for _k in ("f32", "u8"):
        CASES.append((f"ms_{_h}x{_w}_b2c3_{_k}", 5, 2, 3, _h, _w, _k))
    CASES.append((f"ms_{_h}x{_w}_b1c1_u8", 5, 1, 1, _h, _w, "u8"))

DATA_RANGE = {"f32": 1.0, "u8": 255.0}


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (1 << 63)


def _blocks(rng, lo, hi, h, w, g):
    """Integers in [lo, hi] constant over g x g blocks."""
    a = rng.integers(lo, hi + 1, size=(h // g + 1, w // g + 1))
    return np.repeat(np.repeat(a, g, axis=0), g, axis=1)[:h, :w]


def _plane(rng, h, w):
    g = 32
    a = rng.integers(40, 216, size=(h // g + 2, w // g + 2)).astype(np.int64)
    r, c = np.arange(h), np.arange(w)
    ri, fr = (r // g)[:, None], (r % g)[:, None]
    ci, fc = (c // g)[None, :], (c % g)[None, :]
    smooth = ((g - fr) * (g - fc) * a[ri, ci] + fr * (g - fc) * a[ri + 1, ci] + (g - fr) * fc * a[ri, ci + 1]
              + fr * fc * a[ri + 1, ci + 1]) // (g * g)
    x = smooth + _blocks(rng, -20, 20, h, w, 4) + rng.integers(-12, 13, size=(h, w))
    x = np.clip(x, 0, 255)
    noise = (rng.integers(-4, 5, size=(h, w)) + _blocks(rng, -3, 3, h, w, 4) + _blocks(rng, -3, 3, h, w, 16)
             + _blocks(rng, -3, 3, h, w, 64))
    y = np.clip(x + noise, 0, 255)
    return x.astype(np.uint8), y.astype(np.uint8)


def make_bytes(name, B, C, h, w):
    """uint8 [B,C,h,w] pair of a case; the f32 and u8 kinds of one geometry share the bytes."""
    rng = np.random.Generator(np.random.PCG64(_seed(f"{B}x{C}x{h}x{w}")))
    x = np.empty((B, C, h, w), np.uint8)
    y = np.empty((B, C, h, w), np.uint8)
    for b in range(B):
        for c in range(C):
            x[b, c], y[b, c] = _plane(rng, h, w)
    return x, y


def make_case(case):
    """(x, y, data_range) as numpy arrays of the case's kind."""
    name, _, B, C, h, w, kind = case
    x, y = make_bytes(name, B, C, h, w)
    if kind == "f32":
        x, y = x.astype(np.float32) / np.float32(255), y.astype(np.float32) / np.float32(255)
    return x, y, DATA_RANGE[kind]
