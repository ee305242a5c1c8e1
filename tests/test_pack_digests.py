"""CPU: every weight pack entry point of libfvc (host C++) must keep producing the bytes and
output scales recorded in tests/golden/pack_digests.json. The split-precision pack functions share
one definition of the scale exponent and the hi / lo split (csrc/fvc_split.h), and they and the
f32 pack share one tap geometry (csrc/fvc_taps.h); encoder / decoder bit-exactness rests on them,
and the other pack tests only bound their rounding.

The weights are filled by integer arithmetic (no RNG stream to drift between numpy versions). The
golden file holds the SHA-256 of each pack and its scale(s) as float bits. It is regenerated with
    FVC_LIB_PATH=<libfvc.so of a trusted build> python tests/test_pack_digests.py > tests/golden/pack_digests.json
from a build of a commit whose packs are known good (the parent of the change under test), never
from the code under test."""
import ctypes
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from fastvideocodec_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_digests.json")


def _weights(n, seed=0, zero=False):
    """w[i] = (((i + seed) * 2654435761 mod 2^32) / 2^32 - 0.5) * 0.2, rounded once to float32"""
    if zero:
        return np.zeros(n, np.float32)
    h = ((np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return ((h.astype(np.float64) / 2.0 ** 32 - 0.5) * 0.2).astype(np.float32)


def _run(fn, w, nbytes, args_before=(), args_after=(), nosc=1):
    """fn(w, *args_before, pack, osc, *args_after) -> (pack bytes, osc floats)"""
    assert nbytes > 0
    wp = np.zeros(nbytes // 2, np.float16)
    osc = (ctypes.c_float * nosc)()
    _lib.call(fn, w.ctypes.data, *args_before, wp.ctypes.data, ctypes.addressof(osc), *args_after)
    return wp.tobytes(), list(osc)


def _f32(cin, cout, ks, stride, transposed, **kw):
    """the fp32 pack (fvc_conv_pack_weight): plain floats, no scale"""
    geo = (cin, cout, ks, stride, transposed)
    n = _lib.load().fvc_conv_wpack_floats(*geo)
    assert n > 0
    w = _weights(cin * cout * ks * ks, **kw)
    wp = np.zeros(n, np.float32)
    _lib.call("fvc_conv_pack_weight", w.ctypes.data, wp.ctypes.data, *geo)
    return wp.tobytes(), []


def _x3(cin, cout, ks, stride, transposed, **kw):
    geo = (cin, cout, ks, stride, transposed)
    nb = _lib.load().fvc_conv_x3_wpack_bytes(*geo)
    return _run("fvc_conv_x3_pack_weight", _weights(cin * cout * ks * ks, **kw), nb, args_after=geo)


def _x3_tap(np_, cin, **kw):
    """np_ partial rows x cin, packed in 32-row tiles as GdnTap does (one tile when np_ <= 32)"""
    w = _weights(np_ * cin, **kw).reshape(np_, cin)
    packs, oscs = b"", []
    for r0 in range(0, np_, 32):
        rows = np.ascontiguousarray(w[r0:r0 + 32])
        nb = _lib.load().fvc_x3_tap_wpack_bytes(rows.shape[0], cin)
        p, o = _run("fvc_x3_tap_pack_weight", rows, nb, args_after=(rows.shape[0], cin))
        packs += p
        oscs += o
    return packs, oscs


def _wino(**kw):
    return _run("fvc_conv_wino_pack_weight", _weights(64 * 64 * 9, **kw), _lib.load().fvc_conv_wino_wpack_bytes())


def _wino128(**kw):
    return _run("fvc_conv_wino128_pack_weight", _weights(128 * 128 * 9, **kw),
                _lib.load().fvc_conv_wino128_wpack_bytes(), nosc=4)


def _wino_tap(np_, **kw):
    return _run("fvc_wino_tap_pack_weight", _weights(np_ * 64, **kw), _lib.load().fvc_wino_tap_wpack_bytes(np_),
                args_after=(np_,))


def _wr7(cin, cout, ci0, co0, nt, **kw):
    return _run("fvc_conv_wr7_pack_weight", _weights(cout * cin * 49, **kw), _lib.load().fvc_conv_wr7_wpack_bytes(nt),
                args_before=(cin, cout, ci0, co0, nt))


def _stem(cin, cout, k, **kw):
    return _run("fvc_conv_stem_pack_weight", _weights(cout * cin * k * k, **kw),
                _lib.load().fvc_conv_stem_wpack_bytes(cin, cout, k), args_before=(cin, cout, k))


CASES = {
    "f32 8->16 3x3 s1": lambda: _f32(8, 16, 3, 1, 0, seed=18),
    "f32 128->128 3x3 s1 pipelined": lambda: _f32(128, 128, 3, 1, 0, seed=19),
    "f32 64->64 3x3 s2": lambda: _f32(64, 64, 3, 2, 0, seed=20),
    "f32 16->2 7x7 s1 small-N py4": lambda: _f32(16, 2, 7, 1, 0, seed=21),
    "f32 32->3 3x3 s1 small-N py2": lambda: _f32(32, 3, 3, 1, 0, seed=22),
    "f32 64->64 5x5 s2 transposed": lambda: _f32(64, 64, 5, 2, 1, seed=23),
    "f32 16->2 5x5 s2 transposed small-N": lambda: _f32(16, 2, 5, 2, 1, seed=24),
    "f32 3->64 5x5 s2 cc4": lambda: _f32(3, 64, 5, 2, 0, seed=25),
    "x3 64->64 3x3 s1": lambda: _x3(64, 64, 3, 1, 0, seed=1),
    "x3 8->16 3x3 s1 pair-tap": lambda: _x3(8, 16, 3, 1, 0, seed=2),
    "x3 64->64 5x5 s2 transposed": lambda: _x3(64, 64, 5, 2, 1, seed=3),
    "x3 128->64 3x3 s2": lambda: _x3(128, 64, 3, 2, 0, seed=4),
    "x3 64->64 3x3 s1 zero": lambda: _x3(64, 64, 3, 1, 0, zero=True),
    "x3 tap np18 cin128": lambda: _x3_tap(18, 128, seed=5),
    "x3 tap np75 cin64 tiles": lambda: _x3_tap(75, 64, seed=6),
    "x3 tap np18 cin128 zero": lambda: _x3_tap(18, 128, zero=True),
    "wino 64->64": lambda: _wino(seed=7),
    "wino 64->64 zero": lambda: _wino(zero=True),
    "wino128": lambda: _wino128(seed=8),
    "wino tap np18": lambda: _wino_tap(18, seed=9),
    "wino tap np18 zero": lambda: _wino_tap(18, zero=True),
    "wr7 32->64 ci0 0 co0 32 nt2": lambda: _wr7(32, 64, 0, 32, 2, seed=10),
    "wr7 64->32 ci0 0 nt2": lambda: _wr7(64, 32, 0, 0, 2, seed=11),
    "wr7 64->32 ci0 32 nt2": lambda: _wr7(64, 32, 32, 0, 2, seed=11),
    "wr7 32->16 nt1": lambda: _wr7(32, 16, 0, 0, 1, seed=12),
    "wr7 32->16 nt1 zero": lambda: _wr7(32, 16, 0, 0, 1, zero=True),
    "stem 6->64 3x3": lambda: _stem(6, 64, 3, seed=13),
    "stem 2->128 3x3": lambda: _stem(2, 128, 3, seed=14),
    "stem 3->64 5x5": lambda: _stem(3, 64, 5, seed=15),
    "stem 8->128 5x5": lambda: _stem(8, 128, 5, seed=16),
    "stem 1->64 3x3": lambda: _stem(1, 64, 3, seed=17),
    "stem 6->64 3x3 zero": lambda: _stem(6, 64, 3, zero=True),
}


def _digest(name):
    pack, osc = CASES[name]()
    return {"sha256": hashlib.sha256(pack).hexdigest(), "bytes": len(pack),
            "osc_bits": [struct.pack(">f", v).hex() for v in osc]}


if __name__ != "__main__":
    with open(GOLDEN) as f:
        _GOLDEN = json.load(f)


def test_golden_covers_every_case():
    assert sorted(_GOLDEN) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_pack_matches_recorded_digest(name):
    assert _digest(name) == _GOLDEN[name]


def test_zero_weights_take_unit_scale():
    for name in CASES:
        if name.endswith(" zero"):
            _, osc = CASES[name]()
            # kw = 0: scale 1 (wr7 folds its 2^4 V scale into osc)
            assert osc == [16.0 if name.startswith("wr7") else 1.0] * len(osc), name


if __name__ == "__main__":
    json.dump({name: _digest(name) for name in CASES}, sys.stdout, indent=1)
    sys.stdout.write("\n")
