"""What a KernelTimer records for one call of every launch variant of kernels.py (PackedConv.__call__ per
family, call_pool, call_up, call_tap, the tap form, TapConsumer.gather, GdnTap) must stay what
tests/golden/timer_records.json holds: (flops, key, x3, nbytes, family, dispatches) of every conv record
and (name, nbytes) of every HBM record. bench.py's roofline pass and --breakdown are built from them.

Weights and inputs are filled by integer arithmetic (no RNG stream to drift). Each case asserts the pack
flags that identify its path, so a case cannot change path unnoticed. The golden file is regenerated on
an MI355X with
    python tests/test_gpu_timer_records.py > tests/golden/timer_records.json
from a checkout whose records are known good (the parent of the change under test), never from the code
under test."""
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from fastvideocodec_amd import kernels as K
from fastvideocodec_amd import profiling

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "timer_records.json")


def _fill(shape, seed, amp):
    """t[i] = (((i + seed) * 2654435761 mod 2^32) / 2^32 - 0.5) * amp, rounded once to float32"""
    n = 1
    for s in shape:
        n *= s
    h = ((torch.arange(n, dtype=torch.int64) + seed) * 2654435761) & 0xFFFFFFFF
    return ((h.double() / 2.0 ** 32 - 0.5) * amp).float().reshape(shape)


def _pack(dev, cin, cout, k, stride, transposed=False, precision="x3", seed=1):
    w = _fill((cin, cout, k, k) if transposed else (cout, cin, k, k), seed, 0.2)
    return K.PackedConv(w, _fill((cout,), seed + 1, 0.1), k, stride, transposed, dev, precision=precision)


def _consumer(cls, dev, cin, cout, k, stride, transposed, seed=5):
    w = _fill((cin, cout, k, k) if transposed else (cout, cin, k, k), seed, 0.2)
    return cls(w, _fill((cout,), seed + 1, 0.1), k, stride, transposed, dev)


def _x(dev, b, h, w, c, seed=3):
    x = _fill((b, h, w, K.cp4(c)), seed, 1.0)
    x[..., c:] = 0.0
    return x.to(dev)


def _direct(p):
    """a plain split-precision pack: nothing but the direct x3 kernel can take it"""
    return p.x3 and p.tap is None and p.stem is None and not (p.wino or p.wino128 or p.dx or p.wr7)


def _f32(dev):
    p = _pack(dev, 64, 64, 3, 1, precision="f32")
    assert not p.x3 and not p.wino and p.tap is None
    p(_x(dev, 2, 16, 16, 64))


def _x3_s2(dev, with_res=False, batch=2):
    p = _pack(dev, 128, 128, 3, 2)
    assert _direct(p)
    p(_x(dev, batch, 16, 16, 128), act=K.ACT_LRELU, res=_x(dev, batch, 8, 8, 128, seed=4) if with_res else None)


def _x3_in_abs(dev):
    p = _pack(dev, 64, 64, 3, 1)
    assert p.wino and not p.wino128
    p(_x(dev, 2, 16, 16, 64), in_op=K.IN_ABS)


def _dx(dev):
    p = _pack(dev, 128, 128, 3, 2, transposed=True)
    assert p.x3 and p.dx and p.tap is None and not p.wino
    p(_x(dev, 2, 16, 16, 128), act=K.ACT_LRELU)


def _wino(dev, with_res=False):
    p = _pack(dev, 64, 64, 3, 1)
    assert p.wino and not p.wino128 and p.tap is None
    if with_res:
        p(_x(dev, 2, 16, 16, 64), in_op=K.IN_RELU, act=K.ACT_RELU, res=_x(dev, 2, 16, 16, 64, seed=4))
    else:
        p(_x(dev, 2, 16, 16, 64))


def _wino128(dev):
    p = _pack(dev, 128, 128, 3, 1)
    assert p.wino128 and not p.wino and p.tap is None
    p(_x(dev, 2, 16, 16, 128), act=K.ACT_RELU)


def _wr7(dev, cin, cout, launches):
    p = _pack(dev, cin, cout, 7, 1)
    assert len(p.wr7) == launches and [m for _, _, _, m, _, _ in p.wr7] == ([1, 2] if cin == 64 else [0] * launches)
    assert all(nt == (1 if cout == 16 else 2) for _, _, nt, _, _, _ in p.wr7)
    p(_x(dev, 2, 16, 16, cin), act=K.ACT_RELU)


def _stem(dev):
    p = _pack(dev, 4, 64, 3, 2)
    assert p.stem is not None
    p(_x(dev, 2, 16, 34, 4), act=K.ACT_RELU)


def _stem_off(dev):
    p = _pack(dev, 6, 64, 3, 1)
    assert p.stem is None and p.x3 and not p.wino
    p(_x(dev, 2, 16, 16, 6), act=K.ACT_RELU)


def _tap_form(dev):
    p = _pack(dev, 128, 2, 3, 1)
    assert p.tap is not None and p.x3 and _direct(p.tap) and (p.tap.cin, p.tap.cout, p.tap.ksize) == (128, 18, 1)
    p(_x(dev, 2, 16, 16, 128), res=_x(dev, 2, 16, 16, 2, seed=4))


def _pool(dev, wino):
    p = _pack(dev, 64, 64, 3, 1)
    assert p.wino == wino and p.pool_fusable()
    p.call_pool(_x(dev, 2, 16, 16, 64), act=K.ACT_RELU, res=_x(dev, 2, 16, 16, 64, seed=4))


def _up(dev):
    p = _pack(dev, 64, 64, 3, 1)
    assert p.up_fusable()
    p.call_up(_x(dev, 2, 16, 16, 64), _x(dev, 2, 8, 8, 64, seed=4), in_op=K.IN_RELU, act=K.ACT_RELU)


def _tap_wino(dev):
    p = _pack(dev, 64, 64, 3, 1)
    t = _consumer(K.TapConsumer, dev, 64, 2, 3, 1, False)
    assert (t.np, t.pcp) == (18, 20) and t.wino_wpack is not None
    assert p.wino and p.tap_fusable(t) and p._wino_tap(t)
    P = p.call_tap(_x(dev, 2, 16, 16, 64), t, res=_x(dev, 2, 16, 16, 64, seed=4))
    t.gather(P, res=_x(dev, 2, 16, 16, 2, seed=6))


def _tap_dx(dev):
    p = _pack(dev, 128, 128, 3, 2, transposed=True)
    t = _consumer(K.TapConsumer, dev, 128, 2, 3, 2, True)
    assert (t.np, t.pcp) == (18, 20) and t.wino_wpack is None
    assert p.dx and p.tap_fusable(t) and not p._wino_tap(t)
    P = p.call_tap(_x(dev, 2, 16, 16, 128), t, act=K.ACT_LRELU)
    assert tuple(P.shape) == (2, 32, 32, 20)
    y = t.gather(P)
    assert tuple(y.shape) == (2, 64, 64, 4)


def _gdn_tap(dev):
    t = _consumer(K.GdnTap, dev, 64, 3, 5, 2, True)
    assert (t.np, t.pcp, t.ntiles) == (75, 76, 3)
    beta = (_fill((64,), 7, 1.0) + 1.0).to(dev)
    gamma = (_fill((64, 64), 8, 0.05) + 0.025 + torch.eye(64) * 0.2).to(dev)
    t(_x(dev, 2, 16, 16, 64), beta, gamma, True, res=_x(dev, 2, 32, 32, 3, seed=4))


# name: (environment switches set before the pack is built, the case)
CASES = {
    "f32 64->64 3x3 s1": ({}, _f32),
    "x3 128->128 3x3 s2": ({}, _x3_s2),
    "x3 128->128 3x3 s2 +res": ({}, lambda dev: _x3_s2(dev, with_res=True)),
    "x3 64->64 3x3 s1 in_abs on a wino pack": ({}, _x3_in_abs),
    "dx deconv 128->128 3x3 s2": ({}, _dx),
    "wino 64->64": ({}, _wino),
    "wino 64->64 +res in_relu": ({}, lambda dev: _wino(dev, with_res=True)),
    "wino128 quarters": ({"FVC_WINO128_MINPIX": "0"}, _wino128),
    "wino128 pack below the pixel gate": ({}, _wino128),
    "wr7 32->64": ({}, lambda dev: _wr7(dev, 32, 64, 2)),
    "wr7 64->32 modes 1+2": ({}, lambda dev: _wr7(dev, 64, 32, 2)),
    "wr7 32->16 nt1": ({}, lambda dev: _wr7(dev, 32, 16, 1)),
    "stem 4->64 3x3 s2": ({}, _stem),
    "stem off 6->64 3x3 s1": ({"FVC_STEM": "0"}, _stem_off),
    "tap form 128->2 3x3 s1": ({}, _tap_form),
    "call_pool wino": ({}, lambda dev: _pool(dev, True)),
    "call_pool direct": ({"FVC_WINO": "0"}, lambda dev: _pool(dev, False)),
    "call_up": ({}, _up),
    "call_tap wino 64->64 -> 64->2": ({}, _tap_wino),
    "call_tap dx deconv 128->128 -> deconv 128->2": ({}, _tap_dx),
    "gdn+tap 64->3 5x5 s2": ({}, _gdn_tap),
    # 4 images of 8 x 8 x 128 floats (32 KiB each): 4 reach the limit, 2 do not -> two dispatches
    "x3 128->128 3x3 s2 batch split": ({"FVC_X3_SPLIT_BYTES": str(3 * 8 * 8 * 128 * 4)},
                                       lambda dev: _x3_s2(dev, batch=4)),
}


def _records(name, dev, setenv):
    env, case = CASES[name]
    for k, v in env.items():
        setenv(k, v)
    with profiling.KernelTimer() as timer:
        case(dev)
    torch.cuda.synchronize()
    return {"conv": [list(r[2:8]) for r in timer.records], "hbm": [list(r[2:4]) for r in timer.hbm_records]}


if __name__ != "__main__":
    with open(GOLDEN) as f:
        _GOLDEN = json.load(f)


def test_golden_covers_every_case():
    assert sorted(_GOLDEN) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_records_match_golden(dev, name, monkeypatch):
    got = _records(name, dev, monkeypatch.setenv)
    print(name, got)
    assert got == _GOLDEN[name]


if __name__ == "__main__":
    out = {}
    for name in CASES:
        saved = dict(os.environ)
        out[name] = _records(name, torch.device("cuda:0"), os.environ.__setitem__)
        os.environ.clear()
        os.environ.update(saved)
    json.dump(out, sys.stdout, indent=1)
    sys.stdout.write("\n")
