"""Live per-kernel timing with HIP events on the launching stream (used by bench.py).

When a ``KernelTimer`` is active, every ``PackedConv`` launch goes through ``timed_conv``, which
brackets it with a start/end ``torch.cuda.Event`` pair on the current stream (the stream the kernel
is launched on) and appends one ``ConvRecord``: the events and the launch's algorithmic FLOPs and
bytes, its label, kernel family and dispatch count. The HBM-bound kernels go through ``timed_hbm``
in the same way. Events only; no host synchronisation until ``collect``. With no timer active both
helpers run the launch and nothing else.
"""
from __future__ import annotations

from typing import Any, NamedTuple

import torch

_ACTIVE = None


def conv_flops(cin, cout, k, stride, transposed, batch, h, w):
    """Algorithmic FLOPs (2 x MAC, unpadded channels) of one conv / deconv launch."""
    if transposed:
        # every input pixel scatters k*k taps into the output: MAC = B*h*w*cin*cout*k*k
        return 2.0 * batch * h * w * cin * cout * k * k
    ho, wo = h // stride, w // stride
    return 2.0 * batch * ho * wo * cin * cout * k * k


class ConvRecord(NamedTuple):
    """One conv call under a KernelTimer (a tuple: bench.py and the scripts also read it by position)."""
    ev0: Any         # torch.cuda.Event before / after the launch(es) of the call
    ev1: Any
    flops: float     # algorithmic (conv_flops, plus a fused tap consumer's MACs)
    key: str         # geometry + kernel label: the breakdown's row
    x3: bool         # split-precision launch
    nbytes: int      # algorithmic HBM bytes: input + packed weights + output (+ residual), each once
    family: str      # "stem" | "wr7" | "wino" | "dx" | "x3" | "f32"
    dispatches: int  # kernel dispatches, as rocprofv3 counts them


class KernelTimer:
    def __init__(self):
        self.records = []      # ConvRecord
        self.hbm_records = []  # (ev0, ev1, name, algorithmic bytes) of the HBM-bound kernels

    def __enter__(self):
        global _ACTIVE
        _ACTIVE = self
        return self

    def __exit__(self, *exc):
        global _ACTIVE
        _ACTIVE = None

    def _select(self, x3, family):
        return [r for r in self.records if (x3 is None or r.x3 == x3) and (family is None or r.family == family)]

    def collect(self, x3=None, family=None):
        """Synchronise and return (total_ms, total_flops, n_launches); x3=True/False restricts to
        the split-precision / the fp32+VALU conv launches, family to one kernel ('x3': the direct
        conv_x3_kernel, 'wino': conv_wino_kernel, 'f32'). n_launches counts kernel dispatches (the
        128-channel Winograd quarters are 4 per call), as rocprofv3 does."""
        torch.cuda.synchronize()
        rs = self._select(x3, family)
        ms = sum(r.ev0.elapsed_time(r.ev1) for r in rs)
        return ms, sum(r.flops for r in rs), sum(r.dispatches for r in rs)

    def collect_bytes(self, x3=None, family=None):
        """Algorithmic HBM bytes (input + packed weights + output + residual) of the launches
        ``collect(x3, family)`` counts."""
        return sum(r.nbytes for r in self._select(x3, family))

    def collect_hbm(self):
        """{name: [launches, ms, algorithmic bytes]} of the HBM-bound (non-conv) kernels."""
        torch.cuda.synchronize()
        agg = {}
        for ev0, ev1, name, nbytes in self.hbm_records:
            a = agg.setdefault(name, [0, 0.0, 0.0])
            a[0] += 1
            a[1] += ev0.elapsed_time(ev1)
            a[2] += nbytes
        return agg

    def breakdown(self):
        """Per-geometry aggregate: {key: [launches, ms, flops]} (keys recorded by the caller)."""
        torch.cuda.synchronize()
        agg = {}
        for r in self.records:
            a = agg.setdefault(r.key, [0, 0.0, 0.0])
            a[0] += 1
            a[1] += r.ev0.elapsed_time(r.ev1)
            a[2] += r.flops
        return agg


def active():
    return _ACTIVE


def timed_hbm(name, nbytes, fn):
    """Run fn (one HBM-bound kernel launch); with a KernelTimer active, bracket it with HIP events
    on the current stream and record its algorithmic bytes (each input read once, each output
    written once, padded channels included: they are moved)."""
    t = _ACTIVE
    if t is None:
        return fn()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    r = fn()
    ev1.record()
    t.hbm_records.append((ev0, ev1, name, float(nbytes)))
    return r


def timed_conv(launch, describe):
    """Run launch (the kernel launches of one conv call); with a KernelTimer active, bracket it with
    HIP events on the current stream and append ConvRecord(ev0, ev1, *describe()). describe returns
    (flops, key, x3, nbytes, family, dispatches) and is called under a timer only: the untimed path
    (a pipeline whose every launch is issued from Python) pays for no label, FLOP or byte count."""
    t = _ACTIVE
    if t is None:
        return launch()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    r = launch()
    ev1.record()
    t.records.append(ConvRecord(ev0, ev1, *describe()))
    return r
