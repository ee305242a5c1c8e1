"""The RLVC entropy and recurrent kernels one at a time against float64 restatements of the
same operation (oracle/rlvc_ref.py, oracle/dvc_ref.py evaluated in float64 on the float32
inputs): fvc_gc_forward, fvc_eb_forward, fvc_bits_laplace, fvc_bits_factorized, fvc_rpm_scale,
fvc_lstm_gates, fvc_gdn_nhwc_cai -- at the tails, the 0.11 scale bound, the 1e-9 likelihood
bound, the sum == 0 branch of the bottleneck's sign trick, rounding ties, non-integer means,
pixel counts off the group size and a channel pitch above the channel count.

Rate sums. The kernels return one float64 sum, so the tolerance is built from the reference:
per element the bits are evaluated on the CPU in float32 (b32) and float64 (b64) by one formula,
S64 = sum b64, B32 = sum |b32 - b64| (unsigned: a pessimistic float32 budget), and the device sum
must satisfy |dev - S64| <= 4 * B32 + 1e-12 * S64. The margin of 4 covers device libm against
host libm (a few ulp each) and eb_logits' fmaf where torch's matmul need not fuse.
test_rate_case_conditions checks without a GPU that 4 * B32 < 0.05 bits for every case, that
at least 90 % of the elements cost 0.1 bits or more (one dropped or doubled element shows) and
that every named edge class is in the inputs; test_rate_size_case_conditions does the same for
the one-element case and for the case whose 264264 elements make the fixed grid stride.

Measured |dev - S64| / B32 on an MI355X (S64 and B32 are the CPU's, in bits):

    kernel            C  elements        S64      B32   |dev - S64| / B32
    gc_forward       12       840    11661.5  1.5e-03   0.08
    gc_forward       96      4032    55340.1  6.9e-03   0.54
    gc_forward        1         1        3.1  2.0e-07   1.00
    gc_forward       12    264264  3648704.0  4.7e-01   0.47
    eb_forward       12       840     7470.5  1.5e-03   0.15
    eb_forward       96      4032    35930.0  7.2e-03   0.21
    eb_forward        1         1        5.6  3.2e-07   1.00
    eb_forward       12    264264  2344096.4  4.6e-01   0.18
    bits_laplace     12       840     6664.8  2.3e-03   0.54
    bits_laplace     96      4032    32050.6  7.6e-03   1.20
    bits_laplace      1         1        4.0  1.6e-06   1.30
    bits_laplace     12    264264  2104790.9  1.2e-01   1.80
    bits_factorized  12       840     7131.4  4.3e-03   0.08
    bits_factorized  96      4032    35040.7  6.9e-03   0.18
    bits_factorized   1         1        4.3  7.2e-07   1.00
    bits_factorized  12    264264  2294655.3  4.0e-01   0.20

(a ratio of exactly 1.00 on one element: the device and the CPU's float32 give the same value.)
The elementwise kernels' worst measured e_dev / e_cpu32: rpm_scale 1.21, lstm_gates 1.00 (the same
float32 values as torch's), gdn_cai 2.40 of the tensor maximum and 1.41 relative to each output.

Encoder x_hat. fvc_gc_forward / fvc_eb_forward write x_hat = rint(x - m) + m; it must be the
float32 CPU value bit for bit (the float64 value differs: float32 is what the decoder adds) and
the bits of fvc_dequantize_symbols(fvc_quantize_symbols(x, m), m), the decoder's latent.

fvc_rpm_scale, fvc_lstm_gates and fvc_gdn_nhwc_cai are compared elementwise with the bound of
test_gdn_x3_*: e_dev <= 4 * e_cpu32 + 1e-7 * scale, e_cpu32 the float32 torch CPU evaluation's
own error against float64.
"""
import functools
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import rlvc_ref as R  # noqa: E402

from fastvideocodec_amd import _lib  # noqa: E402
from fastvideocodec_amd import kernels as K  # noqa: E402
from fastvideocodec_amd import rlvc  # noqa: E402
from fastvideocodec_amd.net import BitEstimator, _GDNP  # noqa: E402

D = R.D  # oracle/dvc_ref.py, the module rlvc_ref itself uses
gpu = pytest.mark.gpu
CSRC = os.path.join(ROOT, "fastvideocodec_amd", "csrc")
FVC_EINVAL = -1000  # include/fvc.h


def _const(fname, name):
    with open(os.path.join(CSRC, fname)) as f:
        return int(re.search(rf"constexpr int {name} = (\d+);", f.read()).group(1))


K_BLK = _const("fvc_elem.hip", "kBlk")
K_RED_BLOCKS = _const("fvc_elem.hip", "kRedBlocks")
K_GC_PIX = _const("fvc_gdn.hip", "kGcPix")
LAUNCH_N_CAP = 8192  # launch_n's and fvc_gdn_nhwc_cai's block cap

SENTINEL = -7777.25
SHAPES = {12: (2, 5, 7), 96: (2, 3, 7)}  # B = 2, odd H and W; 840 and 4032 elements
# more elements than the fixed reduction grid has threads: its loop strides
STRIDE_SHAPE = (2, 91, 121)
assert 2 * 91 * 121 * 12 > K_RED_BLOCKS * K_BLK
F32_0P11 = float(torch.tensor(0.11, dtype=torch.float32))
BOUND_BITS = -math.log2(1e-5 + 1e-9)  # an element whose likelihood sits on the 1e-9 bound


def _bits(lik):
    """Per element, what estimate_bits (rlvc_ref) and bits_laplace / bits_factorized (dvc_ref) sum."""
    return torch.clamp(-1.0 * torch.log(lik + 1e-5) / math.log(2.0), 0, 50)


def _dbl(t):
    return {k: v.double() for k, v in t.items()} if isinstance(t, dict) else t.double()


class Case:
    """One rate-sum case: NHWC float32 inputs [B,H,W,C], the kernel's parameter tensors, the CPU's
    per-element bits in both precisions, the float32 x_hat (GC / EB) and the edge-class masks."""

    def __init__(self, kind, C, shape, ins, params, b32, b64, classes, xhat32=None, mean=None, sum32=None):
        self.kind, self.C, self.shape = kind, C, shape
        self.ins, self.params = ins, params
        self.b32, self.b64, self.classes = b32, b64, classes
        self.xhat32, self.mean = xhat32, mean
        self.S64 = float(b64.sum())
        self.B32 = float((b32.double() - b64).abs().sum())
        self.sum32 = sum32


def _nhwc_flat(t, shape, C):
    return t.view(*shape, C).contiguous()


# ------------------------------------------------------------------ GaussianConditional
@functools.lru_cache(maxsize=None)
def gc_case(C, shape=None):
    shape = shape or SHAPES[C]
    N = shape[0] * shape[1] * shape[2] * C
    g = torch.Generator().manual_seed(1000 + C + N)
    i = torch.arange(N)
    scale = torch.exp(1.5 * torch.randn(N, generator=g))  # log-normal
    d = torch.linspace(-40.0, 40.0, N)[torch.randperm(N, generator=g)] if N > 1 else torch.tensor([-7.3])
    mu = torch.rand(N, generator=g) * 6 - 3
    named = torch.tensor([0.0, -1.0, 0.05, F32_0P11, 1e3])
    sel = i % 8 == 0
    scale[sel] = named[(i[sel] // 8) % 5]
    # rounding ties: x - mu exact in float32 (mu a multiple of 1/8), both signs round half to even
    ties = torch.tensor([0.5, -0.5, 1.5, -1.5, 2.5, -2.5])
    t = i % 11 == 3
    k = i[t] // 11
    d[t] = ties[k % 6]
    mu[t] = ((k % 17) - 8).float() / 8
    # the far tail at the scale bound: the likelihood underflows to its 1e-9 bound
    far = i % 97 == 5
    scale[far] = F32_0P11
    d[far] = torch.where((i[far] // 97) % 2 == 0, 40.0, -40.0)
    if N == 1:  # the one-element case: an ordinary element, a few bits
        scale, d, mu = torch.tensor([1.7]), torch.tensor([-2.3]), torch.tensor([0.37])
    x = mu + d
    x, scale, mu = (_nhwc_flat(v, shape, C) for v in (x, scale, mu))
    xhat32, lik32 = R.gc_forward(x, scale, mu)
    xhat64, lik64 = R.gc_forward(x.double(), scale.double(), mu.double())
    b32, b64 = _bits(lik32), _bits(lik64)
    dd = x - mu
    classes = {
        "scale 0": scale == 0, "scale negative": scale < 0, "scale 0.05": scale == 0.05,
        "scale exactly 0.11": scale == F32_0P11, "scale 1e3": scale == 1e3,
        "|x - mu| near 40 at scale 0.11, on the likelihood bound":
            (scale == F32_0P11) & (dd.abs() > 39.5) & ((b64 - BOUND_BITS).abs() < 1e-9),
        "non-integer mu": mu != torch.round(mu),
        "same symbol in float32 and float64": None,
    }
    for v in ties.tolist():
        classes[f"x - mu == {v}"] = dd == v
    classes["same symbol in float32 and float64"] = torch.round(dd).double() == torch.round(x.double() - mu.double())
    return Case("gc", C, shape, [x, scale, mu], [], b32, b64, classes, xhat32, mu, float(R.estimate_bits(lik32)))


# ------------------------------------------------------------------ EntropyBottleneck
EB_PREFIX = "eb"


@functools.lru_cache(maxsize=None)
def eb_params(C):
    """compressai's initialisation (init_scale 10, filters (3,3,3,3)) plus 0.3 noise; medians
    non-zero and non-integer, except in every fourth channel, whose biases and median are 0:
    there the logits are an odd function of x (tanh and the products are odd), so at x == median
    lower + upper is exactly 0 in any precision."""
    g = torch.Generator().manual_seed(2000 + C)
    filters = (1,) + R.FILTERS + (1,)
    scale = 10.0 ** (1 / (len(R.FILTERS) + 1))
    sym = torch.arange(C) % 4 == 1
    sd = {}
    for i in range(len(R.FILTERS) + 1):
        init = math.log(math.expm1(1 / scale / filters[i + 1]))
        sd[f"{EB_PREFIX}._matrix{i}"] = init + 0.3 * torch.randn(C, filters[i + 1], filters[i], generator=g)
        b = torch.rand(C, filters[i + 1], 1, generator=g) - 0.5
        b[sym] = 0
        sd[f"{EB_PREFIX}._bias{i}"] = b
        if i < len(R.FILTERS):
            sd[f"{EB_PREFIX}._factor{i}"] = 0.3 * torch.randn(C, filters[i + 1], 1, generator=g)
    med = torch.rand(C, generator=g) * 6 - 3
    med[sym] = 0
    sd[f"{EB_PREFIX}.quantiles"] = torch.stack((med - 10, med, med + 10), 1).view(C, 1, 3).contiguous()
    return sd, med, sym


def eb_kernel_params(C):
    """[C, 58] parameter rows and medians as the product packs them (host float32)."""
    sd, _, _ = eb_params(C)
    eb = rlvc.LearnedEntropyBottleneck(C, device="cpu")
    eb.load_state_dict({k[len(EB_PREFIX) + 1:]: v for k, v in sd.items()})
    eb.invalidate()
    return eb.kernel_params()


def _eb_eval(sd, x_nhwc):
    """R.eb_forward on an NHWC tensor -> NHWC (x_hat, likelihood, lower + upper)."""
    xc = x_nhwc.permute(0, 3, 1, 2).contiguous()
    out, lik = R.eb_forward(sd, EB_PREFIX, xc)
    C = xc.shape[1]
    o = out.permute(1, 0, 2, 3).reshape(C, 1, -1)
    s = R.eb_logits(sd, EB_PREFIX, o - 0.5) + R.eb_logits(sd, EB_PREFIX, o + 0.5)
    s = s.reshape(C, *out.permute(1, 0, 2, 3).shape[1:]).permute(1, 2, 3, 0)
    return out.permute(0, 2, 3, 1).contiguous(), lik.permute(0, 2, 3, 1).contiguous(), s.contiguous()


@functools.lru_cache(maxsize=None)
def eb_case(C, shape=None):
    shape = shape or SHAPES[C]
    sd, med, sym = eb_params(C)
    npix = shape[0] * shape[1] * shape[2]
    N = npix * C
    g = torch.Generator().manual_seed(3000 + C + N)
    x = (med + 12 * torch.randn(npix, C, generator=g)).view(-1)
    i = torch.arange(N)
    medf = med.repeat(npix)
    # 30 to 150 above and below the median: from 60 on the likelihood is 1e-4 .. 1e-9, where only
    # the sign trick (sigmoids of negative arguments) keeps float32 exact
    far = i % 7 == 2
    off = 30 + 120 * torch.rand(int(far.sum()), generator=g)
    x[far] = medf[far] + torch.where((i[far] // 7) % 2 == 0, off, -off)
    x = x.view(npix, C)
    p = torch.arange(npix)
    for c in torch.nonzero(sym).view(-1).tolist():  # the symmetric channels: x == median, and next to it
        x[p % 2 == 0, c] = med[c]
        x[p % 4 == 1, c] = med[c] + 0.3
    x = _nhwc_flat(x, shape, C)
    xhat32, lik32, s32 = _eb_eval(sd, x)
    xhat64, lik64, s64 = _eb_eval(_dbl(sd), x.double())
    b32, b64 = _bits(lik32), _bits(lik64)
    dd = x - med
    classes = {
        "non-zero non-integer median": ((med != 0) & (med != torch.round(med))).expand_as(x),
        "30 or more above the median": dd >= 30, "30 or more below the median": dd <= -30,
        "likelihood of 1e-8 .. 1e-5 above the median": (dd > 0) & (lik64 > 1e-8) & (lik64 < 1e-5),
        "likelihood of 1e-8 .. 1e-5 below the median": (dd < 0) & (lik64 > 1e-8) & (lik64 < 1e-5),
        "lower + upper == 0 in float32": s32 == 0, "lower + upper == 0 in float64": s64 == 0,
        "lower + upper == 0 costs the likelihood bound": (s64 == 0) & ((b64 - BOUND_BITS).abs() < 1e-9),
        "lower + upper > 0": s64 > 0, "lower + upper < 0": s64 < 0,
        "same symbol in float32 and float64": torch.round(dd).double() == torch.round(x.double() - med.double()),
    }
    prm, medk = eb_kernel_params(C)
    return Case("eb", C, shape, [x], [prm, medk], b32, b64, classes, xhat32, med.expand_as(x).contiguous(),
                float(R.estimate_bits(lik32)))


# ------------------------------------------------------------------ DVC rate kernels
def _laplace_lik(feature, sigma):
    """dvc_ref.bits_laplace's probability, per element."""
    sigma = sigma.clamp(1e-5, 1e10)
    lap = torch.distributions.laplace.Laplace(torch.zeros_like(sigma), sigma)
    return lap.cdf(feature + 0.5) - lap.cdf(feature - 0.5)


@functools.lru_cache(maxsize=None)
def laplace_case(C, shape=None):
    """float32 forms the probability as a difference of two CDFs near 0.5 or 1, an absolute error of
    a few 1e-8 whatever the probability, so an element in the transition between centre and far
    tail (p of 1e-7 .. 1e-3) costs float32 up to 1e-2 bits. The inputs therefore sit in the
    centre (|f| <= 2 sigma, sigma 0.5 .. 3), in the far tail (|f| 20 .. 60 at more than 30 sigma:
    p underflows in both precisions) or at a named sigma, with one element in the transition."""
    shape = shape or SHAPES[C]
    N = shape[0] * shape[1] * shape[2] * C
    g = torch.Generator().manual_seed(4000 + C + N)
    i = torch.arange(N)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(N, generator=g)
    sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    sigma = torch.exp(u(math.log(0.5), math.log(3.0)))
    feat = sigma * u(-2.0, 2.0)
    tail = (i % 10 >= 6) & (i % 10 <= 8)
    ft = sign * u(20.0, 60.0)
    feat[tail] = ft[tail]
    sigma[tail] = (ft.abs() / u(30.0, 1000.0))[tail]
    named = torch.tensor([0.0, 1e-7, 1e-5, 1e12])
    sel = i % 10 == 9
    sigma[sel] = named[(i[sel] // 10) % 4]
    feat[sel] = torch.where((i[sel] // 40) % 3 == 0, 0.3 * sign[sel], (sign * u(0.6, 60.0))[sel])
    mid = i == 7  # the transition: one element whatever the size
    sigma[mid] = 1.0
    feat[mid] = (sign * u(8.0, 16.0))[mid]
    feat[i % 211 == 17] = 60.0
    feat[i % 211 == 18] = -60.0
    if N == 1:  # the one-element case: an ordinary element, a few bits
        feat, sigma = torch.tensor([3.2]), torch.tensor([2.5])
    feat, sigma = _nhwc_flat(feat, shape, C), _nhwc_flat(sigma, shape, C)
    q = torch.round(feat)
    b32, b64 = _bits(_laplace_lik(q, sigma)), _bits(_laplace_lik(q.double(), sigma.double()))
    classes = {"sigma 0": sigma == 0, "sigma 1e-7": sigma == 1e-7, "sigma exactly 1e-5": sigma == 1e-5,
               "sigma 1e12": sigma == 1e12, "|feature| 60": feat.abs() == 60, "|feature| above 50": feat.abs() > 50,
               "feature rounds to 0 at a clamped sigma": (q == 0) & (sigma <= 1e-5),
               "feature away from 0 at a clamped sigma": (q != 0) & (sigma <= 1e-5),
               "transition between centre and tail": (sigma == 1.0) & (q.abs() >= 8) & (q.abs() <= 16)}
    return Case("laplace", C, shape, [feat, sigma], [], b32, b64, classes, sum32=float(D.bits_laplace(q, sigma)))


@functools.lru_cache(maxsize=None)
def _mv_estimator():
    from fastvideocodec_amd.weights import seeded_torch_state_dict
    pre = "bitEstimator_mv."
    return {k: v for k, v in seeded_torch_state_dict().items() if k.startswith(pre)}


@functools.lru_cache(maxsize=None)
def factorized_case(C, shape=None):
    """The seeded bitEstimator_mv parameters (its first C channels), |v| up to 60. The seeded
    estimator is wide (16.58 of the 16.61 bits of the bound at |v| = 60), and float32 takes the upper
    tail as a difference of two sigmoids near 1: 1e-4 bits of error per element at v = +25, 1e-2 at
    +60, against 1e-6 anywhere below 0. So the lower tail is a ramp down to -60, and the upper
    tail 23 elements up to +40: one element at +60 would be the whole float32 budget."""
    shape = shape or SHAPES[C]
    N = shape[0] * shape[1] * shape[2] * C
    g = torch.Generator().manual_seed(5000 + C + N)
    sd = {k: v[:, :C].contiguous() for k, v in _mv_estimator().items()}
    i = torch.arange(N)
    v = torch.where(i % 2 == 0, torch.rand(N, generator=g) * 20 - 10, -10 - 50 * torch.rand(N, generator=g))
    up = torch.cat((torch.linspace(10.0, 25.0, 20), torch.tensor([30.0, 30.0, 40.0])))
    if N > 1:
        v[(torch.arange(23) * (N // 23) + 5) % N] = up
        v[11 % N] = -60.0
    else:
        v = torch.tensor([-2.7])
    v = _nhwc_flat(v, shape, C)
    q = torch.round(v).permute(0, 3, 1, 2).contiguous()  # the oracle's parameters broadcast over NCHW
    est = lambda s, t: D.bit_estimator(s, "bitEstimator_mv", t + 0.5) - D.bit_estimator(s, "bitEstimator_mv", t - 0.5)
    b32 = _bits(est(sd, q)).permute(0, 2, 3, 1).contiguous()
    b64 = _bits(est(_dbl(sd), q.double())).permute(0, 2, 3, 1).contiguous()
    be = BitEstimator(C)
    be.load_state_dict({k[len("bitEstimator_mv."):]: t for k, t in sd.items()})
    classes = {"v == 40": v == 40, "v == -60": v == -60, "v below -50": v < -50, "v above 20": v > 20,
               "v rounds to 0": torch.round(v) == 0}
    return Case("factorized", C, shape, [v], [be.params()], b32, b64, classes,
                sum32=float(D.bits_factorized(sd, "bitEstimator_mv", q)))


CASES = {"gc": gc_case, "eb": eb_case, "laplace": laplace_case, "factorized": factorized_case}
RATE_IDS = [(kind, C) for kind in CASES for C in (12, 96)]


@pytest.mark.parametrize("kind,C", RATE_IDS)
def test_rate_case_conditions(kind, C):
    """What the 4 * B32 bound needs of the inputs, checked on the CPU alone."""
    case = CASES[kind](C)
    _describe(case)
    assert case.b64.numel() <= 4100 and case.shape[0] == 2 and case.shape[1] % 2 and case.shape[2] % 2
    assert 4 * case.B32 < 0.05, case.B32
    assert float((case.b64 >= 0.1).double().mean()) >= 0.9
    for name, mask in case.classes.items():
        if name.startswith("same symbol"):
            assert bool(mask.all()), name
        else:
            assert int(mask.sum()) > 0, name
    if case.xhat32 is not None:
        assert not bool((case.xhat32 == SENTINEL).any())


@pytest.mark.parametrize("kind", list(CASES))
def test_rate_size_case_conditions(kind):
    """The two cases that are about the pixel count: one element, and a fixed grid that strides.
    The second has 65 to 315 times the elements and as much more float32 budget: 4 * B32 stays
    below 10 bits, where the elements past the grid's first pass are thousands of bits."""
    one, big = CASES[kind](1, (1, 1, 1)), CASES[kind](12, STRIDE_SHAPE)
    _describe(one)
    _describe(big)
    assert one.b64.numel() == 1 and 1.0 < one.S64 < 16.0  # neither free nor on the likelihood bound
    n = big.b64.numel()
    assert n > K_RED_BLOCKS * K_BLK and 4 * big.B32 < 10.0
    assert float(big.b64.view(-1)[K_RED_BLOCKS * K_BLK:].sum()) > 1000.0
    assert float((big.b64 >= 0.1).double().mean()) >= 0.9
    for name, mask in big.classes.items():
        if name.startswith("same symbol"):
            assert bool(mask.all()), name


def _describe(case):
    n = case.b64.numel()
    print(f"{case.kind} C={case.C} {case.shape}: n {n} S64 {case.S64:.4f} B32 {case.B32:.3e} "
          f"max |b32 - b64| {float((case.b32.double() - case.b64).abs().max()):.2e} min b64 {float(case.b64.min()):.3f}")
    assert bool(torch.isfinite(case.b64).all()) and bool(torch.isfinite(case.b32).all())
    # the per-element restatement sums to the oracle's own (float32) sum
    assert abs(case.sum32 - float(case.b32.double().sum())) <= 1e-5 * case.S64 + 1e-6


# ------------------------------------------------------------------ device wrappers
def _pitched(t, cp, fill, dev):
    """[B,H,W,C] -> device [B,H,W,cp], the pad channels holding `fill`."""
    B, H, W, C = t.shape
    out = torch.full((B, H, W, cp), fill, dtype=t.dtype)
    out[..., :C] = t
    return out.to(dev)


def _i32(t):
    return t.contiguous().view(torch.int32)


def run_rate(case, dev, cp=None):
    """One call of the case's entry point as rlvc.py / kernels.py make it -> (sum: float, x_hat
    [B,H,W,cp] on the device or None). Pad channels of the inputs hold NaN, x_hat starts as SENTINEL."""
    C = case.C
    cp = cp or C
    B, H, W = case.shape
    ins = [_pitched(t, cp, float("nan"), dev) for t in case.ins]
    prm = [p.to(dev) for p in case.params]
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    ws = K._ws(dev)
    xhat = None
    dims = (B, H, W, C, cp, K.stream_handle())
    if case.kind == "gc":
        xhat = torch.full((B, H, W, cp), SENTINEL, device=dev)
        _lib.call("fvc_gc_forward", ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), xhat.data_ptr(),
                  out.data_ptr(), ws.data_ptr(), *dims)
    elif case.kind == "eb":
        xhat = torch.full((B, H, W, cp), SENTINEL, device=dev)
        _lib.call("fvc_eb_forward", ins[0].data_ptr(), prm[0].data_ptr(), prm[1].data_ptr(), xhat.data_ptr(),
                  out.data_ptr(), ws.data_ptr(), *dims)
    elif case.kind == "laplace":
        _lib.call("fvc_bits_laplace", ins[0].data_ptr(), ins[1].data_ptr(), out.data_ptr(), ws.data_ptr(), *dims)
    else:
        _lib.call("fvc_bits_factorized", ins[0].data_ptr(), prm[0].data_ptr(), out.data_ptr(), ws.data_ptr(), *dims)
    torch.cuda.synchronize()
    return float(out.cpu()[0]), xhat


def _check_sum(case, got, label):
    err = abs(got - case.S64)
    ratio = err / case.B32 if case.B32 > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{label}: dev {got:.6f} S64 {case.S64:.6f} B32 {case.B32:.3e} |dev - S64| / B32 = {ratio:.3f}")
    assert err <= 4 * case.B32 + 1e-12 * case.S64, (label, got, case.S64, case.B32, ratio)


# ------------------------------------------------------------------ 1. rate sums
@gpu
@pytest.mark.parametrize("kind,C", RATE_IDS)
def test_rate_sum_vs_float64(dev, kind, C):
    case = CASES[kind](C)
    got, _ = run_rate(case, dev)
    _check_sum(case, got, f"{kind} C={C}")
    again, _ = run_rate(case, dev)
    assert np.float64(got).tobytes() == np.float64(again).tobytes()  # deterministic, to the bit


@gpu
@pytest.mark.parametrize("kind,C", RATE_IDS)
def test_rate_sum_ignores_pad_channels(dev, kind, C):
    """cp = C + 4 with NaN in the four pad channels of every input: the same sum to the bit, and
    x_hat's pad channels keep their sentinel."""
    case = CASES[kind](C)
    tight, xh_tight = run_rate(case, dev)
    assert math.isfinite(tight)
    padded, xh = run_rate(case, dev, cp=C + 4)
    assert np.float64(tight).tobytes() == np.float64(padded).tobytes(), (tight, padded)
    if xh is not None:
        xh = xh.cpu()
        assert bool((xh[..., C:] == SENTINEL).all())
        assert torch.equal(_i32(xh[..., :C]), _i32(xh_tight.cpu()))


@gpu
@pytest.mark.parametrize("kind", list(CASES))
def test_rate_sum_one_pixel_and_strided_grid(dev, kind):
    """npix = 1 with C = 1, and more elements than the fixed reduction grid has threads."""
    one = CASES[kind](1, (1, 1, 1))
    got, xh = run_rate(one, dev)
    _check_sum(one, got, f"{kind} one element")
    big = CASES[kind](12, STRIDE_SHAPE)
    assert big.b64.numel() > K_RED_BLOCKS * K_BLK
    got, xh = run_rate(big, dev)
    _check_sum(big, got, f"{kind} {big.b64.numel()} elements")
    if xh is not None:
        assert torch.equal(_i32(xh.cpu()), _i32(big.xhat32))


# ------------------------------------------------------------------ 2. x_hat
@gpu
@pytest.mark.parametrize("cpad", [0, 4])
@pytest.mark.parametrize("kind,C", [(k, c) for k, c in RATE_IDS if k in ("gc", "eb")])
def test_xhat_is_the_decoders_latent(dev, kind, C, cpad):
    case = CASES[kind](C)
    _, xh = run_rate(case, dev, cp=C + cpad)
    x_hat = xh[..., :C].contiguous()
    # every element written, with the float32 value of round(x - m) + m
    want = torch.round(case.ins[0] - case.mean) + case.mean
    assert torch.equal(want, case.xhat32)
    assert torch.equal(x_hat.cpu(), want) and torch.equal(_i32(x_hat.cpu()), _i32(want))
    # the decoder's path on the same device tensors
    x, m = case.ins[0].to(dev), case.mean.to(dev)
    sym = torch.full(x.shape, 12345, dtype=torch.int32, device=dev)
    dec = torch.full(x.shape, SENTINEL, device=dev)
    _lib.call("fvc_quantize_symbols", x.data_ptr(), m.data_ptr(), sym.data_ptr(), x.numel(), K.stream_handle())
    _lib.call("fvc_dequantize_symbols", sym.data_ptr(), m.data_ptr(), dec.data_ptr(), x.numel(), K.stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(sym.cpu(), torch.round(case.ins[0] - case.mean).to(torch.int32))
    assert torch.equal(_i32(dec), _i32(x_hat))


# ------------------------------------------------------------------ 3. rpm_scale, lstm_gates
ELEM_SIZES = [1, 255, 257, LAUNCH_N_CAP * K_BLK + 257]  # the last: past launch_n's block cap, the loop strides


def _bound(e_dev, e_cpu, scale, label):
    print(f"{label}: e_dev {e_dev:.3e} e_cpu32 {e_cpu:.3e} scale {scale:.3e}")
    assert e_dev <= 4 * e_cpu + 1e-7 * scale, (label, e_dev, e_cpu, scale)


@gpu
@pytest.mark.parametrize("n", ELEM_SIZES)
def test_rpm_scale(dev, n):
    g = torch.Generator().manual_seed(6000 + n % 1000)
    named = torch.tensor([-50.0, -7 - 1e-6, -7.0, -7 + 1e-6, 0.0, 10.0, 100.0])
    x = torch.randn(n, generator=g) * 5
    i = torch.arange(n)
    sel = i % 16 < 7
    x[sel] = named[i[sel] % 16]
    assert float(named[1]) < -7 < float(named[3])
    cpu = torch.exp(torch.maximum(x, torch.tensor(-7.0))) / 10  # rlvc_ref.rec_prob_model
    ref = torch.exp(torch.maximum(x.double(), torch.tensor(-7.0, dtype=torch.float64))) / 10
    xd = x.to(dev)
    out = torch.full((n,), SENTINEL, device=dev)
    _lib.call("fvc_rpm_scale", xd.data_ptr(), out.data_ptr(), n, K.stream_handle())
    got = out.cpu()
    inf = torch.isinf(cpu)  # exp(100) overflows float32
    assert torch.equal(inf, x == 100.0) and torch.equal(torch.isinf(got), inf)
    assert bool((got[inf] > 0).all())
    fin = ~inf
    if int(fin.sum()):
        rel = lambda t: float(((t[fin].double() - ref[fin]).abs() / ref[fin]).max())
        _bound(rel(got), rel(cpu), 1.0, f"rpm_scale n={n} (relative to each output)")
    # below the clamp the output is exp(-7) / 10 whatever the input
    low = x <= -7
    assert len(torch.unique(got[low])) <= 1


@gpu
@pytest.mark.parametrize("forget_bias", [0.0, 1.0])
@pytest.mark.parametrize("n", ELEM_SIZES)
def test_lstm_gates(dev, n, forget_bias):
    g = torch.Generator().manual_seed(7000 + n % 1000)
    j, i_, f, o, c = (torch.randn(n, generator=g) * 3 for _ in range(5))
    # named rows (j, i, f, o, c_prev): saturated gates, negative j, negative c_prev
    rows = torch.tensor([[2.0, -100.0, 100.0, 100.0, 1.5],     # c = c_prev exactly, h = relu(c) = c
                         [2.0, -100.0, 100.0, 100.0, -1.5],    # c = c_prev < 0, h = 0
                         [3.0, 100.0, -100.0, -100.0, 2.0],    # c = relu(j) exactly, h = 0 * c
                         [-3.0, 100.0, 100.0, 100.0, -0.75],   # relu(j) = 0: c = c_prev < 0, h = 0
                         [-2.0, 0.5, -0.25, 0.75, -4.0],       # ordinary gates, negative j and c_prev
                         [1.0, 0.0, 0.0, 0.0, 0.0]])
    idx = torch.arange(n)
    sel = idx % 16 < 6
    for col, t in enumerate((j, i_, f, o, c)):
        t[sel] = rows[idx[sel] % 16, col]
    c32, h32 = R.lstm_gates(j, i_, f, o, c, forget_bias)
    c64, h64 = R.lstm_gates(j.double(), i_.double(), f.double(), o.double(), c.double(), forget_bias)
    dj, di, df, do, dc = (t.to(dev) for t in (j, i_, f, o, c))
    c_out = torch.full((n,), SENTINEL, device=dev)
    h_out = torch.full((n,), SENTINEL, device=dev)
    _lib.call("fvc_lstm_gates", dj.data_ptr(), di.data_ptr(), df.data_ptr(), do.data_ptr(), dc.data_ptr(),
              c_out.data_ptr(), h_out.data_ptr(), n, forget_bias, K.stream_handle())
    cg, hg = c_out.cpu(), h_out.cpu()
    for name, got, cpu, ref in (("c", cg, c32, c64), ("h", hg, h32, h64)):
        scale = float(ref.abs().max())
        _bound(float((got.double() - ref).abs().max()), float((cpu.double() - ref).abs().max()), scale,
               f"lstm_gates {name} n={n} forget_bias={forget_bias}")
    # c_out is the cell before its relu, h_out = o * relu(c)
    neg = c64 < -1e-3
    assert bool((cg[neg] < 0).all()) and bool((hg[neg] == 0).all())
    # saturated sigmoids are exactly 0 and 1 (exp(100) is inf, 1 + exp(-99) is 1 in float32)
    r = idx % 16
    assert torch.equal(cg[r == 0], c[r == 0]) and torch.equal(hg[r == 0], c[r == 0])
    if n > 1:
        assert torch.equal(cg[r == 1], c[r == 1]) and bool((hg[r == 1] == 0).all())
        assert torch.equal(cg[r == 2], j[r == 2]) and bool((hg[r == 2] == 0).all())
        assert torch.equal(cg[r == 3], c[r == 3]) and bool((hg[r == 3] == 0).all())


# ------------------------------------------------------------------ 4. gdn_cai
def _gdn_inputs(C, npix, seed):
    """|x| from 1e-4 to 1e3; effective beta from 1e-6 (compressai's beta_min: raw 0 clamps to it) to 1;
    effective gamma 0.1 on the diagonal, ~1e-7 off it, one dense row (test_gdn_x3_vs_fp32_and_float64)."""
    g = torch.Generator().manual_seed(seed)
    ped = 2.0 ** -36
    x = 10 ** (torch.rand(1, C, npix, 1, generator=g) * 7 - 4)
    x = x * torch.where(torch.rand(x.shape, generator=g) < 0.5, -1.0, 1.0)
    x.view(-1)[0], x.view(-1)[-1] = 1e-4, 1e3
    beta = 10 ** (torch.rand(C, generator=g, dtype=torch.float64) * 6 - 6)
    gamma = torch.rand(C, C, generator=g, dtype=torch.float64) * 1e-7 + torch.eye(C, dtype=torch.float64) * 0.1
    gamma[5, :] = torch.rand(C, generator=g, dtype=torch.float64) * 0.02
    raw_b = torch.sqrt(beta + ped).float()
    raw_b[::7] = 0.0
    return x, {"t.beta": raw_b, "t.gamma": torch.sqrt(gamma + ped).float()}


@gpu
@pytest.mark.parametrize("npix", [1, K_GC_PIX - 1, K_GC_PIX, K_GC_PIX + 1, K_GC_PIX * LAUNCH_N_CAP + 3])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("C", [64, 128])
def test_gdn_cai(dev, C, inverse, npix):
    x, sd = _gdn_inputs(C, npix, 8000 + C + npix % 1000 + int(inverse))
    cpu = R.gdn_cai(sd, "t", x, inverse)
    ref = R.gdn_cai(_dbl(sd), "t", x.double(), inverse)
    p = _GDNP(C, inverse)
    p.load_state_dict({"beta": sd["t.beta"], "gamma": sd["t.gamma"]})
    p.invalidate()
    beta, gamma = (t.to(dev) for t in p.effective())
    assert abs(float(beta.min()) - 1e-6) < 1e-9
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)  # [1, npix, 1, C]
    y = torch.full(xd.shape, SENTINEL, device=dev)
    _lib.call("fvc_gdn_nhwc_cai", xd.data_ptr(), y.data_ptr(), beta.data_ptr(), gamma.data_ptr(), 1, npix, 1, C,
              int(inverse), K.stream_handle())
    got = y.cpu().permute(0, 3, 1, 2).double()
    scale = float(ref.abs().max())
    _bound(float((got - ref).abs().max()), float((cpu.double() - ref).abs().max()), scale,
           f"gdn_cai C={C} inverse={inverse} npix={npix}")
    # the same bound relative to each output: the small activations count as much as the large
    rel = lambda t: float(((t - ref).abs() / ref.abs()).max())
    _bound(rel(got), rel(cpu.double()), 1.0, f"gdn_cai C={C} inverse={inverse} npix={npix} (relative to each output)")


@gpu
def test_gdn_cai_rejects_other_channel_counts(dev):
    x = torch.ones(1, 2, 2, 96, device=dev)
    y = torch.full(x.shape, SENTINEL, device=dev)
    beta, gamma = torch.ones(96, device=dev), torch.eye(96, device=dev)
    rc = _lib.load().fvc_gdn_nhwc_cai(x.data_ptr(), y.data_ptr(), beta.data_ptr(), gamma.data_ptr(), 1, 2, 2, 96, 0,
                                      K.stream_handle())
    torch.cuda.synchronize()
    assert rc == FVC_EINVAL
    assert bool((y == SENTINEL).all())
