// Second half of a cout <= 4 conv / transposed conv computed as a tap-partial GEMM (the x3
// kernel's 1x1 pass writes P[b][iy][ix][t * cout + co] = sum_ci x[b][iy][ix][ci] w_t[ci][co] for
// every input pixel and tap t = ky * ks + kx): y[b][Y][X][co] = bias[co] + sum over the taps that
// reach (Y, X) of P at the source pixel, then activation, residual, exp; pad channel 3 (and any
// co >= cout) = 0. Conv (stride 1): source = (Y + ky - pad, X + kx - pad); transposed (stride s,
// output padding s - 1): source = ((Y + pad - ky) / s, (X + pad - kx) / s) where divisible.
// Fixed tap order: deterministic. HBM-bound (P is re-read from L1/L2 by neighbouring outputs).
#include "fvc_common.h"
#include "fvc_split.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlk = 256;

// Output pixel e from its bias + tap sums: activation, residual (4 floats per pixel), exp, and one
// 16-B store with the channels past COUT zero.
template <int COUT>
__device__ __forceinline__ void gather_finish(const float (&acc)[COUT], const float* res, float* y, size_t e,
                                              float act_slope, int post_op) {
  float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (res) rv = reinterpret_cast<const float4*>(res)[e];
  const float rr[4] = {rv.x, rv.y, rv.z, rv.w};
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  float* ov = &o.x;
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    float v = acc[co];
    v = fmaxf(v, v * act_slope);
    if (res) v += rr[co];
    if (post_op == FVC_POST_EXP) v = expf(v);
    ov[co] = v;
  }
  reinterpret_cast<float4*>(y)[e] = o;
}

// The generic form, straight from HBM: any layer the LDS forms below do not take.
template <int KS, int COUT, int TR>
__global__ __launch_bounds__(256) void k_tap_gather(const float* __restrict__ P, int pcp,
                                                    const float* __restrict__ bias,
                                                    const float* __restrict__ res, float* __restrict__ y,
                                                    int B, int H, int W, int Ho, int Wo, float act_slope,
                                                    int post_op) {
  constexpr int pad = KS / 2;
  const size_t n = (size_t)B * Ho * Wo;
  for (size_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const int X = e % Wo;
    const int Y = (e / Wo) % Ho;
    const size_t b = e / ((size_t)Wo * Ho);
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = bias[co];
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
      // transposed (stride 2): only taps with ky = Y + pad (mod 2) reach row Y
      if (TR && ((Y + pad - ky) & 1)) continue;
      const int iy = TR ? (Y + pad - ky) >> 1 : Y + ky - pad;  // >> 1: floor for negatives
      if (iy < 0 || iy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) {
        if (TR && ((X + pad - kx) & 1)) continue;
        const int ix = TR ? (X + pad - kx) >> 1 : X + kx - pad;
        if (ix < 0 || ix >= W) continue;
        const float* src = P + ((b * H + iy) * W + ix) * pcp + (ky * KS + kx) * COUT;
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[co] += src[co];
      }
    }
    gather_finish<COUT>(acc, res, y, e, act_slope, post_op);
  }
}

// Stage an IR x IC pixel window of P (c4n float4 per pixel, origin (r0, c0), zeros outside the
// image) into LDS at pixel stride ps: eight loads per thread in flight per batch, every address
// clamped into the image and out-of-image values selected to zero after the load (a per-element
// branch made each load wait for the previous one's LDS write: one HBM round trip per element)
__device__ __forceinline__ void stage_p_window(const float* __restrict__ Pb, int pcp, int H, int W, int r0, int c0,
                                               int IR, int IC, int ps, float* sp) {
  constexpr int NB = 8;
  const int c4n = pcp >> 2;
  const int total = IR * IC * c4n;
  for (int e0 = threadIdx.x; e0 < total; e0 += NB * blockDim.x) {
    float4 v[NB];
    int dst[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const int e = e0 + k * blockDim.x;
      const int ee = e < total ? e : total - 1;
      const int c4 = ee % c4n, p = ee / c4n;
      const int iy = r0 + p / IC, ix = c0 + p % IC;
      const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
      const float4 t = *reinterpret_cast<const float4*>(Pb + ((size_t)cy * W + cx) * pcp + 4 * c4);
      v[k] = ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
      dst[k] = e < total ? p * ps + 4 * c4 : -1;
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      if (dst[k] >= 0) {
        float* d = sp + dst[k];
        d[0] = v[k].x; d[1] = v[k].y; d[2] = v[k].z; d[3] = v[k].w;
      }
    }
  }
}

// Output rows per block of the LDS tap gathers below (x 32 columns).
constexpr int kGatherTH = 8;

// Stride-1 3x3 tap gather through LDS (the second half of the fused producer + tap path): a block
// stages the P tile of its 8 x 32 outputs plus a 1-pixel halo with coalesced 16-B loads (zeros
// outside the image), pixel stride pcp + 1 words so the per-tap reads of consecutive outputs hit
// distinct banks, then sums bias + taps in k_tap_gather's order (an out-of-image tap adds +0).
template <int COUT>
__global__ __launch_bounds__(256) void k_tap_gather3_lds(const float* __restrict__ P, int pcp,
                                                         const float* __restrict__ bias,
                                                         const float* __restrict__ res, float* __restrict__ y,
                                                         int H, int W, float act_slope, int post_op) {
  constexpr int TH = kGatherTH, TW = 32, IR = TH + 2, IC = TW + 2;
  extern __shared__ float sp[];
  const int ps = pcp + 1;
  const size_t b = blockIdx.z;
  const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  const float* Pb = P + b * H * W * pcp;
  stage_p_window(Pb, pcp, H, W, y0 - 1, x0 - 1, IR, IC, ps, sp);
  __syncthreads();
  for (int q = threadIdx.x; q < TH * TW; q += blockDim.x) {
    const int r = q / TW, c = q % TW;
    const int Y = y0 + r, X = x0 + c;
    if (Y >= H || X >= W) continue;
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = bias[co];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float* src = sp + ((r + ky) * IC + c + kx) * ps + (ky * 3 + kx) * COUT;
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[co] += src[co];
      }
    gather_finish<COUT>(acc, res, y, (b * H + Y) * W + X, act_slope, post_op);
  }
}

// Transposed (stride 2, output padding 1) tap gather through LDS: a block's 8 x 32 outputs read
// input rows Y0/2 - 1 .. Y0/2 + 4 and columns X0/2 - 1 .. X0/2 + 17 of P (k = 3 or 5), staged
// once with coalesced 16-B loads; per output the same tap order as k_tap_gather.
template <int KS, int COUT>
__global__ __launch_bounds__(256) void k_tap_gather_t2_lds(const float* __restrict__ P, int pcp,
                                                           const float* __restrict__ bias,
                                                           const float* __restrict__ res, float* __restrict__ y,
                                                           int H, int W, float act_slope, int post_op) {
  // output rows Y0 .. Y0 + TH - 1 read input rows Y0/2 - 1 .. Y0/2 + TH/2 (k <= 5)
  constexpr int TH = kGatherTH, TW = 32, IR = TH / 2 + 2, IC = 19, pad = KS / 2;
  extern __shared__ float sp[];
  const int ps = pcp + 1;
  const int Ho = 2 * H, Wo = 2 * W;
  const size_t b = blockIdx.z;
  const int Y0 = blockIdx.y * TH, X0 = blockIdx.x * TW;
  const int r0 = Y0 / 2 - 1, c0 = X0 / 2 - 1;
  const float* Pb = P + b * H * W * pcp;
  stage_p_window(Pb, pcp, H, W, r0, c0, IR, IC, ps, sp);
  __syncthreads();
  for (int q = threadIdx.x; q < TH * TW; q += blockDim.x) {
    const int Y = Y0 + q / TW, X = X0 + q % TW;
    if (Y >= Ho || X >= Wo) continue;
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = bias[co];
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
      if ((Y + pad - ky) & 1) continue;
      const int lr = ((Y + pad - ky) >> 1) - r0;  // in [0, IR): out-of-image rows hold zeros
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) {
        if ((X + pad - kx) & 1) continue;
        const int lc = ((X + pad - kx) >> 1) - c0;
        const float* src = sp + (lr * IC + lc) * ps + (ky * KS + kx) * COUT;
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[co] += src[co];
      }
    }
    gather_finish<COUT>(acc, res, y, (b * Ho + Y) * Wo + X, act_slope, post_op);
  }
}

}  // namespace

extern "C" int fvc_tap_gather_nhwc(const float* P, int pcp, const float* bias, const float* res, float* y, int batch,
                                   int h, int w, int cout, int ksize, int stride, int transposed, int act,
                                   int post_op, fvc_stream_t s) {
  if (!P || !bias || !y || batch <= 0 || h <= 0 || w <= 0 || cout < 1 || cout > 4 ||
      (ksize != 3 && ksize != 5) || pcp < ksize * ksize * cout || pcp % 4)
    return FVC_EINVAL;
  if (transposed ? stride != 2 : stride != 1) return FVC_EINVAL;
  const int Ho = transposed ? h * stride : h, Wo = transposed ? w * stride : w;
  const float slope = fvc_act_slope(act);
  hipStream_t st = (hipStream_t)s;
  if (!transposed && ksize == 3 && pcp <= 32) {
    // 8-row tiles: 39 KB of LDS at pcp 28, four blocks per CU
    const dim3 gt(fvc_cdiv(w, 32), fvc_cdiv(h, kGatherTH), batch);
    const size_t lds = (size_t)(kGatherTH + 2) * 34 * (pcp + 1) * 4;
#define FVC_TGL(CO)                                                                                            \
    if (cout == CO) {                                                                                         \
      return fvc_launch(k_tap_gather3_lds<CO>, gt, dim3(256), lds, st, P, pcp, bias, res, y, h, w, slope, post_op); \
    }
    FVC_TGL(1) FVC_TGL(2) FVC_TGL(3) FVC_TGL(4)
#undef FVC_TGL
  }
  if (transposed && pcp <= 128) {
    // 8-row output tiles (6 x 19 input pixels in LDS: ~35 KB at pcp 76, four blocks per CU)
    const dim3 gt(fvc_cdiv(Wo, 32), fvc_cdiv(Ho, kGatherTH), batch);
    const size_t lds = (size_t)(kGatherTH / 2 + 2) * 19 * (pcp + 1) * 4;
#define FVC_TGT(KS, CO)                                                                                        \
    if (ksize == KS && cout == CO) {                                                                          \
      return fvc_launch(k_tap_gather_t2_lds<KS, CO>, gt, dim3(256), lds, st, P, pcp, bias, res, y, h, w, slope, \
                        post_op);                                                                             \
    }
    FVC_TGT(3, 1) FVC_TGT(3, 2) FVC_TGT(3, 3) FVC_TGT(3, 4)
    FVC_TGT(5, 1) FVC_TGT(5, 2) FVC_TGT(5, 3) FVC_TGT(5, 4)
#undef FVC_TGT
  }
  const dim3 g(fvc_blocks((size_t)batch * Ho * Wo, kBlk, 8192));
#define FVC_TG(KS, CO, TR)                                                                                      \
  if (ksize == KS && cout == CO && transposed == TR)                                                            \
    return fvc_launch(k_tap_gather<KS, CO, TR>, g, dim3(kBlk), 0, st, P, pcp, bias, res, y, batch, h, w, Ho, Wo, slope, \
                      post_op);
  FVC_TG(3, 1, 0) FVC_TG(3, 2, 0) FVC_TG(3, 3, 0) FVC_TG(3, 4, 0)
  FVC_TG(5, 1, 0) FVC_TG(5, 2, 0) FVC_TG(5, 3, 0) FVC_TG(5, 4, 0)
  FVC_TG(3, 1, 1) FVC_TG(3, 2, 1) FVC_TG(3, 3, 1) FVC_TG(3, 4, 1)
  FVC_TG(5, 1, 1) FVC_TG(5, 2, 1) FVC_TG(5, 3, 1) FVC_TG(5, 4, 1)
#undef FVC_TG
  return FVC_EINVAL;
}
