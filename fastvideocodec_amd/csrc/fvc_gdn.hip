// GDN / IGDN: norm_i = beta_i + sum_j gamma[i][j] x_j^2 ; y = x / sqrt(norm) (or x * sqrt(norm)).
// Three matrix-core forms for C = 64 (split-precision fp16, the default; fp32 MFMA, which
// FVC_GDN_X3=0 selects; each also with the next layer's tap-partial GEMM fused) and the RLVC
// path's VALU form for any C.
//
// Contraction is off: the kernels write fmaf where they want a fused multiply-add and rely on
// separately rounded products and sums everywhere else.
#include "fvc_common.h"
#include "fvc_split.h"

#pragma clang fp contract(off)

namespace {

using fvc_split::h8;

// ------------------------------------------------------------------ GDN / IGDN (C = 64)
// GDN / IGDN on the fp32 matrix cores. norm = conv1x1(x^2, gamma) + beta is a [32 px x 64] x
// [64 x 64] product per 32-pixel group: 2 N-tiles x 32 v_mfma_f32_32x32x2_f32 (an exact fp32 FMA
// chain per output). gamma^T fragments stay in 64 VGPRs for the whole kernel. Lane (p, h) loads
// channels [32h, 32h+32) of pixel p (its A operand for all 32 MFMAs: MFMA s pairs channel s with
// s+32), parks them in a per-wave LDS tile, and reads x back in the accumulator layout (lane =
// channel, register = pixel) for the normalisation, so HBM sees x once and y once.
constexpr int kGdnWaves = 4;
constexpr int kGdnRow = 68;  // LDS row stride in floats (272 B = 16 x odd: conflict-free b128 writes)

// What the two fp32-MFMA kernels share. Accumulator layout: lane (li, lh), register r -> pixel
// q = (r&3) + 8(r>>2) + 4lh, channel li (+32).
struct GdnF32 {
  float g0[32], g1[32];  // gamma^T[k = s + 32 lh][n = li (+32)] = gamma[n][k]
  float4 nx[8];          // the next group's x, loaded while the current group's MFMAs run
};

__device__ __forceinline__ void gdn_f32_gamma(GdnF32& w, const float* gamma, int li, int lh) {
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    w.g0[s] = gamma[li * 64 + s + 32 * lh];
    w.g1[s] = gamma[(32 + li) * 64 + s + 32 * lh];
  }
}

__device__ __forceinline__ void gdn_f32_fetch(GdnF32& w, const float* x, size_t gi, size_t npix, int li, int lh) {
  const size_t p = gi * 32 + li;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    w.nx[k] = p < npix ? reinterpret_cast<const float4*>(x + p * 64 + 32 * lh)[k] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Parks the fetched group in the wave's LDS tile xw, starts the next group's loads (if any) and
// forms the two accumulator tiles of gamma . x^2.
__device__ __forceinline__ void gdn_f32_norm(GdnF32& w, const float* x, float* xw, size_t gnext, size_t ngroups,
                                             size_t npix, int li, int lh, f32x16& acc0, f32x16& acc1) {
  float a[32];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 v = w.nx[k];
    a[4 * k] = v.x; a[4 * k + 1] = v.y; a[4 * k + 2] = v.z; a[4 * k + 3] = v.w;
    *reinterpret_cast<float4*>(xw + li * kGdnRow + 32 * lh + 4 * k) = v;
  }
  if (gnext < ngroups) gdn_f32_fetch(w, x, gnext, npix, li, lh);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc0[r] = 0.f;
    acc1[r] = 0.f;
  }
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    const float sq = a[s] * a[s];
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sq, w.g0[s], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(sq, w.g1[s], acc1, 0, 0, 0);
  }
}

__global__ __launch_bounds__(64 * kGdnWaves) void k_gdn_mfma(const float* __restrict__ x, float* __restrict__ y,
                                                          const float* __restrict__ beta,
                                                          const float* __restrict__ gamma, size_t npix,
                                                          int inverse) {
  __shared__ float xt[kGdnWaves * 32 * kGdnRow];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  GdnF32 w;
  gdn_f32_gamma(w, gamma, li, lh);
  const float b0 = beta[li], b1 = beta[32 + li];
  float* xw = xt + wave * 32 * kGdnRow;
  const size_t ngroups = (npix + 31) / 32;
  const size_t gstep = (size_t)gridDim.x * kGdnWaves;
  size_t gi = (size_t)blockIdx.x * kGdnWaves + wave;
  if (gi < ngroups) gdn_f32_fetch(w, x, gi, npix, li, lh);
  for (; gi < ngroups; gi += gstep) {
    const size_t p0 = gi * 32;
    f32x16 acc0, acc1;
    gdn_f32_norm(w, x, xw, gi + gstep, ngroups, npix, li, lh, acc0, acc1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (p0 + q < npix) {
        const float x0 = xw[q * kGdnRow + li], x1 = xw[q * kGdnRow + 32 + li];
        const float n0 = sqrtf(acc0[r] + b0), n1 = sqrtf(acc1[r] + b1);
        float* yo = y + (p0 + q) * 64;
        yo[li] = inverse ? x0 * n0 : x0 / n0;
        yo[32 + li] = inverse ? x1 * n1 : x1 / n1;
      }
    }
  }
}

// GDN / IGDN followed by the next layer's 1x1 tap-partial GEMM (resDecoder igdn3 -> deconv4,
// synthesis.py:26,57: 64 -> 3, 5x5 s2, 75 partials): per 32-pixel group the normalised y goes back
// into the wave's LDS tile (pixel-major), each lane then reads its pixel's channels as split-
// precision B fragments (channel order of fvc_x3_tap_pack_weight) and NPT P tiles of 32 partials
// come out of three fp16 MFMAs per k16 block, P = main * 2^-kt + corr * 2^-kt-11. y itself never
// reaches HBM; fvc_tap_gather_nhwc sums the partials into the deconv's output.
template <int NPT>
__global__ __launch_bounds__(64 * kGdnWaves) void k_gdn_tap_mfma(const float* __restrict__ x, float* __restrict__ P,
                                                             const float* __restrict__ beta,
                                                             const float* __restrict__ gamma,
                                                             const uint4* __restrict__ tw, float4 tosc,
                                                             size_t npix, int inverse, int pcp, int* ovf) {
  __shared__ float xt[kGdnWaves * 32 * kGdnRow];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  GdnF32 w;
  gdn_f32_gamma(w, gamma, li, lh);
  const float b0 = beta[li], b1 = beta[32 + li];
  const float ts[4] = {tosc.x, tosc.y, tosc.z, tosc.w};
  float* xw = xt + wave * 32 * kGdnRow;
  const size_t ngroups = (npix + 31) / 32;
  const size_t gstep = (size_t)gridDim.x * kGdnWaves;
  size_t gi = (size_t)blockIdx.x * kGdnWaves + wave;
  float mx = 0.f;
  if (gi < ngroups) gdn_f32_fetch(w, x, gi, npix, li, lh);
  for (; gi < ngroups; gi += gstep) {
    const size_t p0 = gi * 32;
    f32x16 acc0, acc1;
    gdn_f32_norm(w, x, xw, gi + gstep, ngroups, npix, li, lh, acc0, acc1);
    // y (the same expression as k_gdn_mfma) back into the tile; pixels past npix hold 0
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = (r & 3) + 8 * (r >> 2) + 4 * lh;
      const bool ok = p0 + q < npix;
      const float x0 = xw[q * kGdnRow + li], x1 = xw[q * kGdnRow + 32 + li];
      const float n0 = sqrtf(acc0[r] + b0), n1 = sqrtf(acc1[r] + b1);
      const float y0 = inverse ? x0 * n0 : x0 / n0, y1 = inverse ? x1 * n1 : x1 / n1;
      xw[q * kGdnRow + li] = ok ? y0 : 0.f;
      xw[q * kGdnRow + 32 + li] = ok ? y1 : 0.f;
    }
    // lane (li, lh): pixel li's channels 16 kb + 4 lh + {0-3, 8-11} as hi / lo*2^11 halves
    h8 yh[4], yl[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const float* row = xw + li * kGdnRow + 16 * kb + 4 * lh;
      const float4 u = *reinterpret_cast<const float4*>(row), v = *reinterpret_cast<const float4*>(row + 8);
      const float f[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const _Float16 h = (_Float16)f[t];
        yh[kb][t] = h;
        yl[kb][t] = (_Float16)((f[t] - (float)h) * 2048.f);
        mx = fmaxf(mx, fabsf(f[t]));
      }
    }
    const bool px_ok = p0 + li < npix;
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
      f32x16 pa, pc;
#pragma unroll
      for (int r = 0; r < 16; ++r) pa[r] = pc[r] = 0.f;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const uint4* f = tw + (size_t)((pt * 4 + kb) * 2) * 64 + lane;
        const h8 wh = __builtin_bit_cast(h8, f[0]), wl = __builtin_bit_cast(h8, f[64]);
        pa = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, yh[kb], pa, 0, 0, 0);
        pc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, yh[kb], pc, 0, 0, 0);
        pc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, yl[kb], pc, 0, 0, 0);
      }
      const float sc = ts[pt], scc = ts[pt] * (1.0f / 2048.f);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int pp = pt * 32 + 8 * g + 4 * lh;
        if (px_ok && pp < pcp) {
          float o[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = fmaf(pc[4 * g + i], scc, pa[4 * g + i] * sc);
          *reinterpret_cast<float4*>(P + (p0 + li) * pcp + pp) = make_float4(o[0], o[1], o[2], o[3]);
        }
      }
    }
  }
  if (!(mx < 65000.f) && ovf) atomicOr(ovf, 1);
}

// GDN / IGDN with the norm on the split-precision fp16 matrix cores (the conv kernels' scheme):
// norm = beta + gamma . x^2 is a [64 out ch] x [64 in ch] x [32 px] GEMM per 32-pixel group with
// gamma as the row operand (one launch-wide scale 2^kw: max |gamma| * 2^kw in [2^13, 2^14)) and
// x^2 * 2^-8 as the column operand, both split exactly into fp16 hi + lo * 2^-11:
// 2 N-tiles x 4 k-blocks x 3 v_mfma_f32_32x32x16_f16 (24 MFMAs of 8 passes) instead of 64
// v_mfma_f32_32x32x2_f32 of 16 passes -- the fp32 form's matrix time is as long as its HBM time.
// Lane (li, lh) owns pixel li and channels 32t + 8g + 4lh + {0..3} (t = 0..1, g = 0..3) from load
// to store: k-block kb = 2t + gp orders its channels {16gp + 4lh + 0-3 | 16gp + 8 + 4lh + 0-3}
// (+32t), so a lane's column operand is its own x / accumulator registers 8gp .. 8gp + 7 and no
// LDS tile is needed (the same order as fvc_x3_tap_pack_weight: in the tap form (NPT > 0) the
// normalised y already is the B fragment of the tap GEMM). The omitted lo * lo term and the lo
// roundings are ~2^-22 relative per product; every term of the norm is >= 0, so the norm carries
// that relative error (fp32 chain: ~2^-24 per add). The column operand carries a power-of-two
// scale per pixel, x^2 * 2^e with the pixel's max x^2 * 2^e in [2^14, 2^15) (e clamped to
// [-60, 60]), undone per lane in the epilogue (the accumulator column of a lane is its own pixel):
// small activations stay in the fp16 normal range, so the ~2^-22 relative bound holds for every
// pixel whose max |x| is above ~1e-11, whatever beta is. A group with an inf or NaN x^2 runs the
// fp32 MFMA chain instead (wave-uniform branch, gamma read from L2).
template <int NPT, bool INV>
__global__ __launch_bounds__(256, 2) void k_gdn_x3(const float* __restrict__ x, float* __restrict__ out,
                                                   const float* __restrict__ beta, const float* __restrict__ gamma,
                                                   const uint4* __restrict__ tw, float4 tosc, size_t npix,
                                                   int pcp, int* ovf) {
  __shared__ float4 sbeta[16];
  __shared__ uint4 sg[2 * 4 * 2 * 64];  // row-operand fragments [n][kb][hi, lo][lane]
  __shared__ uint4 stw[NPT > 0 ? NPT * 512 : 1];  // the tap pack (fvc_x3_tap_pack_weight layout)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  if (threadIdx.x < 64) reinterpret_cast<float*>(sbeta)[threadIdx.x] = beta[threadIdx.x];
  if constexpr (NPT > 0)
    for (int i = threadIdx.x; i < NPT * 512; i += 256) stw[i] = tw[i];
  // row operand: lane (li, lh) -> out channel 32n + li, k-block kb's 8 channels of half lh; every
  // wave reads all 4096 entries (the same scale in every wave of the launch), wave 0 stores them
  float gv[2][4][8];
  float gmax = 0.f;
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int ch = 32 * (kb >> 1) + 16 * (kb & 1) + 4 * lh + (e < 4 ? e : 4 + e);
        gv[n][kb][e] = gamma[(32 * n + li) * 64 + ch];
        gmax = fmaxf(gmax, fabsf(gv[n][kb][e]));
      }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, o, 64));
  int ge = 0;
  (void)frexpf(gmax, &ge);
  const int kw = gmax > 0.f ? max(-60, min(60, 14 - ge)) : 0;
  if (wave == 0) {
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        h8 gh, gl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float s = ldexpf(gv[n][kb][e], kw);
          const _Float16 h = (_Float16)s;
          gh[e] = h;
          gl[e] = (_Float16)((s - (float)h) * 2048.f);
        }
        sg[((n * 4 + kb) * 2) * 64 + lane] = __builtin_bit_cast(uint4, gh);
        sg[((n * 4 + kb) * 2 + 1) * 64 + lane] = __builtin_bit_cast(uint4, gl);
      }
  }
  const float ts[4] = {tosc.x, tosc.y, tosc.z, tosc.w};
  __syncthreads();
  const size_t ngroups = (npix + 31) / 32;
  float4 nx[8];  // nx[2 kb + h]: channels 32t + 16gp + 8h + 4lh + 0..3
  auto fetch = [&](size_t gi) {
    const size_t p = gi * 32 + li;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      nx[k] = p < npix ? *reinterpret_cast<const float4*>(x + p * 64 + 16 * (k >> 1) + 8 * (k & 1) + 4 * lh)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  const size_t gstep = (size_t)gridDim.x * 4;
  size_t gi = (size_t)blockIdx.x * 4 + wave;
  float mx = 0.f;
  if (gi < ngroups) fetch(gi);
  for (; gi < ngroups; gi += gstep) {
    // keeps the loop-invariant fragment reads from LDS inside the loop (hoisted, they would take
    // 64 registers and spill)
    asm volatile("" ::: "memory");
    const size_t p = gi * 32 + li;
    // xr[t][r]: channel 32t + 8(r / 4) + 4lh + r % 4 (the accumulator layout)
    float xr[2][16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int t = k >> 2, r0 = 4 * (k & 3);
      xr[t][r0] = nx[k].x; xr[t][r0 + 1] = nx[k].y; xr[t][r0 + 2] = nx[k].z; xr[t][r0 + 3] = nx[k].w;
    }
    if (gi + gstep < ngroups) fetch(gi + gstep);
    // this pixel's scale: max |x| over its 64 channels (this lane's 32 and lane li + 32's)
    float ax = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) ax = fmaxf(ax, fabsf(xr[t][r]));
    ax = fmaxf(ax, __shfl_xor(ax, 32, 64));
    int pe = 0;
    (void)frexpf(ax * ax, &pe);
    const int es = ax > 0.f ? max(-60, min(60, 15 - pe)) : 0;  // max x^2 2^es in [2^14, 2^15)
    const float xsc = ldexpf(1.f, es);
    const float sc = ldexpf(1.f, -es - kw), scc = ldexpf(1.f, -es - kw - 11);
    h8 sh[4], sl[4];
    bool big = false;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = xr[kb >> 1][8 * (kb & 1) + e];
        const float s = (v * v) * xsc;
        big |= !(s < 65000.f);
        const _Float16 h = (_Float16)s;
        sh[kb][e] = h;
        sl[kb][e] = (_Float16)((s - (float)h) * 2048.f);
      }
    // per N-tile: norm (x3 MFMAs, or the fp32 chain for a group out of fp16 range), then
    // y = x / sqrt(norm) (GDN) or x * sqrt(norm) (IGDN), norm = sum + beta, written over x (tile 0's
    // y is parked until tile 1's fp32 chain has read x)
    const bool slow = __any(big);
    float y0[16];
    const float s1 = slow ? 1.f : sc, s2 = slow ? 0.f : scc;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      f32x16 a, c;
#pragma unroll
      for (int r = 0; r < 16; ++r) a[r] = c[r] = 0.f;
      if (!slow) {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
          const h8 wh = __builtin_bit_cast(h8, sg[((n * 4 + kb) * 2) * 64 + lane]);
          const h8 wl = __builtin_bit_cast(h8, sg[((n * 4 + kb) * 2 + 1) * 64 + lane]);
          a = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, sh[kb], a, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, sh[kb], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, sl[kb], c, 0, 0, 0);
        }
      } else {
        // v_mfma_f32_32x32x2_f32, k = (register s of the lane, half lh)
#pragma unroll
        for (int s = 0; s < 32; ++s) {
          const int t = s >> 4, r = s & 15;
          const int ch = 32 * t + 8 * (r >> 2) + 4 * lh + (r & 3);
          const float v = xr[t][r];
          a = __builtin_amdgcn_mfma_f32_32x32x2f32(gamma[(32 * n + li) * 64 + ch], v * v, a, 0, 0, 0);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 b = sbeta[8 * n + 2 * g + lh];
        const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float nv = sqrtf(fmaf(c[4 * g + i], s2, a[4 * g + i] * s1) + bb[i]);
          const float xv = xr[n][4 * g + i];
          const float yv = INV ? xv * nv : xv / nv;
          if (n == 0) y0[4 * g + i] = yv;
          else xr[1][4 * g + i] = yv;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) xr[0][r] = y0[r];
    float (&yr)[2][16] = xr;
    if constexpr (NPT == 0) {
      if (p < npix) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(out + p * 64 + 32 * t + 8 * g + 4 * lh) =
                make_float4(yr[t][4 * g], yr[t][4 * g + 1], yr[t][4 * g + 2], yr[t][4 * g + 3]);
      }
    } else {
      // the tap GEMM: y registers 8gp .. 8gp + 7 of tile t are the k16 block kb = 2t + gp
      const bool px_ok = p < npix;
      h8 yh[4], yl[4];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = px_ok ? yr[kb >> 1][8 * (kb & 1) + e] : 0.f;
          const _Float16 h = (_Float16)f;
          yh[kb][e] = h;
          yl[kb][e] = (_Float16)((f - (float)h) * 2048.f);
          mx = fmaxf(mx, fabsf(f));
        }
      // the same GEMM and store as k_gdn_tap_mfma's, the pack read from LDS (written out in both:
      // a shared function changes this kernel's register allocation)
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
        f32x16 pa, pc;
#pragma unroll
        for (int r = 0; r < 16; ++r) pa[r] = pc[r] = 0.f;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
          const uint4* f = stw + ((pt * 4 + kb) * 2) * 64 + lane;
          const h8 wh = __builtin_bit_cast(h8, f[0]), wl = __builtin_bit_cast(h8, f[64]);
          pa = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, yh[kb], pa, 0, 0, 0);
          pc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, yh[kb], pc, 0, 0, 0);
          pc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, yl[kb], pc, 0, 0, 0);
        }
        const float sc = ts[pt], scc = ts[pt] * (1.0f / 2048.f);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int pp = pt * 32 + 8 * g + 4 * lh;
          if (px_ok && pp < pcp) {
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = fmaf(pc[4 * g + i], scc, pa[4 * g + i] * sc);
            *reinterpret_cast<float4*>(out + p * pcp + pp) = make_float4(o[0], o[1], o[2], o[3]);
          }
        }
      }
    }
  }
  if (NPT > 0 && !(mx < 65000.f) && ovf) atomicOr(ovf, 1);
}

// ------------------------------------------------------------------ RLVC path
// compressai.layers.GDN (models.py:23,529-538): norm = conv1x1(x^2, gamma) + beta,
// y = x * rsqrt(norm) (GDN) or x * sqrt(norm) (IGDN), any C (RLVC: 128). A block of C threads
// walks pixels in groups of kGcPix: the group's x rows go to LDS, thread i keeps row i of gamma
// in registers and sums gamma[i][j] x_j^2 over the LDS rows (broadcast reads).
constexpr int kGcPix = 8;

template <int C>
__global__ __launch_bounds__(C) void k_gdn_cai(const float* __restrict__ x, float* __restrict__ y,
                                               const float* __restrict__ beta, const float* __restrict__ gamma,
                                               size_t npix, int inverse) {
  __shared__ float xs[kGcPix][C];
  const int i = threadIdx.x;
  float g[C];
#pragma unroll
  for (int j = 0; j < C; ++j) g[j] = gamma[(size_t)i * C + j];
  const float b = beta[i];
  for (size_t p0 = (size_t)blockIdx.x * kGcPix; p0 < npix; p0 += (size_t)gridDim.x * kGcPix) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kGcPix; ++q) xs[q][i] = p0 + q < npix ? x[(p0 + q) * C + i] : 0.f;
    __syncthreads();
    float acc[kGcPix];
#pragma unroll
    for (int q = 0; q < kGcPix; ++q) acc[q] = 0.f;
#pragma unroll 8
    for (int j = 0; j < C; ++j) {
#pragma unroll
      for (int q = 0; q < kGcPix; ++q) {
        const float v = xs[q][j];
        acc[q] = fmaf(g[j], v * v, acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < kGcPix; ++q) {
      if (p0 + q >= npix) break;
      const float norm = acc[q] + b;
      const float xv = xs[q][i];
      y[(p0 + q) * C + i] = inverse ? xv * sqrtf(norm) : xv * (1.f / sqrtf(norm));
    }
  }
}

// blocks of the fp32-MFMA kernels: kGdnWaves groups of 32 pixels per block and pass
unsigned gdn_f32_blocks(size_t npix) { return fvc_blocks(npix, 32 * kGdnWaves, 2048); }

// persistent grid of the split-precision GDN kernels: 4 groups of 32 pixels per block and pass
unsigned gdn_x3_blocks(size_t npix) {
  static const int cap = fvc_env_int("FVC_GDN_BLOCKS", 1024);
  return fvc_blocks(npix, 32 * 4, (size_t)cap);
}

}  // namespace

extern "C" {

int fvc_gdn_nhwc(const float* x, float* y, const float* beta, const float* gamma, int batch, int h, int w, int c,
                 int inverse, fvc_stream_t s) {
  if (!x || !y || !beta || !gamma || c != 64) return FVC_EINVAL;
  const size_t npix = (size_t)batch * h * w;
  hipStream_t st = (hipStream_t)s;
  if (fvc_env_int("FVC_GDN_X3", 1)) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const dim3 g(gdn_x3_blocks(npix));
    if (inverse)
      return fvc_launch(k_gdn_x3<0, true>, g, dim3(256), 0, st, x, y, beta, gamma, (const uint4*)nullptr, z4, npix, 0,
                        (int*)nullptr);
    return fvc_launch(k_gdn_x3<0, false>, g, dim3(256), 0, st, x, y, beta, gamma, (const uint4*)nullptr, z4, npix, 0,
                      (int*)nullptr);
  }
  return fvc_launch(k_gdn_mfma, dim3(gdn_f32_blocks(npix)), dim3(64 * kGdnWaves), 0, st, x, y, beta, gamma, npix,
                    inverse);
}

int fvc_gdn_tap_nhwc(const float* x, float* P, const float* beta, const float* gamma, const void* tap_wpack,
                     const float* tap_osc, int ntiles, int pcp, int batch, int h, int w, int c, int inverse,
                     int* overflow_flag, fvc_stream_t s) {
  if (!x || !P || !beta || !gamma || !tap_wpack || !tap_osc || c != 64 || ntiles < 1 || ntiles > 4 || pcp <= 0 ||
      pcp % 4 || pcp > 32 * ntiles)
    return FVC_EINVAL;
  const size_t npix = (size_t)batch * h * w;
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < ntiles; ++i) t[i] = tap_osc[i];
  const float4 tosc = make_float4(t[0], t[1], t[2], t[3]);
  const uint4* tw = (const uint4*)tap_wpack;
  hipStream_t st = (hipStream_t)s;
  if (fvc_env_int("FVC_GDN_X3", 1)) {
    const dim3 g(gdn_x3_blocks(npix));
#define FVC_GX(N, I)                 \
  if (ntiles == N && !!inverse == I) \
    return fvc_launch(k_gdn_x3<N, I>, g, dim3(256), 0, st, x, P, beta, gamma, tw, tosc, npix, pcp, overflow_flag);
    FVC_GX(1, false) FVC_GX(2, false) FVC_GX(3, false) FVC_GX(4, false)
    FVC_GX(1, true) FVC_GX(2, true) FVC_GX(3, true) FVC_GX(4, true)
#undef FVC_GX
  }
#define FVC_GT(N)                                                                                               \
  if (ntiles == N)                                                                                              \
    return fvc_launch(k_gdn_tap_mfma<N>, dim3(gdn_f32_blocks(npix)), dim3(64 * kGdnWaves), 0, st, x, P, beta, gamma, \
                      tw, tosc, npix, inverse, pcp, overflow_flag);
  FVC_GT(1) FVC_GT(2) FVC_GT(3) FVC_GT(4)
#undef FVC_GT
  return FVC_EINVAL;
}

int fvc_gdn_nhwc_cai(const float* x, float* y, const float* beta, const float* gamma, int batch, int h, int w, int c,
                     int inverse, fvc_stream_t s) {
  if (!x || !y || !beta || !gamma || (c != 64 && c != 128)) return FVC_EINVAL;
  const size_t npix = (size_t)batch * h * w;
  const dim3 g(fvc_blocks(npix, kGcPix, 8192));
  if (c == 128) return fvc_launch(k_gdn_cai<128>, g, dim3(128), 0, (hipStream_t)s, x, y, beta, gamma, npix, inverse);
  return fvc_launch(k_gdn_cai<64>, g, dim3(64), 0, (hipStream_t)s, x, y, beta, gamma, npix, inverse);
}

}  // extern "C"
