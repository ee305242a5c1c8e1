// Elementwise and reduction kernels of the DVC and RLVC forwards, all HBM-bound: layout
// conversion, 2x2 average pool, warp (grid_sample), bilinear 2x upsample-add, the SpyNet and
// motion-compensation assemble kernels, subtraction, recon/loss finalisation with the
// deterministic reductions, the bit estimators and the RLVC elementwise kernels; also fvc_version
// and fvc_device_arch_ok. GDN is in fvc_gdn.hip, the tap gathers in fvc_tap_gather.hip.
//
// Float expressions that the reference computes as separate ATen ops are written with
// contraction off (no FMA fusion) and in the reference's operand order, so results track the
// CPU path to ~1 ulp.
#include "fvc_common.h"
#include "fvc_dist.h"
#include <string.h>

#pragma clang fp contract(off)

namespace {

constexpr int kBlk = 256;
constexpr int kRedBlocks = 1024;  // fixed grid for deterministic reductions

__device__ __forceinline__ int grid_stride_start() { return blockIdx.x * blockDim.x + threadIdx.x; }

// ------------------------------------------------------------------ layout
__global__ void k_nchw_to_nhwc(const float* __restrict__ src, float* __restrict__ dst, int B, int C,
                               int H, int W, int cp) {
  const size_t npix = (size_t)B * H * W;
  for (size_t p = grid_stride_start(); p < npix; p += (size_t)gridDim.x * blockDim.x) {
    const size_t b = p / ((size_t)H * W);
    const size_t hw = p - b * H * W;
    for (int c = 0; c < cp; ++c) {
      dst[p * cp + c] = c < C ? src[(b * C + c) * H * W + hw] : 0.f;
    }
  }
}

__global__ void k_nhwc_to_nchw(const float* __restrict__ src, float* __restrict__ dst, int B, int C,
                               int H, int W, int cp, int clamp01) {
  const size_t n = (size_t)B * C * H * W;
  for (size_t e = grid_stride_start(); e < n; e += (size_t)gridDim.x * blockDim.x) {
    const size_t hw = e % ((size_t)H * W);
    const size_t bc = e / ((size_t)H * W);
    const size_t c = bc % C, b = bc / C;
    const float v = src[(b * H * W + hw) * cp + c];
    dst[e] = clamp01 ? fminf(fmaxf(v, 0.f), 1.f) : v;
  }
}

// avg_pool2d(k=2,s=2): ((x00 + x01) + x10) + x11, then / 4 (ATen CPU order)
__global__ void k_avgpool2(const float* __restrict__ src, float* __restrict__ dst, int B, int H, int W,
                           int cp) {
  const int Ho = H / 2, Wo = W / 2, c4n = cp / 4;
  const size_t n = (size_t)B * Ho * Wo * c4n;
  for (size_t e = grid_stride_start(); e < n; e += (size_t)gridDim.x * blockDim.x) {
    const int c4 = e % c4n;
    size_t p = e / c4n;
    const int ox = p % Wo; p /= Wo;
    const int oy = p % Ho;
    const size_t b = p / Ho;
    const float4* s = reinterpret_cast<const float4*>(src);
    const size_t r0 = ((b * H + 2 * oy) * W + 2 * ox) * c4n + c4;
    const size_t r1 = r0 + (size_t)W * c4n;
    const float4 a = s[r0], bb = s[r0 + c4n], c = s[r1], d = s[r1 + c4n];
    float4 o;
    o.x = (((a.x + bb.x) + c.x) + d.x) / 4.f;
    o.y = (((a.y + bb.y) + c.y) + d.y) / 4.f;
    o.z = (((a.z + bb.z) + c.z) + d.z) / 4.f;
    o.w = (((a.w + bb.w) + c.w) + d.w) / 4.f;
    reinterpret_cast<float4*>(dst)[e] = o;
  }
}

// ------------------------------------------------------------------ warp (torch_warp)
// torch.linspace(-1, 1, n)[i] as ATen computes it (symmetric two-sided formula)
__device__ __forceinline__ float linspace_m1p1(int i, int n) {
  if (n == 1) return -1.f;
  const float step = 2.f / (float)(n - 1);
  const int half = n / 2;
  return (i < half) ? (-1.f + step * (float)i) : (1.f - step * (float)(n - 1 - i));
}

struct WarpTap {
  int x0, y0;
  float nw, ne, sw, se;
  bool vx1, vy1;
};

// grid = linspace grid + flow/((n-1)/2); grid_sample(bilinear, border, align_corners=False)
// (endecoder.py:52-67; ATen CPU GridSamplerKernel unnormalize/clip/interp order)
__device__ __forceinline__ WarpTap warp_tap(int y, int x, float fx, float fy, int H, int W) {
  const float gx = linspace_m1p1(x, W) + fx / ((float)(W - 1) / 2.f);
  const float gy = linspace_m1p1(y, H) + fy / ((float)(H - 1) / 2.f);
  float ix = (gx + 1.f) * ((float)W / 2.f) - 0.5f;
  float iy = (gy + 1.f) * ((float)H / 2.f) - 0.5f;
  ix = fminf(fmaxf(ix, 0.f), (float)(W - 1));
  iy = fminf(fmaxf(iy, 0.f), (float)(H - 1));
  const float xw = floorf(ix), yn = floorf(iy);
  const float w = ix - xw, e = 1.f - w;
  const float n = iy - yn, s = 1.f - n;
  WarpTap t;
  t.x0 = (int)xw;
  t.y0 = (int)yn;
  t.nw = s * e; t.ne = s * w; t.sw = n * e; t.se = n * w;
  t.vx1 = t.x0 + 1 < W;
  t.vy1 = t.y0 + 1 < H;
  return t;
}

// the four taps in ATen's order, every product and sum rounded on its own
__device__ __forceinline__ float4 warp_blend4(const float4& vnw, const float4& vne, const float4& vsw,
                                              const float4& vse, const WarpTap& t) {
  float4 o;
  o.x = ((vnw.x * t.nw + vne.x * t.ne) + vsw.x * t.sw) + vse.x * t.se;
  o.y = ((vnw.y * t.nw + vne.y * t.ne) + vsw.y * t.sw) + vse.y * t.se;
  o.z = ((vnw.z * t.nw + vne.z * t.ne) + vsw.z * t.sw) + vse.z * t.se;
  o.w = ((vnw.w * t.nw + vne.w * t.ne) + vsw.w * t.sw) + vse.w * t.se;
  return o;
}

__device__ __forceinline__ float4 warp_sample4(const float* im, size_t bbase, int W, int c4n, int c4,
                                               const WarpTap& t) {
  const float4* s = reinterpret_cast<const float4*>(im);
  const size_t r0 = (bbase + (size_t)t.y0 * W + t.x0) * c4n + c4;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 vnw = s[r0];
  const float4 vne = t.vx1 ? s[r0 + c4n] : z;
  const float4 vsw = t.vy1 ? s[r0 + (size_t)W * c4n] : z;
  const float4 vse = (t.vx1 && t.vy1) ? s[r0 + (size_t)W * c4n + c4n] : z;
  return warp_blend4(vnw, vne, vsw, vse, t);
}

// warp_sample4 with every tap loaded unconditionally (an out-of-image tap reads the clamped edge
// pixel): when x0 + 1 == W the border clamp made ix == W - 1 exactly, so the east weights are 0 and
// the tap adds 0 * v where warp_sample4 adds 0 * 0: the same values for finite images (a zero can
// only differ in sign, and only in an exactly-zero sum); no branches, so the compiler can count the
// loads in flight exactly
__device__ __forceinline__ float4 warp_sample4_nb(const float4* __restrict__ s, unsigned bbase, int W, int H,
                                                  const WarpTap& t) {
  const unsigned r0 = bbase + (unsigned)t.y0 * W + t.x0;
  const unsigned dx = t.vx1 ? 1u : 0u, dy = t.vy1 ? (unsigned)W : 0u;
  const float4 vnw = s[r0], vne = s[r0 + dx], vsw = s[r0 + dy], vse = s[r0 + dy + dx];
  return warp_blend4(vnw, vne, vsw, vse, t);
}

__global__ void k_warp(const float* __restrict__ im, const float* __restrict__ flow, float* __restrict__ out,
                       int B, int H, int W, int cp) {
  const int c4n = cp / 4;
  const size_t npix = (size_t)B * H * W;
  for (size_t p = grid_stride_start(); p < npix; p += (size_t)gridDim.x * blockDim.x) {
    const int x = p % W;
    const int y = (p / W) % H;
    const size_t b = p / ((size_t)H * W);
    const float4 f = reinterpret_cast<const float4*>(flow)[p];
    const WarpTap t = warp_tap(y, x, f.x, f.y, H, W);
    for (int c4 = 0; c4 < c4n; ++c4)
      reinterpret_cast<float4*>(out)[p * c4n + c4] = warp_sample4(im, b * H * W, W, c4n, c4, t);
  }
}

// ------------------------------------------------------------------ bilinear upsampling
// ATen compute_indices_weights_linear, align_corners=False: src = max(scale*(d+0.5)-0.5, 0)
__device__ __forceinline__ FvcUpIdx up_index(int d, int in, int out) {
  const float scale = (float)in / (float)out;
  const float src = fmaxf(scale * ((float)d + 0.5f) - 0.5f, 0.f);
  int i0 = (int)floorf(src);
  float lam = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
  if (i0 > in - 1) i0 = in - 1;
  FvcUpIdx u;
  u.i0 = i0;
  u.i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  u.l1 = lam;
  u.l0 = 1.f - lam;
  return u;
}

// the 2x upsample kernels' index: align_corners=True with the scale (in - 1) / (out - 1) computed once on
// the host (the float division ATen performs on the CPU; the Winograd kernel's fused upsample-add
// staging takes the same host value), else the half-pixel form
__device__ __forceinline__ FvcUpIdx up2_index(int d, int in, int out, int ac, float s) {
  return ac ? fvc_up_index_scaled(d, in, s) : up_index(d, in, out);
}

__device__ __forceinline__ float4 up_sample4(const float* src, size_t bbase, int w, int c4n, int c4,
                                             const FvcUpIdx& uy, const FvcUpIdx& ux) {
  const float4* s = reinterpret_cast<const float4*>(src);
  const float4 a = s[(bbase + (size_t)uy.i0 * w + ux.i0) * c4n + c4];
  const float4 b = s[(bbase + (size_t)uy.i0 * w + ux.i1) * c4n + c4];
  const float4 c = s[(bbase + (size_t)uy.i1 * w + ux.i0) * c4n + c4];
  const float4 d = s[(bbase + (size_t)uy.i1 * w + ux.i1) * c4n + c4];
  return fvc_lerp2d4(a, b, c, d, uy, ux);
}

// 64-channel form (Warp_net's c3_u / c4_u, endecoder.py:288-293): 32-bit indexes with the pixel
// and row divisions as multiply-high by a host-computed ceil(2^32 / d) plus one correction (exact for
// any 32-bit numerator: the estimate is floor(n / d) or one above it), instead of the generic
// kernel's 64-bit divisions per float4. Same arithmetic per element as k_up2_add.
__device__ __forceinline__ unsigned udiv_magic(unsigned n, unsigned d, unsigned m) {
  unsigned q = __umulhi(n, m);
  return q * d > n ? q - 1 : q;
}

// NE elements per thread per iteration (e, e + stride, ...), all loads issued before the stores:
// more independent loads in flight per wave than a one-element loop (as k_mc_assemble_q); the skip
// tensor by non-temporal loads (it is read once)
__device__ __forceinline__ float4 up2_q16_elem(const float4* __restrict__ s4, const float* __restrict__ skip,
                                               unsigned e, unsigned H, unsigned W, int h, int w, int ac, float scale,
                                               unsigned mW, unsigned mH, float usy, float usx) {
  const unsigned c4 = e & 15u;
  const unsigned p = e >> 4;
  const unsigned row = udiv_magic(p, W, mW);
  const int x = (int)(p - row * W);
  const unsigned b = udiv_magic(row, H, mH);
  const int y = (int)(row - b * H);
  const FvcUpIdx uy = up2_index(y, h, (int)H, ac, usy), ux = up2_index(x, w, (int)W, ac, usx);
  const unsigned bb = b * (unsigned)h * (unsigned)w;
  const float4 a = s4[(bb + (unsigned)uy.i0 * w + ux.i0) * 16u + c4];
  const float4 bq = s4[(bb + (unsigned)uy.i0 * w + ux.i1) * 16u + c4];
  const float4 c = s4[(bb + (unsigned)uy.i1 * w + ux.i0) * 16u + c4];
  const float4 d = s4[(bb + (unsigned)uy.i1 * w + ux.i1) * 16u + c4];
  float4 v = fvc_lerp2d4(a, bq, c, d, uy, ux);
  if (scale != 1.f) { v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale; }
  if (skip) {
    const float* q = skip + 4 * (size_t)e;
    const float4 sk = make_float4(__builtin_nontemporal_load(q), __builtin_nontemporal_load(q + 1),
                                  __builtin_nontemporal_load(q + 2), __builtin_nontemporal_load(q + 3));
    v.x = sk.x + v.x; v.y = sk.y + v.y; v.z = sk.z + v.z; v.w = sk.w + v.w;
  }
  return v;
}

template <int NE>
__global__ void k_up2_add_q16p(const float* __restrict__ src, const float* __restrict__ skip, float* __restrict__ out,
                               int B, int h, int w, int ac, float scale, unsigned mW, unsigned mH, float usy,
                               float usx) {
  const unsigned H = 2u * h, W = 2u * w;
  const unsigned n = (unsigned)B * H * W * 16u;
  const unsigned st = gridDim.x * blockDim.x;
  const float4* s4 = reinterpret_cast<const float4*>(src);
  for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += NE * st) {
    unsigned ei[NE];
    float4 v[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      ei[k] = e + k * st < n ? e + k * st : e;
      v[k] = up2_q16_elem(s4, skip, ei[k], H, W, h, w, ac, scale, mW, mH, usy, usx);
    }
#pragma unroll
    for (int k = 0; k < NE; ++k) reinterpret_cast<float4*>(out)[ei[k]] = v[k];
  }
}

__global__ void k_up2_add(const float* __restrict__ src, const float* __restrict__ skip, float* __restrict__ out,
                          int B, int h, int w, int cp, int ac, float scale, float usy, float usx) {
  const int H = 2 * h, W = 2 * w, c4n = cp / 4;
  const size_t n = (size_t)B * H * W * c4n;
  for (size_t e = grid_stride_start(); e < n; e += (size_t)gridDim.x * blockDim.x) {
    const int c4 = e % c4n;
    size_t p = e / c4n;
    const int x = p % W; p /= W;
    const int y = p % H;
    const size_t b = p / H;
    const FvcUpIdx uy = up2_index(y, h, H, ac, usy), ux = up2_index(x, w, W, ac, usx);
    float4 v = up_sample4(src, b * h * w, w, c4n, c4, uy, ux);
    if (scale != 1.f) { v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale; }
    if (skip) {
      const float4 s = reinterpret_cast<const float4*>(skip)[e];
      v.x = s.x + v.x; v.y = s.y + v.y; v.z = s.z + v.z; v.w = s.w + v.w;
    }
    reinterpret_cast<float4*>(out)[e] = v;
  }
}

// 4-channel form of k_nchw_to_nhwc (frames and flows: C <= 4 into a 4-channel pixel): one 16-B
// store per pixel instead of four 4-B ones, the image split by a multiply-high division
__global__ void k_nchw_to_nhwc4(const float* __restrict__ src, float* __restrict__ dst, int B, int C,
                                unsigned HW, unsigned mHW) {
  const unsigned npix = (unsigned)B * HW;
  for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
    const unsigned b = udiv_magic(p, HW, mHW);
    const float* const sp = src + (size_t)b * C * HW + (p - b * HW);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (C > 0) v.x = sp[0];
    if (C > 1) v.y = sp[HW];
    if (C > 2) v.z = sp[2 * (size_t)HW];
    if (C > 3) v.w = sp[3 * (size_t)HW];
    reinterpret_cast<float4*>(dst)[p] = v;
  }
}

// ------------------------------------------------------------------ SpyNet level assembly
__device__ __forceinline__ void spynet_assemble_px(const float* __restrict__ im1, const float* __restrict__ im2,
                                                   const float* __restrict__ flow_prev, float* __restrict__ flow_up,
                                                   float* __restrict__ x8, size_t p, int x, int y, size_t b, int H,
                                                   int W) {
  const int h = H / 2, w = W / 2;
  float4 fu = make_float4(0.f, 0.f, 0.f, 0.f);
  if (flow_prev) {
    const FvcUpIdx uy = up_index(y, h, H), ux = up_index(x, w, W);
    fu = up_sample4(flow_prev, b * h * w, w, 1, 0, uy, ux);
    fu.x = fu.x * 2.f; fu.y = fu.y * 2.f; fu.z = 0.f; fu.w = 0.f;
  }
  reinterpret_cast<float4*>(flow_up)[p] = fu;
  const WarpTap t = warp_tap(y, x, fu.x, fu.y, H, W);
  const float4 wv = warp_sample4(im2, b * H * W, W, 1, 0, t);
  const float4 a = reinterpret_cast<const float4*>(im1)[p];
  float4* o = reinterpret_cast<float4*>(x8) + p * 2;
  o[0] = make_float4(a.x, a.y, a.z, wv.x);
  o[1] = make_float4(wv.y, wv.z, fu.x, fu.y);
}

__global__ void k_spynet_assemble(const float* __restrict__ im1, const float* __restrict__ im2,
                                  const float* __restrict__ flow_prev, float* __restrict__ flow_up,
                                  float* __restrict__ x8, int B, int H, int W) {
  const size_t npix = (size_t)B * H * W;
  for (size_t p = grid_stride_start(); p < npix; p += (size_t)gridDim.x * blockDim.x)
    spynet_assemble_px(im1, im2, flow_prev, flow_up, x8, p, p % W, (p / W) % H, p / ((size_t)H * W), H, W);
}

// 32-bit forms of the pixel-walking kernels (B*H*W*2 < 2^32): the pixel -> (b, y, x) split as two
// multiply-high divisions by host-computed magic numbers (udiv_magic) instead of three 64-bit
// divisions per pixel; the per-pixel arithmetic is the 64-bit kernels' (same device functions)
__global__ void k_spynet_assemble_q(const float* __restrict__ im1, const float* __restrict__ im2,
                                    const float* __restrict__ flow_prev, float* __restrict__ flow_up,
                                    float* __restrict__ x8, int B, int H, int W, unsigned mW, unsigned mH) {
  const unsigned npix = (unsigned)B * H * W;
  const unsigned st = gridDim.x * blockDim.x;
  const int h = H / 2, w = W / 2;
  const float4* const f4 = reinterpret_cast<const float4*>(flow_prev);
  const float4* const i2 = reinterpret_cast<const float4*>(im2);
  const float4* const i1 = reinterpret_cast<const float4*>(im1);
  // two pixels per iteration with every load issued ahead of the stores (see k_mc_assemble_q);
  // the flow upsample is up_sample4's arithmetic with unconditional (clamped: i1 == i0 at the
  // edge, same address) loads
  auto up = [&](unsigned b, int y, int x) -> float4 {
    if (!flow_prev) return make_float4(0.f, 0.f, 0.f, 0.f);
    const FvcUpIdx uy = up_index(y, h, H), ux = up_index(x, w, W);
    const unsigned bb = b * (unsigned)h * (unsigned)w;
    const float4 a = f4[bb + (unsigned)uy.i0 * w + ux.i0], bq = f4[bb + (unsigned)uy.i0 * w + ux.i1];
    const float4 c = f4[bb + (unsigned)uy.i1 * w + ux.i0], d = f4[bb + (unsigned)uy.i1 * w + ux.i1];
    float4 o = fvc_lerp2d4(a, bq, c, d, uy, ux);
    o.x = o.x * 2.f;
    o.y = o.y * 2.f;
    o.z = 0.f;
    o.w = 0.f;
    return o;
  };
  for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += 2 * st) {
    const unsigned p2 = p + st < npix ? p + st : p;
    const unsigned row1 = udiv_magic(p, W, mW), b1 = udiv_magic(row1, H, mH);
    const unsigned row2 = udiv_magic(p2, W, mW), b2 = udiv_magic(row2, H, mH);
    const int y1 = (int)(row1 - b1 * H), x1 = (int)(p - row1 * W);
    const int y2 = (int)(row2 - b2 * H), x2 = (int)(p2 - row2 * W);
    const float4 a1 = i1[p], a2 = i1[p2];
    const float4 fu1 = up(b1, y1, x1), fu2 = up(b2, y2, x2);
    const WarpTap t1 = warp_tap(y1, x1, fu1.x, fu1.y, H, W);
    const WarpTap t2 = warp_tap(y2, x2, fu2.x, fu2.y, H, W);
    const float4 wv1 = warp_sample4_nb(i2, b1 * H * W, W, H, t1);
    const float4 wv2 = warp_sample4_nb(i2, b2 * H * W, W, H, t2);
    float4* const fo = reinterpret_cast<float4*>(flow_up);
    float4* const o = reinterpret_cast<float4*>(x8);
    fo[p] = fu1;
    o[2 * p] = make_float4(a1.x, a1.y, a1.z, wv1.x);
    o[2 * p + 1] = make_float4(wv1.y, wv1.z, fu1.x, fu1.y);
    fo[p2] = fu2;
    o[2 * p2] = make_float4(a2.x, a2.y, a2.z, wv2.x);
    o[2 * p2 + 1] = make_float4(wv2.y, wv2.z, fu2.x, fu2.y);
  }
}

// motion compensation input: warpframe = warp(ref, mv); x8 = [warpframe, ref, 0, 0]
__device__ __forceinline__ void mc_assemble_px(const float* __restrict__ ref, const float* __restrict__ mv,
                                               float* __restrict__ warpframe, float* __restrict__ x8, size_t p,
                                               int x, int y, size_t b, int H, int W) {
  const float4 f = reinterpret_cast<const float4*>(mv)[p];
  const WarpTap t = warp_tap(y, x, f.x, f.y, H, W);
  float4 wv = warp_sample4(ref, b * H * W, W, 1, 0, t);
  wv.w = 0.f;
  reinterpret_cast<float4*>(warpframe)[p] = wv;
  const float4 r = reinterpret_cast<const float4*>(ref)[p];
  float4* o = reinterpret_cast<float4*>(x8) + p * 2;
  o[0] = make_float4(wv.x, wv.y, wv.z, r.x);
  o[1] = make_float4(r.y, r.z, 0.f, 0.f);
}

__global__ void k_mc_assemble(const float* __restrict__ ref, const float* __restrict__ mv,
                              float* __restrict__ warpframe, float* __restrict__ x8, int B, int H, int W) {
  const size_t npix = (size_t)B * H * W;
  for (size_t p = grid_stride_start(); p < npix; p += (size_t)gridDim.x * blockDim.x)
    mc_assemble_px(ref, mv, warpframe, x8, p, p % W, (p / W) % H, p / ((size_t)H * W), H, W);
}

__global__ void k_mc_assemble_q(const float* __restrict__ ref, const float* __restrict__ mv,
                                float* __restrict__ warpframe, float* __restrict__ x8, int B, int H, int W,
                                unsigned mW, unsigned mH) {
  const unsigned npix = (unsigned)B * H * W;
  const unsigned st = gridDim.x * blockDim.x;
  const float4* const r4 = reinterpret_cast<const float4*>(ref);
  // two pixels per iteration, all loads of both issued before either's stores: the gathers depend
  // on the flow load (two dependent HBM round trips per pixel), so latency, not bytes, bounds a
  // one-pixel loop
  for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += 2 * st) {
    const unsigned p2 = p + st < npix ? p + st : p;
    const float4 f1 = reinterpret_cast<const float4*>(mv)[p];
    const float4 f2 = reinterpret_cast<const float4*>(mv)[p2];
    const float4 r1 = r4[p], r2 = r4[p2];
    const unsigned row1 = udiv_magic(p, W, mW), b1 = udiv_magic(row1, H, mH);
    const unsigned row2 = udiv_magic(p2, W, mW), b2 = udiv_magic(row2, H, mH);
    const WarpTap t1 = warp_tap((int)(row1 - b1 * H), (int)(p - row1 * W), f1.x, f1.y, H, W);
    const WarpTap t2 = warp_tap((int)(row2 - b2 * H), (int)(p2 - row2 * W), f2.x, f2.y, H, W);
    float4 w1 = warp_sample4_nb(r4, b1 * H * W, W, H, t1);
    float4 w2 = warp_sample4_nb(r4, b2 * H * W, W, H, t2);
    w1.w = 0.f;
    w2.w = 0.f;
    float4* const wf = reinterpret_cast<float4*>(warpframe);
    float4* const o = reinterpret_cast<float4*>(x8);
    wf[p] = w1;
    o[2 * p] = make_float4(w1.x, w1.y, w1.z, r1.x);
    o[2 * p + 1] = make_float4(r1.y, r1.z, 0.f, 0.f);
    wf[p2] = w2;
    o[2 * p2] = make_float4(w2.x, w2.y, w2.z, r2.x);
    o[2 * p2 + 1] = make_float4(r2.y, r2.z, 0.f, 0.f);
  }
}

__global__ void k_sub(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ o, size_t n) {
  for (size_t e = grid_stride_start(); e < n; e += (size_t)gridDim.x * blockDim.x) o[e] = a[e] - b[e];
}


// ------------------------------------------------------------------ deterministic reductions
template <int K>
__device__ void block_reduce_store(double (&v)[K], double* out) {
  __shared__ double red[kBlk / 64][K];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = v[k];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) red[wid][k] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double s = 0.0;
      for (int w = 0; w < kBlk / 64; ++w) s += red[w][k];
      out[blockIdx.x * K + k] = s;
    }
  }
}

template <int K>
__global__ void k_reduce_partials(const double* __restrict__ ws, int nblocks, double* __restrict__ out) {
  __shared__ double red[kBlk][K];
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += blockDim.x)
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += ws[i * K + k];
#pragma unroll
  for (int k = 0; k < K; ++k) red[threadIdx.x][k] = s[k];
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st)
#pragma unroll
      for (int k = 0; k < K; ++k) red[threadIdx.x][k] += red[threadIdx.x + st][k];
    __syncthreads();
  }
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = red[0][k];
}

__global__ __launch_bounds__(kBlk) void k_recon_finalize(const float* __restrict__ recon, const float* __restrict__ in,
                                                         const float* __restrict__ wf, const float* __restrict__ pred,
                                                         float* __restrict__ clipped, double* __restrict__ ws,
                                                         int B, int H, int W) {
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const size_t npix = (size_t)B * H * W;
  const size_t hw = (size_t)H * W;
  for (size_t p = grid_stride_start(); p < npix; p += (size_t)gridDim.x * blockDim.x) {
    const float4 r = reinterpret_cast<const float4*>(recon)[p];
    const float4 x = reinterpret_cast<const float4*>(in)[p];
    const float4 wv = reinterpret_cast<const float4*>(wf)[p];
    const float4 pv = reinterpret_cast<const float4*>(pred)[p];
    const float rr[3] = {r.x, r.y, r.z}, xx[3] = {x.x, x.y, x.z};
    const float ww[3] = {wv.x, wv.y, wv.z}, pp[3] = {pv.x, pv.y, pv.z};
    const size_t b = p / hw, q = p - b * hw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d0 = rr[c] - xx[c], d1 = ww[c] - xx[c], d2 = pp[c] - xx[c];
      acc[0] += (double)(d0 * d0);
      acc[1] += (double)(d1 * d1);
      acc[2] += (double)(d2 * d2);
      const float cv = fminf(fmaxf(rr[c], 0.f), 1.f);
      const float d3 = cv - xx[c];
      acc[3] += (double)(d3 * d3);
      clipped[(b * 3 + c) * hw + q] = cv;
    }
  }
  block_reduce_store<4>(acc, ws);
}

__device__ __forceinline__ float bits_of_prob(float p) {
  float b = -1.0f * logf(p + 1e-5f) / 0.6931471805599453f;
  return fminf(fmaxf(b, 0.f), 50.f);
}

// Laplace bits (net.py:121-151): p = cdf(f+.5) - cdf(f-.5), cdf(v) = .5 - .5 sign(v) expm1(-|v|/s)
// (fvc_laplace_cdf)
__global__ __launch_bounds__(kBlk) void k_bits_laplace(const float* __restrict__ feat, const float* __restrict__ sigma,
                                                       double* __restrict__ ws, size_t npix, int C, int cp) {
  double acc[1] = {0.0};
  const size_t n = npix * C;
  for (size_t e = grid_stride_start(); e < n; e += (size_t)gridDim.x * blockDim.x) {
    const size_t p = e / C;
    const int c = e - p * C;
    const float f = rintf(feat[p * cp + c]);
    const float s = fminf(fmaxf(sigma[p * cp + c], 1e-5f), 1e10f);
    const float prob = fvc_laplace_cdf(f + 0.5f, s) - fvc_laplace_cdf(f - 0.5f, s);
    acc[0] += (double)bits_of_prob(prob);
  }
  block_reduce_store<1>(acc, ws);
}

__global__ __launch_bounds__(kBlk) void k_bits_factorized(const float* __restrict__ v, const float* __restrict__ prm,
                                                          double* __restrict__ ws, size_t npix, int C, int cp) {
  double acc[1] = {0.0};
  const size_t n = npix * C;
  for (size_t e = grid_stride_start(); e < n; e += (size_t)gridDim.x * blockDim.x) {
    const size_t p = e / C;
    const int c = e - p * C;
    const float q = rintf(v[p * cp + c]);
    const float prob = fvc_bitest_cdf(q + 0.5f, prm, C, c) - fvc_bitest_cdf(q - 0.5f, prm, C, c);
    acc[0] += (double)bits_of_prob(prob);
  }
  block_reduce_store<1>(acc, ws);
}



// ConvLSTM gates (entropy_models.py:367-378): f = sigmoid(f + forget_bias), i = sigmoid(i),
// c = c * f + i * relu(j), o = sigmoid(o), h = o * relu(c); NHWC tensors of C channels
__device__ __forceinline__ float sigmoid_t(float v) { return 1.f / (1.f + expf(-v)); }

__global__ void k_lstm_gates(const float* __restrict__ gj, const float* __restrict__ gi, const float* __restrict__ gf,
                             const float* __restrict__ go, const float* __restrict__ c_prev, float* __restrict__ c_out,
                             float* __restrict__ h_out, size_t n, float forget_bias) {
  for (size_t e = grid_stride_start(); e < n; e += (size_t)gridDim.x * blockDim.x) {
    const float f = sigmoid_t(gf[e] + forget_bias);
    const float ig = sigmoid_t(gi[e]);
    const float c = c_prev[e] * f + ig * fmaxf(gj[e], 0.f);
    const float o = sigmoid_t(go[e]);
    c_out[e] = c;
    h_out[e] = o * fmaxf(c, 0.f);
  }
}

// RecProbModel sigma (entropy_models.py:61-62): exp(max(sigma, -7)) / 10
__global__ void k_rpm_scale(const float* __restrict__ in, float* __restrict__ out, size_t n) {
  for (size_t e = grid_stride_start(); e < n; e += (size_t)gridDim.x * blockDim.x)
    out[e] = expf(fmaxf(in[e], -7.f)) / 10.f;
}

__device__ __forceinline__ float bits_lb(float l) {  // likelihood_lower_bound(1e-9), then the bits clamp
  return bits_of_prob(fmaxf(l, 1e-9f));
}

// compressai EntropyBottleneck, filters (3,3,3,3) (compressai EB._logits_cumulative): per
// channel prm[c][kEbPrm] = softplus(matrix0..4) (3, 9, 9, 9, 3), bias0..4 (3, 3, 3, 3, 1),
// tanh(factor0..3) (3 x 4)
constexpr int kEbPrm = 58;
__device__ float eb_logits(float v, const float* __restrict__ p) {
  const float* m0 = p;
  const float* m1 = p + 3;
  const float* m2 = p + 12;
  const float* m3 = p + 21;
  const float* m4 = p + 30;
  const float* bs = p + 33;  // b0[3] b1[3] b2[3] b3[3] b4[1]
  const float* fs = p + 46;  // f0[3] f1[3] f2[3] f3[3]
  float a[3], t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    a[r] = m0[r] * v + bs[r];
    a[r] += fs[r] * tanhf(a[r]);
  }
  const float* ms[3] = {m1, m2, m3};
#pragma unroll
  for (int l = 0; l < 3; ++l) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      float acc = ms[l][3 * r] * a[0];
      acc = fmaf(ms[l][3 * r + 1], a[1], acc);
      acc = fmaf(ms[l][3 * r + 2], a[2], acc);
      t[r] = acc + bs[3 * (l + 1) + r];
      t[r] += fs[3 * (l + 1) + r] * tanhf(t[r]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) a[r] = t[r];
  }
  float o = m4[0] * a[0];
  o = fmaf(m4[1], a[1], o);
  o = fmaf(m4[2], a[2], o);
  return o + bs[12];
}

// x_hat = round(x - median) + median; likelihood = |sigmoid(s*upper) - sigmoid(s*lower)|,
// s = -sign(lower + upper) (compressai EB._likelihood); out: x_hat and the bits sum
__global__ __launch_bounds__(kBlk) void k_eb_forward(const float* __restrict__ x, const float* __restrict__ prm,
                                                     const float* __restrict__ med, float* __restrict__ xhat,
                                                     double* __restrict__ ws, size_t npix, int C, int cp) {
  double acc[1] = {0.0};
  const size_t n = npix * C;
  for (size_t e = grid_stride_start(); e < n; e += (size_t)gridDim.x * blockDim.x) {
    const size_t p = e / C;
    const int c = (int)(e - p * C);
    const float m = med[c];
    const float v = rintf(x[p * cp + c] - m) + m;
    xhat[p * cp + c] = v;
    const float lo = eb_logits(v - 0.5f, prm + (size_t)c * kEbPrm);
    const float up = eb_logits(v + 0.5f, prm + (size_t)c * kEbPrm);
    const float sum = lo + up;
    const float sg = sum > 0.f ? -1.f : (sum < 0.f ? 1.f : 0.f);
    acc[0] += (double)bits_lb(fabsf(sigmoid_t(sg * up) - sigmoid_t(sg * lo)));
  }
  block_reduce_store<1>(acc, ws);
}

// GaussianConditional with means (compressai GC._likelihood): x_hat = round(x - mu) + mu,
// v = |x_hat - mu|, s = max(scale, 0.11), l = Phi((.5 - v)/s) - Phi((-.5 - v)/s),
// Phi(t) = .5 erfc(-t / sqrt 2)
__global__ __launch_bounds__(kBlk) void k_gc_forward(const float* __restrict__ x, const float* __restrict__ scale,
                                                     const float* __restrict__ mu, float* __restrict__ xhat,
                                                     double* __restrict__ ws, size_t npix, int C, int cp) {
  double acc[1] = {0.0};
  const size_t n = npix * C;
  const float k = -0.70710678118654752f;  // -(2^-0.5)
  for (size_t e = grid_stride_start(); e < n; e += (size_t)gridDim.x * blockDim.x) {
    const size_t p = e / C;
    const int c = (int)(e - p * C);
    const size_t o = p * cp + c;
    const float m = mu[o];
    const float xh = rintf(x[o] - m) + m;
    xhat[o] = xh;
    const float v = fabsf(xh - m);
    const float s = fmaxf(scale[o], 0.11f);
    const float up = 0.5f * erfcf(k * ((0.5f - v) / s));
    const float lo = 0.5f * erfcf(k * ((-0.5f - v) / s));
    acc[0] += (double)bits_lb(up - lo);
  }
  block_reduce_store<1>(acc, ws);
}

// Grid-stride launch over n elements: kBlk threads per block, at most 8192 blocks.
template <typename... P, typename... A>
int launch_n(void (*kernel)(P...), size_t n, fvc_stream_t s, const A&... args) {
  return fvc_launch(kernel, dim3(fvc_blocks(n, kBlk, 8192)), dim3(kBlk), 0, (hipStream_t)s, args...);
}

// A deterministic sum of K doubles: `kernel` (args..., ws among them) leaves one partial per block
// of the fixed grid in ws, k_reduce_partials adds them in a fixed order into out.
template <int K, typename... P, typename... A>
int reduce_launch(void (*kernel)(P...), double* out, double* ws, fvc_stream_t s, const A&... args) {
  const int rc = fvc_launch(kernel, dim3(kRedBlocks), dim3(kBlk), 0, (hipStream_t)s, args...);
  if (rc) return rc;
  return fvc_launch(k_reduce_partials<K>, dim3(1), dim3(kBlk), 0, (hipStream_t)s, ws, kRedBlocks, out);
}

// ceil(2^32 / d): the multiplier of udiv_magic
unsigned magic_of(unsigned long long d) { return (unsigned)(((1ull << 32) + d - 1) / d); }

}  // namespace

extern "C" {

int fvc_version(void) { return 1; }

int fvc_device_arch_ok(void) {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, 0) != hipSuccess) return 0;
  return strncmp(p.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

int fvc_nchw_to_nhwc(const float* src, float* dst, int batch, int c, int h, int w, int cp, fvc_stream_t s) {
  if (!src || !dst || c > cp || cp % 4) return FVC_EINVAL;
  const size_t n = (size_t)batch * h * w;
  const unsigned long long hw = (unsigned long long)h * w;
  if (cp == 4 && hw >= 2 && 2ull * n < (1ull << 32))
    return launch_n(k_nchw_to_nhwc4, n, s, src, dst, batch, c, (unsigned)hw, magic_of(hw));
  return launch_n(k_nchw_to_nhwc, n, s, src, dst, batch, c, h, w, cp);
}

int fvc_nhwc_to_nchw(const float* src, float* dst, int batch, int c, int h, int w, int cp, int clamp01,
                     fvc_stream_t s) {
  if (!src || !dst || c > cp) return FVC_EINVAL;
  return launch_n(k_nhwc_to_nchw, (size_t)batch * c * h * w, s, src, dst, batch, c, h, w, cp, clamp01);
}

int fvc_avgpool2_nhwc(const float* src, float* dst, int batch, int h, int w, int cp, fvc_stream_t s) {
  if (!src || !dst || (h & 1) || (w & 1) || cp % 4) return FVC_EINVAL;
  return launch_n(k_avgpool2, (size_t)batch * (h / 2) * (w / 2) * (cp / 4), s, src, dst, batch, h, w, cp);
}

int fvc_warp_nhwc(const float* im, const float* flow, float* out, int batch, int h, int w, int cp, fvc_stream_t s) {
  if (!im || !flow || !out || cp % 4 || h < 2 || w < 2) return FVC_EINVAL;
  return launch_n(k_warp, (size_t)batch * h * w, s, im, flow, out, batch, h, w, cp);
}

int fvc_upsample2x_add_nhwc(const float* src, const float* skip, float* out, int batch, int h, int w, int cp,
                            int align_corners, float scale, fvc_stream_t s) {
  if (!src || !out || cp % 4) return FVC_EINVAL;
  const size_t n = (size_t)batch * 4 * h * w * (cp / 4);
  const unsigned long long H2 = 2ull * h, W2 = 2ull * w;
  // align_corners scales (in - 1) / (out - 1), one host float division each (as ATen's CPU kernel)
  const float usy = H2 > 1 ? (float)(h - 1) / (float)(H2 - 1) : 0.f;
  const float usx = W2 > 1 ? (float)(w - 1) / (float)(W2 - 1) : 0.f;
  // 64 channels: two elements per thread with 32-bit indexes (e + 2 * stride stays below 2^32:
  // stride <= 8192 * kBlk, 2 * stride < 2^24), the skip tensor (read once: c0 / c1 are dead after this add) by
  // non-temporal loads: 1088x1920x64 at 8 frames 2.16 -> 1.99 ms (profiles/r5/up2_pair); same bits
  // as the generic kernel, which FVC_UP2_Q16=0 selects
  if (cp == 64 && n + (1ull << 24) < (1ull << 32) && fvc_env_int("FVC_UP2_Q16", 1))
    return launch_n(k_up2_add_q16p<2>, (n + 1) / 2, s, src, skip, out, batch, h, w, align_corners, scale,
                    magic_of(W2), magic_of(H2), usy, usx);
  return launch_n(k_up2_add, n, s, src, skip, out, batch, h, w, cp, align_corners, scale, usy, usx);
}

int fvc_spynet_assemble(const float* im1, const float* im2, const float* flow_prev, float* flow_up, float* x8,
                        int batch, int h, int w, fvc_stream_t s) {
  if (!im1 || !im2 || !flow_up || !x8 || (h & 1) || (w & 1) || h < 2 || w < 2) return FVC_EINVAL;
  const size_t n = (size_t)batch * h * w;
  // two pixels per thread per iteration: half as many threads as pixels
  if (2ull * n < (1ull << 32) && fvc_env_int("FVC_ASSEMBLE_Q", 1))
    return launch_n(k_spynet_assemble_q, (n + 1) / 2, s, im1, im2, flow_prev, flow_up, x8, batch, h, w, magic_of(w),
                    magic_of(h));
  return launch_n(k_spynet_assemble, n, s, im1, im2, flow_prev, flow_up, x8, batch, h, w);
}

int fvc_mc_assemble(const float* ref, const float* mv, float* warpframe, float* x8, int batch, int h, int w,
                    fvc_stream_t s) {
  if (!ref || !mv || !warpframe || !x8 || h < 2 || w < 2) return FVC_EINVAL;
  const size_t n = (size_t)batch * h * w;
  if (2ull * n < (1ull << 32) && fvc_env_int("FVC_ASSEMBLE_Q", 1))
    return launch_n(k_mc_assemble_q, (n + 1) / 2, s, ref, mv, warpframe, x8, batch, h, w, magic_of(w), magic_of(h));
  return launch_n(k_mc_assemble, n, s, ref, mv, warpframe, x8, batch, h, w);
}

int fvc_sub_f32(const float* a, const float* b, float* out, size_t n, fvc_stream_t s) {
  if (!a || !b || !out) return FVC_EINVAL;
  return launch_n(k_sub, n, s, a, b, out, n);
}

int fvc_lstm_gates(const float* gj, const float* gi, const float* gf, const float* go, const float* c_prev,
                   float* c_out, float* h_out, size_t n, float forget_bias, fvc_stream_t s) {
  if (!gj || !gi || !gf || !go || !c_prev || !c_out || !h_out) return FVC_EINVAL;
  return launch_n(k_lstm_gates, n, s, gj, gi, gf, go, c_prev, c_out, h_out, n, forget_bias);
}

int fvc_rpm_scale(const float* in, float* out, size_t n, fvc_stream_t s) {
  if (!in || !out) return FVC_EINVAL;
  return launch_n(k_rpm_scale, n, s, in, out, n);
}

int fvc_eb_forward(const float* x, const float* params, const float* medians, float* xhat, double* out1, double* ws,
                   int batch, int h, int w, int c, int cp, fvc_stream_t s) {
  if (!x || !params || !medians || !xhat || !out1 || !ws || c > cp) return FVC_EINVAL;
  return reduce_launch<1>(k_eb_forward, out1, ws, s, x, params, medians, xhat, ws, (size_t)batch * h * w, c, cp);
}

int fvc_gc_forward(const float* x, const float* scale, const float* mu, float* xhat, double* out1, double* ws,
                   int batch, int h, int w, int c, int cp, fvc_stream_t s) {
  if (!x || !scale || !mu || !xhat || !out1 || !ws || c > cp) return FVC_EINVAL;
  return reduce_launch<1>(k_gc_forward, out1, ws, s, x, scale, mu, xhat, ws, (size_t)batch * h * w, c, cp);
}

size_t fvc_reduce_ws_doubles(void) { return (size_t)kRedBlocks * 4; }

int fvc_recon_finalize(const float* recon, const float* input, const float* warpframe, const float* prediction,
                       float* clipped, double* out4, double* ws, int batch, int h, int w, fvc_stream_t s) {
  if (!recon || !input || !warpframe || !prediction || !clipped || !out4 || !ws) return FVC_EINVAL;
  return reduce_launch<4>(k_recon_finalize, out4, ws, s, recon, input, warpframe, prediction, clipped, ws, batch, h, w);
}

int fvc_bits_laplace(const float* feature, const float* sigma, double* out1, double* ws, int batch, int h, int w,
                     int c, int cp, fvc_stream_t s) {
  if (!feature || !sigma || !out1 || !ws || c > cp) return FVC_EINVAL;
  return reduce_launch<1>(k_bits_laplace, out1, ws, s, feature, sigma, ws, (size_t)batch * h * w, c, cp);
}

int fvc_bits_factorized(const float* v, const float* params, double* out1, double* ws, int batch, int h, int w,
                        int c, int cp, fvc_stream_t s) {
  if (!v || !params || !out1 || !ws || c > cp) return FVC_EINVAL;
  return reduce_launch<1>(k_bits_factorized, out1, ws, s, v, params, ws, (size_t)batch * h * w, c, cp);
}

}  // extern "C"
