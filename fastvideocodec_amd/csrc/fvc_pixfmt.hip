// 8-bit planar YUV 4:2:0 <-> float RGB with the replicate padding / display crop folded in, and the
// exact u8 sum of squared differences behind the per-plane PSNR. All three are streaming kernels:
// a lane owns 8 horizontally adjacent pixels, reads its bytes as aligned 32-bit words where the
// address allows (always at widths that are a multiple of 4, such as 1920) and clamped single
// bytes at the picture edges, and writes float4 / 32-bit words.
#include "fvc_common.h"

#include <math.h>

namespace {

constexpr int kBlk = 256;
constexpr int kPix = 8;  // pixels per lane (one row)

struct PixCoef {
  int32_t m[9];      // RGB8 -> YUV8 rows, 16 fractional bits
  int32_t yoff;      // luma offset (16 limited, 0 full); the chroma offset is always 128
  float ky, rv, gu, gv, bu;  // (Y - yoff, C16 - 2048) -> RGB in [0,1]
};

// Host: coefficient tables of one matrix / range pair. Forward rows are rint(M * 65536) with the
// largest-magnitude entry of each row adjusted so that the luma row sums to rint(s_y * 65536) and
// the chroma rows to 0: every grey level then maps Y -> RGB -> Y exactly and to U = V = 128.
bool make_coef(int matrix, int range, PixCoef* c) {
  double kr, kb;
  if (matrix == FVC_MATRIX_BT601) {
    kr = 0.299, kb = 0.114;
  } else if (matrix == FVC_MATRIX_BT709) {
    kr = 0.2126, kb = 0.0722;
  } else {
    return false;
  }
  if (range != FVC_RANGE_LIMITED && range != FVC_RANGE_FULL) return false;
  const double kg = 1.0 - kr - kb;
  const double sy = range == FVC_RANGE_LIMITED ? 219.0 / 255.0 : 1.0;
  const double sc = range == FVC_RANGE_LIMITED ? 224.0 / 255.0 : 1.0;
  const double M[9] = {sy * kr, sy * kg, sy * kb,
                       -sc * kr / (2 * (1 - kb)), -sc * kg / (2 * (1 - kb)), sc * 0.5,
                       sc * 0.5, -sc * kg / (2 * (1 - kr)), -sc * kb / (2 * (1 - kr))};
  for (int r = 0; r < 3; ++r) {
    int big = 0;
    int64_t sum = 0;
    for (int k = 0; k < 3; ++k) {
      c->m[3 * r + k] = (int32_t)rint(M[3 * r + k] * 65536.0);
      sum += c->m[3 * r + k];
      if (fabs(M[3 * r + k]) > fabs(M[3 * r + big])) big = k;
    }
    const int64_t want = r == 0 ? (int64_t)rint(sy * 65536.0) : 0;
    c->m[3 * r + big] += (int32_t)(want - sum);
  }
  c->yoff = range == FVC_RANGE_LIMITED ? 16 : 0;
  const double kc = 1.0 / (16.0 * (range == FVC_RANGE_LIMITED ? 224.0 : 255.0));
  c->ky = (float)(1.0 / (range == FVC_RANGE_LIMITED ? 219.0 : 255.0));
  c->rv = (float)(2 * (1 - kr) * kc);
  c->bu = (float)(2 * (1 - kb) * kc);
  c->gu = (float)(-2 * kb * (1 - kb) / kg * kc);
  c->gv = (float)(-2 * kr * (1 - kr) / kg * kc);
  return true;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// 4 bytes row[x .. x+3] (all inside the row) as one aligned word when the address allows
__device__ __forceinline__ void load4(const uint8_t* __restrict__ row, int x, int* o) {
  const uint8_t* p = row + x;
  if (((uintptr_t)p & 3) == 0) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
    o[0] = v & 255, o[1] = (v >> 8) & 255, o[2] = (v >> 16) & 255, o[3] = v >> 24;
  } else {
    o[0] = p[0], o[1] = p[1], o[2] = p[2], o[3] = p[3];
  }
}

__device__ __forceinline__ void store4(uint8_t* __restrict__ row, int x, const int* v) {
  uint8_t* p = row + x;
  if (((uintptr_t)p & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) |
                                      ((uint32_t)v[3] << 24);
  } else {
    p[0] = (uint8_t)v[0], p[1] = (uint8_t)v[1], p[2] = (uint8_t)v[2], p[3] = (uint8_t)v[3];
  }
}

// ------------------------------------------------------------------------------------ ingest
// Output pixel (r, c) of the padded frame is source pixel (min(r, h-1), min(c, w-1)). Chroma at a
// luma pixel is the centre-sited bilinear tap 9/3/3/1 over the nearest chroma sample and its
// neighbours towards the pixel (indices clamped to the plane), kept as an integer in 1/16 units.
__global__ void __launch_bounds__(kBlk)
    k_yuv420_to_rgb_pad(const uint8_t* __restrict__ Y, const uint8_t* __restrict__ U, const uint8_t* __restrict__ V,
                        float* __restrict__ out, int batch, int h, int w, int Hp, int Wp, PixCoef cf) {
  const int gw = Wp / kPix;
  const size_t n = (size_t)batch * Hp * gw;
  const size_t i = blockIdx.x * (size_t)kBlk + threadIdx.x;
  if (i >= n) return;
  const int g = (int)(i % gw);
  const int r = (int)((i / gw) % Hp);
  const size_t b = i / ((size_t)gw * Hp);
  const int ch = (h + 1) >> 1, cw = (w + 1) >> 1;
  const int c0 = g * kPix;
  const int rr = min(r, h - 1);
  const int cy = rr >> 1;
  const int cyn = clampi(cy + ((rr & 1) ? 1 : -1), 0, ch - 1);
  const uint8_t* yrow = Y + (b * h + rr) * (size_t)w;
  const uint8_t* un = U + (b * ch + cy) * (size_t)cw;
  const uint8_t* uf = U + (b * ch + cyn) * (size_t)cw;
  const uint8_t* vn = V + (b * ch + cy) * (size_t)cw;
  const uint8_t* vf = V + (b * ch + cyn) * (size_t)cw;

  int yv[kPix], u16[kPix], v16[kPix];
  if (c0 + kPix <= w) {
    // interior: 8 luma bytes, and chroma columns cx0-1 .. cx0+4 of the near and the far row
    load4(yrow, c0, yv);
    load4(yrow, c0 + 4, yv + 4);
    const int cx0 = c0 >> 1;  // cx0 + 3 <= cw - 1 here
    const int xl = max(cx0 - 1, 0), xr = min(cx0 + 4, cw - 1);
    int a[6], f[6], p[6], q[6];
    load4(un, cx0, a + 1);
    load4(uf, cx0, f + 1);
    load4(vn, cx0, p + 1);
    load4(vf, cx0, q + 1);
    a[0] = un[xl], a[5] = un[xr];
    f[0] = uf[xl], f[5] = uf[xr];
    p[0] = vn[xl], p[5] = vn[xr];
    q[0] = vf[xl], q[5] = vf[xr];
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
      const int k = 1 + (j >> 1), kn = k + ((j & 1) ? 1 : -1);
      u16[j] = 3 * (3 * a[k] + a[kn]) + (3 * f[k] + f[kn]);
      v16[j] = 3 * (3 * p[k] + p[kn]) + (3 * q[k] + q[kn]);
    }
  } else {
    // right edge and the padding to its right: per-pixel clamped bytes
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
      const int cc = min(c0 + j, w - 1);
      const int cx = cc >> 1;
      const int cxn = clampi(cx + ((cc & 1) ? 1 : -1), 0, cw - 1);
      yv[j] = yrow[cc];
      u16[j] = 3 * (3 * un[cx] + un[cxn]) + (3 * uf[cx] + uf[cxn]);
      v16[j] = 3 * (3 * vn[cx] + vn[cxn]) + (3 * vf[cx] + vf[cxn]);
    }
  }

  float R[kPix], G[kPix], B[kPix];
#pragma unroll
  for (int j = 0; j < kPix; ++j) {
    const float yy = cf.ky * (float)(yv[j] - cf.yoff);
    const float cb = (float)(u16[j] - 2048), cr = (float)(v16[j] - 2048);
    R[j] = clamp01(fmaf(cf.rv, cr, yy));
    G[j] = clamp01(fmaf(cf.gv, cr, fmaf(cf.gu, cb, yy)));
    B[j] = clamp01(fmaf(cf.bu, cb, yy));
  }
  const size_t plane = (size_t)Hp * Wp;
  float* o = out + b * 3 * plane + (size_t)r * Wp + c0;  // 32-byte aligned: Wp % 64 == 0, c0 % 8 == 0
  float4* oR = reinterpret_cast<float4*>(o);
  float4* oG = reinterpret_cast<float4*>(o + plane);
  float4* oB = reinterpret_cast<float4*>(o + 2 * plane);
  oR[0] = make_float4(R[0], R[1], R[2], R[3]);
  oR[1] = make_float4(R[4], R[5], R[6], R[7]);
  oG[0] = make_float4(G[0], G[1], G[2], G[3]);
  oG[1] = make_float4(G[4], G[5], G[6], G[7]);
  oB[0] = make_float4(B[0], B[1], B[2], B[3]);
  oB[1] = make_float4(B[4], B[5], B[6], B[7]);
}

// ------------------------------------------------------------------------------------ egress
// A lane owns a 2-row x 8-column patch of the display area: 16 luma bytes and 4 + 4 chroma bytes.
// Integer arithmetic after the rounding to 8 bits, so the planes are exact.
__global__ void __launch_bounds__(kBlk)
    k_rgb_to_yuv420_crop(const float* __restrict__ x, uint8_t* __restrict__ Y, uint8_t* __restrict__ U,
                         uint8_t* __restrict__ V, int batch, int h, int w, int Hp, int Wp, PixCoef cf) {
  const int ch = (h + 1) >> 1, cw = (w + 1) >> 1;
  const int gw = (w + kPix - 1) / kPix;
  const size_t n = (size_t)batch * ch * gw;
  const size_t i = blockIdx.x * (size_t)kBlk + threadIdx.x;
  if (i >= n) return;
  const int g = (int)(i % gw);
  const int cy = (int)((i / gw) % ch);
  const size_t b = i / ((size_t)gw * ch);
  const int c0 = g * kPix;  // c0 < w <= Wp and Wp % 8 == 0: the 8 columns are inside the padded row
  const size_t plane = (size_t)Hp * Wp;
  const int rows[2] = {2 * cy, min(2 * cy + 1, h - 1)};

  int yv[2][kPix], us[kPix], vs[kPix];  // us / vs: per-pixel chroma summed over the two rows
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float* p = x + b * 3 * plane + (size_t)rows[t] * Wp + c0;
    float c[3][kPix];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 lo = reinterpret_cast<const float4*>(p + k * plane)[0];
      const float4 hi = reinterpret_cast<const float4*>(p + k * plane)[1];
      c[k][0] = lo.x, c[k][1] = lo.y, c[k][2] = lo.z, c[k][3] = lo.w;
      c[k][4] = hi.x, c[k][5] = hi.y, c[k][6] = hi.z, c[k][7] = hi.w;
    }
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
      const int r8 = (int)rintf(clamp01(c[0][j]) * 255.0f);
      const int g8 = (int)rintf(clamp01(c[1][j]) * 255.0f);
      const int b8 = (int)rintf(clamp01(c[2][j]) * 255.0f);
      yv[t][j] = clampi((cf.m[0] * r8 + cf.m[1] * g8 + cf.m[2] * b8 + (cf.yoff << 16) + 32768) >> 16, 0, 255);
      const int u = clampi((cf.m[3] * r8 + cf.m[4] * g8 + cf.m[5] * b8 + (128 << 16) + 32768) >> 16, 0, 255);
      const int v = clampi((cf.m[6] * r8 + cf.m[7] * g8 + cf.m[8] * b8 + (128 << 16) + 32768) >> 16, 0, 255);
      us[j] = t ? us[j] + u : u;
      vs[j] = t ? vs[j] + v : v;
    }
  }
  // 2x2 mean; a pair's second column past the picture repeats the first (column clamp to w - 1)
  int uo[4], vo[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j1 = (c0 + 2 * k + 1 < w) ? 2 * k + 1 : 2 * k;
    uo[k] = (us[2 * k] + us[j1] + 2) >> 2;
    vo[k] = (vs[2 * k] + vs[j1] + 2) >> 2;
  }

  const int nrow = (2 * cy + 1 < h) ? 2 : 1;
  for (int t = 0; t < nrow; ++t) {
    uint8_t* yrow = Y + (b * h + rows[t]) * (size_t)w;
    if (c0 + kPix <= w) {
      store4(yrow, c0, yv[t]);
      store4(yrow, c0 + 4, yv[t] + 4);
    } else {
#pragma unroll
      for (int j = 0; j < kPix; ++j)
        if (c0 + j < w) yrow[c0 + j] = (uint8_t)yv[t][j];
    }
  }
  const int cx0 = c0 >> 1;
  uint8_t* urow = U + (b * ch + cy) * (size_t)cw;
  uint8_t* vrow = V + (b * ch + cy) * (size_t)cw;
  if (cx0 + 4 <= cw) {
    store4(urow, cx0, uo);
    store4(vrow, cx0, vo);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (cx0 + k < cw) urow[cx0 + k] = (uint8_t)uo[k], vrow[cx0 + k] = (uint8_t)vo[k];
  }
}

// ------------------------------------------------------------------------------------ metric
__device__ __forceinline__ uint32_t sq4(uint32_t a, uint32_t b) {
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = (int)((a >> (8 * k)) & 255) - (int)((b >> (8 * k)) & 255);
    s += (uint32_t)(d * d);
  }
  return s;
}

// sum (a - b)^2 over n bytes: 16-byte loads over the common aligned body, bytes for the rest;
// wave shuffle, then LDS across the block's waves, then one integer atomic per block.
__global__ void __launch_bounds__(kBlk)
    k_sse_u8(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, size_t n, int vec,
             unsigned long long* __restrict__ out) {
  const size_t tid = blockIdx.x * (size_t)kBlk + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * kBlk;
  unsigned long long acc = 0;
  const size_t nv = vec ? n / 16 : 0;
  const uint4* a4 = reinterpret_cast<const uint4*>(a);
  const uint4* b4 = reinterpret_cast<const uint4*>(b);
  for (size_t i = tid; i < nv; i += nth) {
    const uint4 p = a4[i], q = b4[i];
    acc += sq4(p.x, q.x) + sq4(p.y, q.y) + sq4(p.z, q.z) + sq4(p.w, q.w);  // <= 16 * 255^2: fits 32 bits
  }
  for (size_t i = nv * 16 + tid; i < n; i += nth) {
    const int d = (int)a[i] - (int)b[i];
    acc += (unsigned)(d * d);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ unsigned long long part[kBlk / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < kBlk / 64; ++k) s += part[k];
    if (s) atomicAdd(out, s);
  }
}

bool bad_geometry(int batch, int h, int w, int hp, int wp) {
  return batch <= 0 || h <= 0 || w <= 0 || hp < h || wp < w || hp % 64 || wp % 64;
}

}  // namespace

extern "C" {

int fvc_pixfmt_coeffs(int matrix, int range, int32_t* fwd9, int32_t* offs2, float* inv5) {
  PixCoef c;
  if (!fwd9 || !offs2 || !inv5 || !make_coef(matrix, range, &c)) return FVC_EINVAL;
  for (int k = 0; k < 9; ++k) fwd9[k] = c.m[k];
  offs2[0] = c.yoff, offs2[1] = 128;
  inv5[0] = c.ky, inv5[1] = c.rv, inv5[2] = c.gu, inv5[3] = c.gv, inv5[4] = c.bu;
  return 0;
}

int fvc_yuv420_to_rgb_pad(const uint8_t* y, const uint8_t* u, const uint8_t* v, float* out, int batch, int h, int w,
                          int hp, int wp, int matrix, int range, fvc_stream_t s) {
  PixCoef c;
  if (!y || !u || !v || !out || bad_geometry(batch, h, w, hp, wp) || !make_coef(matrix, range, &c)) return FVC_EINVAL;
  if ((uintptr_t)out & 15) return FVC_EINVAL;
  const size_t blocks = ((size_t)batch * hp * (wp / kPix) + kBlk - 1) / kBlk;
  if (blocks > 0x7fffffffu) return FVC_EINVAL;
  hipLaunchKernelGGL(k_yuv420_to_rgb_pad, dim3((unsigned)blocks), dim3(kBlk), 0, (hipStream_t)s, y, u, v, out, batch,
                     h, w, hp, wp, c);
  FVC_CHECK_LAUNCH();
  return 0;
}

int fvc_rgb_to_yuv420_crop(const float* x, uint8_t* y, uint8_t* u, uint8_t* v, int batch, int h, int w, int hp,
                           int wp, int matrix, int range, fvc_stream_t s) {
  PixCoef c;
  if (!x || !y || !u || !v || bad_geometry(batch, h, w, hp, wp) || !make_coef(matrix, range, &c)) return FVC_EINVAL;
  if ((uintptr_t)x & 15) return FVC_EINVAL;
  const size_t blocks = ((size_t)batch * ((h + 1) / 2) * ((w + kPix - 1) / kPix) + kBlk - 1) / kBlk;
  if (blocks > 0x7fffffffu) return FVC_EINVAL;
  hipLaunchKernelGGL(k_rgb_to_yuv420_crop, dim3((unsigned)blocks), dim3(kBlk), 0, (hipStream_t)s, x, y, u, v, batch,
                     h, w, hp, wp, c);
  FVC_CHECK_LAUNCH();
  return 0;
}

int fvc_sse_u8(const uint8_t* a, const uint8_t* b, size_t n, uint64_t* out, fvc_stream_t s) {
  if (!a || !b || !out || n == 0) return FVC_EINVAL;
  hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t), (hipStream_t)s);
  if (e != hipSuccess) return -(int)e;
  const int vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
  size_t blocks = (n / 16 + kBlk - 1) / kBlk;  // one 16-byte word per lane, capped: the rest strides
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_sse_u8, dim3((unsigned)blocks), dim3(kBlk), 0, (hipStream_t)s, a, b, n, vec,
                     reinterpret_cast<unsigned long long*>(out));
  FVC_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
