// MS-SSIM over a batch of planes (include/fvc.h, fvc_ms_ssim_planes): per scale one fused kernel that
// reads X and Y once, filters X, Y, X^2, Y^2 and XY with the separable 11-tap Gaussian on chip and
// forms cs and ssim per pixel without writing a map, then a small kernel that pools both planes for
// the next scale, and at the end one kernel that sums every (scale, plane)'s block partials in a
// fixed order.
//
// A block owns a 32 x 32 tile of the valid (h-10) x (w-10) map. It stages the 42 x 42 input tile of
// both planes in LDS as float32 (exact for float32 and uint8 inputs alike), runs the horizontal pass
// from there into LDS (a lane: one input row, four adjacent columns, so 14 + 14 reads feed 220 FMAs)
// and the vertical pass from that (a lane: one column, four adjacent rows, 70 reads for 220 FMAs).
// Everything after the load is float64: sigma^2 = E[X^2] - mu^2 cancels six digits at data range 255,
// and the check this kernel answers to (twice the reference's own float32 - float64 gap) leaves a
// float32 formulation no margin, while float64 on chip costs FMA rate and LDS bytes but no HBM byte.
// Reductions: lane sums, a fixed shuffle tree, the block's four waves in order, one (cs, ssim) pair
// of doubles per block in the workspace; no floating-point atomics, so a plane's result is the same
// bits in every call and in every batch.
#include "fvc_common.h"

namespace {

constexpr int kWin = 11;             // taps
constexpr int kHalo = kWin - 1;      // a valid map is this much smaller than its input
constexpr int kTile = 32;            // outputs per block and dimension
constexpr int kIn = kTile + kHalo;   // 42 input rows / columns per block
constexpr int kInLd = 44;            // float row stride of the staged input (16-byte rows; columns 42, 43 zero)
constexpr int kBlk = 256;
constexpr int kMaxLevels = 5;

// exp(-(k-5)^2 / (2 * 1.5^2)) / sum as torch forms them in float32 (arange, pow, div, exp, sum, div)
#define FVC_SSIM_TAPS                                                                                     \
  0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,        \
      0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d957p-10f
__constant__ float kTapsDev[kWin] = {FVC_SSIM_TAPS};
const float kTapsHost[kWin] = {FVC_SSIM_TAPS};

__device__ __forceinline__ float ld(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float ld(const uint8_t* p, size_t i) { return (float)p[i]; }

// cs and ssim of one pixel from its five filtered quantities, every product and sum rounded on its
// own: with x == y numerator and denominator are then the same bits and both quotients exactly 1.
__device__ __forceinline__ void ssim_pixel(double mu1, double mu2, double exx, double eyy, double exy, double c1,
                                           double c2, double& cs, double& ss) {
#pragma clang fp contract(off)
  const double m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
  const double s1 = exx - m11, s2 = eyy - m22, s12 = exy - m12;
  cs = (2.0 * s12 + c2) / (s1 + s2 + c2);
  ss = ((2.0 * m12 + c1) / (m11 + m22 + c1)) * cs;
}

// part: [planes][tiles][2] doubles = this block's sum of cs and of ssim over its valid pixels
template <typename T>
__global__ void __launch_bounds__(kBlk)
    k_ssim_tile(const T* __restrict__ X, const T* __restrict__ Y, int h, int w, int tx_n, int ty_n, double c1, double c2,
                double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float sx[kIn][kInLd];
  __shared__ __attribute__((aligned(16))) float sy[kIn][kInLd];
  __shared__ __attribute__((aligned(16))) double hq[5][kIn][kTile];
  __shared__ double red[kBlk / 64][2];

  const int tiles = tx_n * ty_n;
  const size_t plane = blockIdx.x / (unsigned)tiles;
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const int oy = (tile / tx_n) * kTile, ox = (tile % tx_n) * kTile;
  const T* xp = X + plane * (size_t)h * w;
  const T* yp = Y + plane * (size_t)h * w;

  // stage: rows oy .. oy+41, columns ox .. ox+43, zero outside the plane (no read leaves it; a
  // valid output never uses such a zero)
  for (int i = threadIdx.x; i < kIn * kInLd; i += kBlk) {
    const int r = i / kInLd, c = i % kInLd;
    const int gr = oy + r, gc = ox + c;
    float a = 0.f, b = 0.f;
    if (c < kIn && gr < h && gc < w) {
      const size_t o = (size_t)gr * w + gc;
      a = ld(xp, o), b = ld(yp, o);
    }
    sx[r][c] = a, sy[r][c] = b;
  }
  __syncthreads();

  double tap[kWin];
#pragma unroll
  for (int k = 0; k < kWin; ++k) tap[k] = (double)kTapsDev[k];

  // horizontal pass: item = (input row r, column group g): outputs columns 4g .. 4g+3 from inputs 4g .. 4g+13
  for (int it = threadIdx.x; it < kIn * (kTile / 4); it += kBlk) {
    const int r = it / (kTile / 4), c0 = (it % (kTile / 4)) * 4;
    float a[16], b[16];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float4 p = *reinterpret_cast<const float4*>(&sx[r][c0 + 4 * v]);
      const float4 q = *reinterpret_cast<const float4*>(&sy[r][c0 + 4 * v]);
      a[4 * v] = p.x, a[4 * v + 1] = p.y, a[4 * v + 2] = p.z, a[4 * v + 3] = p.w;
      b[4 * v] = q.x, b[4 * v + 1] = q.y, b[4 * v + 2] = q.z, b[4 * v + 3] = q.w;
    }
    double acc[5][4];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[q][j] = 0.0;
#pragma unroll
    for (int k = 0; k < 14; ++k) {
      const double xv = (double)a[k], yv = (double)b[k];
      const double xx = xv * xv, yy = yv * yv, xy = xv * yv;  // exact: 24-bit factors
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = k - j;  // tap index of input k for output j
        if (t >= 0 && t < kWin) {
          acc[0][j] = fma(tap[t], xv, acc[0][j]);
          acc[1][j] = fma(tap[t], yv, acc[1][j]);
          acc[2][j] = fma(tap[t], xx, acc[2][j]);
          acc[3][j] = fma(tap[t], yy, acc[3][j]);
          acc[4][j] = fma(tap[t], xy, acc[4][j]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      double2* o = reinterpret_cast<double2*>(&hq[q][r][c0]);
      o[0] = make_double2(acc[q][0], acc[q][1]);
      o[1] = make_double2(acc[q][2], acc[q][3]);
    }
  }
  __syncthreads();

  // vertical pass: lane = (column c, row group): outputs rows r0 .. r0+3 from hq rows r0 .. r0+13
  const int c = threadIdx.x & (kTile - 1), r0 = (threadIdx.x / kTile) * 4;
  double acc[5][4];
#pragma unroll
  for (int q = 0; q < 5; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[q][j] = 0.0;
#pragma unroll
  for (int k = 0; k < 14; ++k) {
    double v[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) v[q] = hq[q][r0 + k][c];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = k - j;
      if (t >= 0 && t < kWin) {
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[q][j] = fma(tap[t], v[q], acc[q][j]);
      }
    }
  }
  double scs = 0.0, sss = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (oy + r0 + j < h - kHalo && ox + c < w - kHalo) {
      double cs, ss;
      ssim_pixel(acc[0][j], acc[1][j], acc[2][j], acc[3][j], acc[4][j], c1, c2, cs, ss);
      scs += cs, sss += ss;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    scs += __shfl_down(scs, off, 64);
    sss += __shfl_down(sss, off, 64);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = scs, red[threadIdx.x >> 6][1] = sss;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int k = 0; k < kBlk / 64; ++k) a += red[k][0], b += red[k][1];
    part[2 * (size_t)blockIdx.x] = a;
    part[2 * (size_t)blockIdx.x + 1] = b;
  }
}

// avg_pool2d(kernel 2, stride 2, padding side % 2, count_include_pad): output (k, j) is the sum of
// input rows 2k - (h & 1), +1 and columns 2j - (w & 1), +1 over 4, index -1 reading as zero. One
// lane per output pixel of both planes; the sum is formed in float64 and rounded once.
template <typename T>
__global__ void __launch_bounds__(kBlk)
    k_pool2(const T* __restrict__ X, const T* __restrict__ Y, float* __restrict__ PX, float* __restrict__ PY, size_t planes,
            int h, int w) {
  const int h2 = (h + 1) >> 1, w2 = (w + 1) >> 1;
  const size_t n = planes * h2 * w2;
  for (size_t i = blockIdx.x * (size_t)kBlk + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlk) {
    const int j = (int)(i % w2), k = (int)((i / w2) % h2);
    const size_t p = i / ((size_t)w2 * h2);
    const int ra = 2 * k - (h & 1), ca = 2 * j - (w & 1);  // ra + 1 <= h - 1 and ca + 1 <= w - 1 always
    const T* xp = X + p * (size_t)h * w;
    const T* yp = Y + p * (size_t)h * w;
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int dr = 0; dr < 2; ++dr)
#pragma unroll
      for (int dc = 0; dc < 2; ++dc) {
        const int r = ra + dr, cc = ca + dc;
        if (r >= 0 && cc >= 0) {
          const size_t o = (size_t)r * w + cc;
          sa += (double)ld(xp, o), sb += (double)ld(yp, o);
        }
      }
    PX[i] = (float)(sa * 0.25), PY[i] = (float)(sb * 0.25);
  }
}

struct Levels {
  size_t part_off[kMaxLevels];  // doubles from the partials' base
  int tiles[kMaxLevels];        // blocks per plane
  double count[kMaxLevels];     // valid pixels per plane
};

// out[level][plane] = (sum cs, sum ssim) / count: one wave per (plane, level); lane i adds tiles
// i, i+64, ... in that order, then the fixed shuffle tree
__global__ void __launch_bounds__(64) k_ssim_final(const double* __restrict__ part, Levels lv, int planes,
                                                    double* __restrict__ out) {
  const int p = blockIdx.x, l = blockIdx.y;
  const double* src = part + lv.part_off[l] + 2 * (size_t)p * lv.tiles[l];
  double a = 0.0, b = 0.0;
  for (int k = threadIdx.x; k < lv.tiles[l]; k += 64) a += src[2 * k], b += src[2 * k + 1];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  if (threadIdx.x == 0) {
    double* o = out + 2 * ((size_t)l * planes + p);
    o[0] = a / lv.count[l];
    o[1] = b / lv.count[l];
  }
}

// Host: the workspace layout. Pooled planes of levels 1 .. levels-1 (x then y, float32, each
// section 256-byte aligned), then every level's block partials. False on bad geometry.
struct Plan {
  int h[kMaxLevels], w[kMaxLevels];
  size_t px[kMaxLevels], py[kMaxLevels];  // byte offsets (level 0 unused)
  size_t part;                            // byte offset of the partials
  Levels lv;
  size_t bytes;
};

size_t rup256(size_t v) { return (v + 255) & ~(size_t)255; }

bool make_plan(int planes, int h, int w, int levels, Plan* p) {
  if (planes <= 0 || planes > 65535 || h <= 0 || w <= 0 || levels < 1 || levels > kMaxLevels) return false;
  if (((h < w ? h : w) >> (levels - 1)) < kWin) return false;  // the last scale must hold one window
  size_t off = 0, parts = 0;
  for (int l = 0; l < levels; ++l) {
    p->h[l] = l ? (p->h[l - 1] + 1) >> 1 : h;
    p->w[l] = l ? (p->w[l - 1] + 1) >> 1 : w;
    if (l) {
      const size_t b = rup256((size_t)planes * p->h[l] * p->w[l] * sizeof(float));
      p->px[l] = off, p->py[l] = off + b;
      off += 2 * b;
    }
    const int mh = p->h[l] - kHalo, mw = p->w[l] - kHalo;
    const size_t tiles = (size_t)fvc_cdiv(mh, kTile) * fvc_cdiv(mw, kTile);
    if (tiles * planes > 0x7fffffffu) return false;
    p->lv.tiles[l] = (int)tiles;
    p->lv.count[l] = (double)mh * (double)mw;
    p->lv.part_off[l] = parts;
    parts += 2 * tiles * planes;
  }
  p->part = off;
  p->bytes = off + parts * sizeof(double);
  return true;
}

template <typename T>
int launch_level(const T* x, const T* y, int planes, const Plan& p, int l, int levels, double c1, double c2, char* ws,
                 hipStream_t s) {
  const int tx = fvc_cdiv(p.w[l] - kHalo, kTile), ty = fvc_cdiv(p.h[l] - kHalo, kTile);
  double* part = reinterpret_cast<double*>(ws + p.part) + p.lv.part_off[l];
  hipLaunchKernelGGL(k_ssim_tile<T>, dim3((unsigned)(p.lv.tiles[l] * (size_t)planes)), dim3(kBlk), 0, s, x, y, p.h[l],
                     p.w[l], tx, ty, c1, c2, part);
  FVC_CHECK_LAUNCH();
  if (l + 1 < levels) {
    const size_t n = (size_t)planes * p.h[l + 1] * p.w[l + 1];
    hipLaunchKernelGGL(k_pool2<T>, dim3(fvc_blocks(n, kBlk, 4096)), dim3(kBlk), 0, s, x, y,
                       reinterpret_cast<float*>(ws + p.px[l + 1]), reinterpret_cast<float*>(ws + p.py[l + 1]),
                       (size_t)planes, p.h[l], p.w[l]);
    FVC_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" {

int fvc_ms_ssim_window(float* taps11) {
  if (!taps11) return FVC_EINVAL;
  for (int k = 0; k < kWin; ++k) taps11[k] = kTapsHost[k];
  return 0;
}

size_t fvc_ms_ssim_workspace_bytes(int planes, int h, int w, int levels) {
  Plan p;
  return make_plan(planes, h, w, levels, &p) ? p.bytes : 0;
}

int fvc_ms_ssim_planes(const void* x, const void* y, int dtype, int planes, int h, int w, int levels, double data_range,
                       void* ws, size_t ws_bytes, double* out, fvc_stream_t stream) {
  Plan p;
  if (!x || !y || !ws || !out || (dtype != FVC_DTYPE_F32 && dtype != FVC_DTYPE_U8)) return FVC_EINVAL;
  if (!make_plan(planes, h, w, levels, &p) || ws_bytes < p.bytes || !(data_range > 0.0)) return FVC_EINVAL;
  if (((uintptr_t)ws & 15) || ((uintptr_t)out & 7)) return FVC_EINVAL;
  if (dtype == FVC_DTYPE_F32 && (((uintptr_t)x | (uintptr_t)y) & 3)) return FVC_EINVAL;
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  char* wsb = static_cast<char*>(ws);
  hipStream_t s = (hipStream_t)stream;
  for (int l = 0; l < levels; ++l) {
    int st;
    if (l == 0 && dtype == FVC_DTYPE_U8) {
      st = launch_level(static_cast<const uint8_t*>(x), static_cast<const uint8_t*>(y), planes, p, l, levels, c1, c2,
                        wsb, s);
    } else {
      const float* lx = l ? reinterpret_cast<const float*>(wsb + p.px[l]) : static_cast<const float*>(x);
      const float* ly = l ? reinterpret_cast<const float*>(wsb + p.py[l]) : static_cast<const float*>(y);
      st = launch_level(lx, ly, planes, p, l, levels, c1, c2, wsb, s);
    }
    if (st) return st;
  }
  hipLaunchKernelGGL(k_ssim_final, dim3((unsigned)planes, (unsigned)levels), dim3(64), 0, s,
                     reinterpret_cast<const double*>(wsb + p.part), p.lv, planes, out);
  FVC_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
