// The split-precision ("fp16 x3") contract shared by the matrix-core conv families
// (fvc_conv_x3 / fvc_deconv_x3 / fvc_conv_wino / fvc_conv_wr7 / fvc_conv_stem). Internal: every
// definition is forceinline, constexpr or inline, nothing is exported.
//
// A value is carried as v = hi + lo * 2^-11 in two fp16 planes, hi = fp16(v) and
// lo = fp16((v - hi) * 2^11). Weights are first scaled by a per-layer 2^kw so that max|w| 2^kw lies
// in [2^13, 2^14) (fvc_split_kw) and split on the host (fvc_split_store); activations are split in
// the kernels (split2 / split8). main += hi hi goes to one fp32 accumulator, the correction products
// hi lo + lo hi to a second one that the epilogue scales by 2^-11. A staged |v| >= 65000 (or NaN)
// raises the caller's overflow flag.
#pragma once
#include "fvc_common.h"
#include <math.h>

// ---------------------------------------------------------------------------------- device side
// The kernel files pull these in with `using namespace fvc_split;` inside their own namespace.
namespace fvc_split {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr;

// Accumulation: two weight planes (hi, lo*2^11) and activations split as hi + lo*2^-11; the
// correction products go to a second accumulator scaled by 2^-11 at the end. (Measured and
// rejected, r2: one accumulator with UNSCALED residual halves -- 64 fewer VGPRs, same speed on
// every geometry (profiles/r2/x3_experiments), but an activation residual below 2^-14 is an
// fp16 subnormal and small-activation layers lose accuracy: 4.8e-4 relative at |x| ~ 1e-4.)
constexpr float kLoScale = 2048.f;

// Activations and outputs are addressed through buffer descriptors with 32-bit offsets (the host
// keeps every descriptor's range under 4 GB): a halo pixel outside the image gets an offset past
// the descriptor's range (kOob) and loads zeros (the conv's zero padding, no select), and a store
// whose lane is outside the output is dropped by the same range check -- no branches.
constexpr unsigned kOob = 0xFFFFFF00u;
constexpr int kRsrcFlags = 0x00020000;

// a raw buffer descriptor over [p, p + bytes): offsets at or past `bytes` read 0 / drop the store.
// The inputs go through readfirstlane (free on values already in SGPRs): the compiler must see the
// descriptor as uniform or it wraps every access in a waterfall loop (cdna_hip_programming.md T20).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p, unsigned bytes) {
  const unsigned long long v = (unsigned long long)(uintptr_t)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  void* const q = (void*)(uintptr_t)(((unsigned long long)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(q, (short)0, (int)__builtin_amdgcn_readfirstlane(bytes), kRsrcFlags);
}

template <int IOP>
__device__ __forceinline__ float in_op_t(float v) {
  if (IOP == FVC_IN_RELU) return fmaxf(v, 0.f);
  if (IOP == FVC_IN_ABS) return fabsf(v);
  if (IOP == FVC_IN_ROUND) return rintf(v);  // torch.round: half-to-even
  return v;
}

// max(x, 0) as one v_max_f32 (fmaxf compiles to a NaN-quieting v_max x, x first)
__device__ __forceinline__ float relu1(float x) {
  float r;
  asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(x));
  return r;
}

// v = hi + lo * 2^-11 for 8 values (packed fp16 conversions); mx tracks max |v| for the
// representability check (|v| < 65000)
__device__ __forceinline__ void split8(const float (&v)[8], h8& hi, h8& lo, float& mx) {
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const f2v x = {v[i], v[i + 1]};
    const h2v h = __builtin_convertvector(x, h2v);
    const f2v back = __builtin_convertvector(h, f2v);
    const h2v l = __builtin_convertvector((x - back) * kLoScale, h2v);
    hi[i] = h[0];
    hi[i + 1] = h[1];
    lo[i] = l[0];
    lo[i + 1] = l[1];
  }
  mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))),
                       fmaxf(fmaxf(fabsf(v[4]), fabsf(v[5])), fmaxf(fabsf(v[6]), fabsf(v[7])))));
}

// y = hi + lo * 2^-11 for two values: hi by one packed round-to-nearest conversion, the residual
// y - hi by v_fma_mix (hi read as f16 inside the FMA: exact), lo rounded straight to f16 by
// v_fma_mix{lo,hi} (5 VALU per pair instead of 8 for convert / convert back / subtract / scale /
// convert). Pure VALU asm: the hardware interlocks VALU dependencies.
__device__ __forceinline__ void split2(float v0, float v1, unsigned& hi, unsigned& lo) {
  float r0, r1;
  asm("v_cvt_pk_f16_f32 %0, %3, %4\n\t"
      "v_fma_mix_f32 %1, %0, -1.0, %3 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mix_f32 %2, %0, -1.0, %4 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(hi), "=&v"(r0), "=&v"(r1)
      : "v"(v0), "v"(v1));
  asm("v_fma_mixlo_f16 %0, %1, %3, 0\n\t"
      "v_fma_mixhi_f16 %0, %2, %3, 0"
      : "=&v"(lo)
      : "v"(r0), "v"(r1), "s"(kLoScale));
}

// The three split-precision products of one 16x16 output tile and one 32-channel k-step (Winograd
// kernels: one (position, 16-channel N-tile) pair):
//   acc += U_hi V_hi, cor += U_lo V_hi, cor += U_hi V_lo
// U is an AGPR operand ("a": the resident U registers fill the accumulator half of the file, the
// k-loop's VGPRs stay free for the transforms); hipcc does not place MFMAs with A/B operands in
// AGPRs, hence inline asm. Wait states (cdna_hip_programming.md §5.7): a VALU write of vh / vl or
// a v_accvgpr_write of U right before -> 2 states (s_nop 1, opening the string); the accumulate
// chains need none; the VALU reads of acc / cor after the last MFMA are fenced by the kernel's
// own drain (wino_mfma_drain, wr7_drain).
// FIRST: the chains start from C = 0. NOP: open with the 2 states (s_nop 1) a VALU-written vh / vl
// needs; blocks whose operands were written three or more instructions earlier skip it
// (scripts/check_wino_hazards.py audits the built .s for VALU writes of MFMA sources within 2
// states).
#define FVC_MFMA3_BODY(C0, C1)                     \
  "v_mfma_f32_16x16x32_f16 %0, %2, %4, " C0 "\n\t" \
  "v_mfma_f32_16x16x32_f16 %1, %3, %4, " C1 "\n\t" \
  "v_mfma_f32_16x16x32_f16 %1, %2, %5, %1"
template <bool FIRST, bool NOP>
__device__ __forceinline__ void mfma3(f32x4& acc, f32x4& cor, const h8& uh, const h8& ul, const h8& vh,
                                      const h8& vl) {
  if constexpr (FIRST) {
    if constexpr (NOP)
      asm volatile("s_nop 1\n\t" FVC_MFMA3_BODY("0", "0") : "=&v"(acc), "=&v"(cor) : "a"(uh), "a"(ul), "v"(vh), "v"(vl));
    else
      asm volatile(FVC_MFMA3_BODY("0", "0") : "=&v"(acc), "=&v"(cor) : "a"(uh), "a"(ul), "v"(vh), "v"(vl));
  } else {
    if constexpr (NOP)
      asm volatile("s_nop 1\n\t" FVC_MFMA3_BODY("%0", "%1") : "+v"(acc), "+v"(cor) : "a"(uh), "a"(ul), "v"(vh), "v"(vl));
    else
      asm volatile(FVC_MFMA3_BODY("%0", "%1") : "+v"(acc), "+v"(cor) : "a"(uh), "a"(ul), "v"(vh), "v"(vl));
  }
}

}  // namespace fvc_split

// ------------------------------------------------------------------------------------ host side
// CUs of the current device, queried once per process (hidden, not static: one cache for the
// whole library)
__attribute__((visibility("hidden"))) inline int fvc_num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

// CUs a persistent grid may fill: cu_reserve CUs are left out for kernels of other streams (the
// latency-bound rANS chains): a block that cannot find a free CU would start only when another
// block has finished its whole run, doubling the launch's time. Never more than half the device;
// FVC_X3_RESERVE overrides the caller's value.
static inline int fvc_persistent_cus(int cu_reserve) {
  const int forced = fvc_env_int("FVC_X3_RESERVE", -1);
  const int reserve = forced >= 0 ? forced : cu_reserve;
  const int cus = fvc_num_cus();
  return cus - (reserve < cus / 2 ? reserve : cus / 2);
}

// the caller's schedule scratch if it holds the `need` counters of a dynamic schedule, else null
// (static runs; FVC_X3_DYN=0 forces them)
static inline int* fvc_dyn_sched(int* sched, long long sched_len, long long need) {
  return (sched && sched_len >= need && fvc_env_int("FVC_X3_DYN", 1)) ? sched : nullptr;
}

// The launch tail every persistent split-precision entry point ends with (kernels._launch_tail):
// CUs left to other streams, the overflow flag, the schedule scratch with its length, the stream.
struct FvcTail {
  int cu_reserve;
  int *ovf, *sched;
  int sched_len;
  hipStream_t stream;
};
static inline bool fvc_tail_ok(const FvcTail& t) { return t.cu_reserve >= 0 && t.sched_len >= 0; }

// One launch of a split-precision conv family. An entry point lists the members up to `tail` in
// the order of its own C ABI arguments and names what else it sets: the ops, and the optional
// fused parts, absent by default.
struct FvcConvCall {
  const float* x;
  const void* wpack;
  float osc;
  const float *bias, *res;
  float* y;  // the output, or the tap partials P [batch][Ho][Wo][pcp] when tw is set
  int batch, h, w;
  FvcTail tail;
  int in_op = FVC_IN_NONE, act = FVC_ACT_NONE, post_op = FVC_POST_NONE;
  const void* tw = nullptr;  // tap epilogue: packed partial weights, their scale, channels of P
  float tosc = 0.f;
  int pcp = 0;
  float* pool = nullptr;  // avg_pool2d(y, 2) as a second output
};

struct FvcConvGeom { int cin, cout, ksize, stride, transposed; };  // the layer a call runs

// kw with max_abs * 2^kw in [2^13, 2^14), clamped to +-100; 0 for an all-zero or non-finite layer
static inline int fvc_split_kw(double max_abs) {
  if (!(max_abs > 0.0) || !isfinite(max_abs)) return 0;
  int e;
  frexp(max_abs, &e);  // max_abs = m * 2^e, m in [0.5, 1)
  const int kw = 14 - e;
  return kw < -100 ? -100 : (kw > 100 ? 100 : kw);
}

// kw of a contiguous fp32 array (largest |w|; NaNs are skipped)
static inline int fvc_split_kw_of(const float* w, size_t n) {
  float mx = 0.f;
  for (size_t i = 0; i < n; ++i) mx = fabsf(w[i]) > mx ? fabsf(w[i]) : mx;
  return fvc_split_kw(mx);
}

// the epilogue's scale of the correction accumulator: the output scale times the lo planes' 2^-11
static inline float fvc_lo_scale(float osc) { return osc * (1.0f / 2048.f); }

// activation as y = max(t, t * slope): ReLU 0, LeakyReLU 0.1, none 1
static inline float fvc_act_slope(int act) { return act == FVC_ACT_RELU ? 0.f : (act == FVC_ACT_LRELU ? 0.1f : 1.f); }

// one (already scaled) weight into its place in the hi plane and the lo * 2^11 plane
static inline void fvc_split_store(_Float16* hi_plane, _Float16* lo_plane, float v) {
  const _Float16 hi = (_Float16)v;
  *hi_plane = hi;
  *lo_plane = (_Float16)((v - (float)hi) * 2048.f);
}
