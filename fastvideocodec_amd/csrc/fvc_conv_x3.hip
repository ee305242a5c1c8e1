// Split-precision implicit-GEMM convolution / transposed convolution on the fp16 matrix cores
// (v_mfma_f32_32x32x16_f16), at fp32-level accuracy.
//
// Replaces the same ATen conv2d / conv_transpose2d calls as fvc_conv.hip (DVC/subnet/
// endecoder.py:142-169 MEBasic 7x7, :228-296 Warp_net/ResBlock 3x3, analysis_mv.py /
// synthesis_mv.py 3x3, analysis.py / synthesis.py / prior nets 5x5 s2) for every layer whose
// padded input channel count is a multiple of 8.
//
// Numerics ("fp16 x3"): every fp32 operand v is split exactly as v = hi + lo * 2^-11 with
// hi = fp16(v), lo = fp16((v - hi) * 2^11) (the residual scaled back into fp16's normal range,
// so the split keeps ~22 significant bits for any |v| in [6.1e-5, 65504]). Weights are first
// scaled by a per-layer power of two 2^kw so that max|w| 2^kw lies in [2^13, 2^14). A 32x32 output
// tile keeps two fp32 accumulators:
//     main += hi_x * hi_w                       (one MFMA)
//     corr += hi_x * lo_w + lo_x * hi_w         (two MFMAs)
// and the epilogue forms (main + corr * 2^-11) * 2^-kw + bias. The omitted lo*lo term is
// ~2^-22 relative; fp16 products are exact in the fp32 accumulator, so the result tracks an
// fp32 conv to ~1e-6 relative (tests/test_gpu_kernels.py bounds it like the fp32 kernel).
// Three fp16 MFMAs (3 x 32 cycles per K=16) replace eight fp32 ones (8 x 64 cycles): 5.3x
// less matrix time per MAC. An activation with |v| >= 65000 (or NaN) cannot be represented:
// the staging code ORs 1 into the caller's device flag (overflow_flag argument) instead of
// silently saturating; the host layer checks it and recomputes on the fp32 kernels.
//
// Tiling: GEMM M = output pixels (32-pixel strips), N = output channels (32-channel N-tiles),
// K = taps x input channels walked in k8-blocks = (tap, 8 consecutive channels). One MFMA
// consumes two k8-blocks: lanes 0-31 hold k8-block 2s, lanes 32-63 hold 2s+1, 8 fp16 each.
//  * a block = 8 waves stacked vertically, each WM strips x WN N-tiles (2 accumulators per
//    tile); grid = (spatial tiles, N-tile groups, batch x parity classes);
//  * the input halo tile of one channel chunk (CC channels) is staged in LDS as
//    [pixel][hi CC | lo CC] fp16 with the pixel stride padded to 16 x odd bytes, so the
//    ds_read_b128 of 32 strip pixels is conflict-free; stride-2 convs store the tile columns
//    parity-split (even columns, then odd) so their strips also read consecutive pixels;
//  * two LDS buffers: while chunk c is multiplied, every thread stages one item of chunk c+1 per
//    k-step (global load before the MFMAs, split + LDS write after) -> one barrier per chunk;
//  * weights are pre-split at pack time into [class][chunk][k-step][N-tile][hi|lo][lane] 16-B
//    fragments, read from L2 straight into VGPRs (1 KB contiguous per wave instruction),
//    software-pipelined one k-step ahead together with the LDS reads;
//  * transposed convs: stride^2 output-parity classes, each a stride-1 conv with a tap subset;
//  * epilogue: scale + bias, ReLU / LeakyReLU(0.1), residual add, exp; pad channels = 0.
#include "fvc_dx.h"
#include "fvc_split.h"

namespace {

using namespace fvc_split;

constexpr int kMaxTapsX = 49;

constexpr int kNPL = 2;                   // weight planes per (k-step, N-tile): hi, lo
constexpr int kFrag = 64 * kNPL;          // uint4 per (k-step, N-tile)
// internal post-op of the fused tap path (fvc_conv2d_nhwc_x3_tap): not part of the public enum
constexpr int kPostTap = 2;
// internal post-op of fvc_conv2d_nhwc_x3_pool: y and its 2x2 average pool (stride-1 convs, WM = 2)
constexpr int kPostPool = 3;

struct X3Args {
  const float* x;
  const uint4* w;
  const float* bias;
  const float* res;
  float* y;
  int B, H, W, cinp;
  int Ho, Wo, coutp, cout;
  int Hq, Wq;
  int sin, sout, nclass, nchunks, ntp;
  int dymin, dxmin, ir, ic, half;  // half > 0: parity-split tile columns (stride-2 conv)
  int in_op, act, post_op;
  float osc, osc_c;                // 2^-kw, 2^-kw-11
  float inv_ic;                    // 1 / ic
  float act_slope;                 // 0 (ReLU), 0.1 (LeakyReLU), 1 (none)
  int nks[4];                      // k-steps per chunk, per class
  int ntaps[4];
  int oy0[4], ox0[4];
  long long wcls[4];               // uint4 offset of each class in the pack
  int ps;                          // LDS plane stride (halves): 8 x (pixels rounded to 8 mod 16)
  unsigned y_bytes;                // bytes of y (and res): < 4 GB - 4 KB, the buffer range
  unsigned x_bytes;                // bytes of one input image: < 4 GB - 4 KB
  int xcd;                         // XCD-aware mapping of blocks to tile runs (static schedule)
  int* sched;                      // dynamic schedule (may be null: static runs): sched[0] = blocks
                                   // finished, sched[1 + y * B + z] = next work item of group (y, z);
                                   // zero on entry, reset to zero by the last block
  int* ovf;                        // caller's overflow flag (device int; may be null)
  unsigned res_bytes;              // bytes of res (its own descriptor range)
  // POST == kPostTap: the epilogue applies the next layer's 1x1 tap-partial GEMM to the finished
  // output tile and writes P [B][Ho][Wo][pcp] to y instead of the tile itself
  const uint4* tw;                 // tap weights [k16 block][hi|lo][lane] (fvc_x3_tap_pack_weight)
  float tosc, tosc_c;              // 2^-kt, 2^-kt-11
  int pcp;                         // P channels (partials rounded up to 4, <= 32)
  // POST == kPostPool: the epilogue also writes avg_pool2d(y) (2x2, stride 2) to pool
  float* pool;
  unsigned pool_bytes;
  int toff[4][kMaxTapsX + 1];      // LDS offset (halves) of each tap's window; 0 past ntaps
  // pair-tap form (stride-1 convs with 16 output channels): an N-tile's rows 16-31 hold the same 16
  // channels' weights of the odd tap (ky, kx + 1) of each (ky, even kx) pair, multiplied with the even
  // tap's window: row 16 + c of pixel p is tap (ky, kx + 1)'s product for output pixel p - 1, so the
  // epilogue adds it from lane p + 1 and every strip of 32 pixels finishes 31 output columns
  int pt;
};

// Wave grid: the NWV waves of a block stack vertically, each WM strips x WN N-tiles; every wave owns
// the block's N-tiles nt0 .. nt0 + WN - 1 and fetches their weight fragments itself from L2.
template <int CC, int WM, int WN, int IOP, int POST, int NWV>
__global__ __launch_bounds__(NWV * 64) void conv_x3_kernel(const X3Args a) {
  constexpr int C8 = CC / 8;
  constexpr int TH = NWV * WM;
  constexpr int TW = 32;
  constexpr int NT = NWV * 64;       // threads staging the first tile
  constexpr int NTS = NWV * 64;      // threads staging later chunks

  extern __shared__ __attribute__((aligned(16))) _Float16 smh[];
  const int tile_h = 2 * C8 * a.ps;  // halves per A buffer: 2*C8 planes (hi octets, lo octets)
  _Float16* const tile0 = smh + 512;  // two buffers at tile0 and tile0 + tile_h (LDS pointers;
                                      // no pointer array, which would degrade them to flat)
  // LDS header (1 KB): bias of this block's N-tiles [WN * 32] floats at bytes 0..511, the staging
  // sink at 512..543, the work-item queue at 576..591
  float* const sbias = reinterpret_cast<float*>(smh);
  static_assert(WN * 32 * 4 <= 512, "bias area");
  _Float16* const sdump = smh + 256;  // 32 B sink for staging writes of items past the tile
  int* const squeue = reinterpret_cast<int*>(smh) + 144;  // item k of this block at squeue[k & 3]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform (scalar branches)
  const int li = lane & 31;
  const int lh = lane >> 5;
  const int b = blockIdx.z;
  const int TWo = a.pt ? TW - 1 : TW;  // output columns per tile
  const int tiles_x = (a.Wq + TWo - 1) / TWo;
  const int ntiles = tiles_x * ((a.Hq + TH - 1) / TH);
  // persistent over a contiguous run of work items w = tile * nclass + class (row-major tiles:
  // neighbours share halo rows and columns in this CU's L2; all parity classes of a transposed
  // conv's tile run back to back on one CU, so their shared input tile is fetched from HBM once
  // and every block gets the same mix of 4- / 2- / 1-tap classes); the staging pipeline runs on
  // across item boundaries
  const int nitems = ntiles * a.nclass;
  // Work items are taken from the group's counter (a.sched: dynamic schedule; a block that
  // starts late -- its CU held by another stream's kernel -- just takes fewer items), or as a
  // static contiguous run per block. The queue holds items k .. k+2 of this block: item k+2 is
  // taken (one atomic by thread 0) when item k starts and published at the end of its first
  // chunk, so item k+1 is in LDS before its chunk 0 is staged during item k's last chunk.
  // Static runs are XCD-aware: consecutive block ids are dispatched round-robin to the 8 XCDs,
  // so logical run lb = (b % 8)-major gives each XCD's blocks one contiguous band of the image.
  int* const ctr = a.sched ? a.sched + 1 + blockIdx.z * gridDim.y + blockIdx.y : nullptr;
  int lb = blockIdx.x;
  if (a.xcd) {
    const int G = gridDim.x, q8 = G / 8, r8 = G % 8, x8 = lb % 8;
    lb = (x8 < r8 ? x8 * (q8 + 1) : r8 * (q8 + 1) + (x8 - r8) * q8) + lb / 8;
  }
  const int run_begin = (int)(((long long)nitems * lb) / gridDim.x);
  const int run_end = (int)(((long long)nitems * (lb + 1)) / gridDim.x);
  auto take = [&](int k) -> int {  // thread 0 only
    if (ctr) return atomicAdd(ctr, 1);
    return run_begin + k < run_end ? run_begin + k : nitems;
  };
  auto finish = [&]() {  // every block, once: the last one leaves the schedule zeroed
    if (ctr && tid == 0) {
      __threadfence();
      const int nblk = (int)(gridDim.x * gridDim.y * gridDim.z);
      if (atomicAdd(a.sched, 1) == nblk - 1) {
        for (int g = 0; g < (int)(gridDim.y * gridDim.z); ++g) atomicExch(a.sched + 1 + g, 0);
        atomicExch(a.sched, 0);
      }
    }
  };
  if (tid == 0) {
    squeue[0] = take(0);
    squeue[1] = take(1);
  }
  __syncthreads();
  const int w_first = squeue[0];
  if (w_first >= nitems) {
    finish();
    return;
  }
  const int nt0 = blockIdx.y * WN;  // first N-tile of the block
  int cls = w_first % a.nclass;
  int nq = a.nks[cls];
  const int hf = a.half;
  const int nch = a.nchunks;
  const int tile_items = a.ir * a.ic * C8;
  const int nstage = (tile_items + NTS - 1) / NTS;
  const int stid = tid;  // staging thread index
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(a.x + (size_t)b * a.H * a.W * a.cinp), (short)0, (int)a.x_bytes, kRsrcFlags);
  const uint4* wcls = a.w + a.wcls[cls];  // (cls, nq, wcls, tap_tab: updated per work item)
  float mx = 0.f;  // max |staged value| (fp16 representability check)

  // one staging item = 8 channels of one halo pixel: 2 x 16-B buffer loads -> hi/lo h8 in LDS.
  // fetch always issues its two loads (halo pixels outside the image read zeros through the
  // descriptor's range check), so the k-loop has no divergent branches and the compiler can
  // count vmcnt exactly; in_op, the split and the LDS write happen in store, after the MFMAs.
  struct Stage {
    float4 v0, v1;
    int dst;
    bool ok;
  };
  auto fetch = [&](int e, int tile, int ch, Stage& st) {
    st.ok = e < tile_items;  // past the end: loads of a clamped index, no LDS write
    e = st.ok ? e : tile_items - 1;
    const int o = e & (C8 - 1);
    const int p = e / C8;
    const int r = (int)(((float)p + 0.5f) * a.inv_ic);  // exact: p < 2^14, ic <= 128
    const int c = p - r * a.ic;
    const int iy = (tile / tiles_x) * TH * a.sin + a.dymin + r;
    const int ix = (tile % tiles_x) * TWo * a.sin + a.dxmin + c;
    const bool inb = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
    const unsigned off = inb ? ((unsigned)(iy * a.W + ix) * (unsigned)a.cinp + (unsigned)(ch * CC + o * 8)) * 4u : kOob;
    st.v0 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
    // 4-channel inputs (cin 2 / 3): the octet's upper half is zero padding -- the second load goes past
    // the descriptor's range and returns zeros (no branch)
    st.v1 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, a.cinp == 4 ? kOob : off + 16u, 0, 0));
    const int cpos = hf ? ((c & 1) * hf + (c >> 1)) : c;
    st.dst = o * a.ps + (r * a.ic + cpos) * 8;  // plane o (hi), pixel-minor
  };
  auto store = [&](_Float16* t, const Stage& st) {
    float v[8] = {st.v0.x, st.v0.y, st.v0.z, st.v0.w, st.v1.x, st.v1.y, st.v1.z, st.v1.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = in_op_t<IOP>(v[i]);  // zero padding stays zero
    h8 hi, lo;
    split8(v, hi, lo, mx);
    // branch-free (keeps the split in the MFMA basic block for interleaving): items past the
    // tile write to a sink
    _Float16* const ph = st.ok ? t + st.dst : sdump;
    _Float16* const pl = st.ok ? t + st.dst + C8 * a.ps : sdump + 8;
    *reinterpret_cast<h8*>(ph) = hi;
    *reinterpret_cast<h8*>(pl) = lo;
  };

  for (int e = tid; e < tile_items; e += NT) {
    Stage st;
    fetch(e, w_first / a.nclass, 0, st);
    store(tile0, st);
  }
  if (tid < WN * 32) {
    const int j = nt0 * 32 + tid;
    sbias[tid] = j < a.cout ? a.bias[j] : 0.f;
  }

  // Row of this wave in the block's column of NWV waves, and its N-group, which is always 0: wave comes
  // from readfirstlane, so the compiler cannot see wave < NWV and keeps both as arithmetic. Folding them
  // by hand (wm_ = wave, ntw = nt0) moves the register allocation of 36 of the 90 instantiations (spill
  // counts by up to 6 VGPRs either way), so they stay as the compiler has always seen them.
  const int wm_ = wave % NWV;
  const int wg_ = wave / NWV;
  const int ntw = nt0 + wg_ * WN;           // first N-tile of this wave
  const int pix0 = (((wm_ * WM) * a.sin) * a.ic + li) * 8;  // strip m adds m * pix_m (halves)
  const int pix_m = a.sin * a.ic * 8;
  // tap window offsets live one per lane; v_readlane turns them into wave-uniform scalars
  // without a memory wait inside the k-loop
  int tap_tab = a.toff[cls][lane <= kMaxTapsX ? lane : kMaxTapsX];
  __syncthreads();

  struct Ops {
    h8 ah[WM], al[WM];
    uint4 bh[WN], bl[WN];
  };
  f32x16 acc[WM][WN], cor[WM][WN];
  int buf = 0;  // LDS buffer holding the chunk being multiplied
  const __amdgpu_buffer_rsrc_t ry =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.y, (short)0, (int)a.y_bytes, kRsrcFlags);
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.res, (short)0, (int)a.res_bytes, kRsrcFlags);
  for (int k = 0;; ++k) {
    const int w = squeue[k & 3];
    if (w >= nitems) break;
    int taken = 0;
    if (tid == 0) taken = take(k + 2);
    const int tile = w / a.nclass;
    if (k != 0) {
      cls = w % a.nclass;
      nq = a.nks[cls];
      wcls = a.w + a.wcls[cls];
      tap_tab = a.toff[cls][lane <= kMaxTapsX ? lane : kMaxTapsX];
    }
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
      for (int n = 0; n < WN; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc[m][n][r] = 0.f;
          cor[m][n][r] = 0.f;
        }

    // K loop over channel chunks. Two operand register sets (ping-pong, no copies). Each
    // half-step issues the LDS and global loads of the next k-step (index clamped: the last
    // prefetch is a harmless repeat) and, in the first k-steps of a chunk, one staging load of
    // the next chunk (of this tile, or chunk 0 of the next tile); then its MFMAs; then the staging
    // LDS write. All loads are unconditional and sched_barrier pins the order, so every load has
    // a full k-step of MFMA work to land behind.
    for (int ch = 0; ch < nch; ++ch) {
      const _Float16* cur = tile0 + buf * tile_h;
      _Float16* nxt = tile0 + (buf ^ 1) * tile_h;
      const bool last = ch + 1 == nch;
      const int s_item = last ? squeue[(k + 1) & 3] : w;
      const int s_tile = s_item / a.nclass;
      const int s_ch = last ? 0 : ch + 1;
      const bool stage_next = s_item < nitems;
      const uint4* wch = wcls + (size_t)ch * nq * a.ntp * kFrag;
      // k-step q: lane half lh takes k8-block kb = 2q + lh = (tap kb / C8, octet kb % C8)
      auto load = [&](int q, Ops& op) {
        int toff;
        if (C8 == 1) {
          const int t0 = __builtin_amdgcn_readlane(tap_tab, 2 * q);
          const int t1 = __builtin_amdgcn_readlane(tap_tab, 2 * q + 1);
          toff = lh ? t1 : t0;
        } else {
          toff = __builtin_amdgcn_readlane(tap_tab, (2 * q) / C8) + (((2 * q) & (C8 - 1)) + lh) * a.ps;
        }
#pragma unroll
        for (int m = 0; m < WM; ++m) {
          op.ah[m] = *reinterpret_cast<const h8*>(cur + pix0 + m * pix_m + toff);
          op.al[m] = *reinterpret_cast<const h8*>(cur + pix0 + m * pix_m + toff + C8 * a.ps);
        }
        const uint4* wk = wch + ((size_t)q * a.ntp + ntw) * kFrag + lane;
#pragma unroll
        for (int n = 0; n < WN; ++n) {
          op.bh[n] = wk[n * kFrag];
          op.bl[n] = wk[n * kFrag + 64];
        }
      };
      // weights as the A (row) operand, pixels as B: the 32x32 result is channel x pixel, so
      // each lane ends up with 4 consecutive channels of one pixel per register group (16-B
      // epilogue stores)
      auto mfmas = [&](const Ops& op) {
#pragma unroll
        for (int m = 0; m < WM; ++m)
#pragma unroll
          for (int n = 0; n < WN; ++n) {
            const h8 wh = __builtin_bit_cast(h8, op.bh[n]);
            const h8 wl = __builtin_bit_cast(h8, op.bl[n]);
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, op.ah[m], acc[m][n], 0, 0, 0);
            cor[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, op.ah[m], cor[m][n], 0, 0, 0);
            cor[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, op.al[m], cor[m][n], 0, 0, 0);
          }
      };
      // order pins inside a half-step (loads, then MFMAs) and closing it
      auto pin = [&]() { __builtin_amdgcn_sched_barrier(0); };
      auto close = [&]() { __builtin_amdgcn_sched_barrier(0); };
      auto half_plain = [&](int q, const Ops& use, Ops& nxt_ops) {
        load(q + 1 < nq ? q + 1 : nq - 1, nxt_ops);
        pin();
        mfmas(use);
        close();
      };
      int staged = 0;
      Ops S0, S1;
      load(0, S0);
      // staging items of the next chunk are spread evenly over the k-step pairs (one per staged
      // pair) so their VALU work interleaves with MFMA-only steps instead of bunching up at the
      // chunk start, where every wave would be VALU-bound at once
      const int npair = nq >> 1;
      const int nst = stage_next ? min(nstage, npair) : 0;
      const int spread = nst ? max(1, npair / nst) : 1;
      int q = 0;
      for (; staged < nst; ++staged) {
        // the staged item's split + LDS write come after the pair's second half-step, so its
        // loads have two half-steps of MFMAs (both waves of the SIMD) to land behind
        load(q + 1 < nq ? q + 1 : nq - 1, S1);
        Stage st;
        fetch(stid + staged * NTS, s_tile, s_ch, st);
        pin();
        mfmas(S0);
        close();
        load(q + 2 < nq ? q + 2 : nq - 1, S0);
        pin();
        mfmas(S1);
        close();
        store(nxt, st);
        q += 2;
        for (int r = 1; r < spread; ++r, q += 2) {
          half_plain(q, S0, S1);
          half_plain(q + 1, S1, S0);
        }
      }
      for (; q + 1 < nq; q += 2) {
        half_plain(q, S0, S1);
        half_plain(q + 1, S1, S0);
      }
      if (nq & 1) mfmas(S0);
      if (stage_next) {
        for (int qs = staged; qs < nstage; ++qs) {
          Stage st;
          fetch(stid + qs * NTS, s_tile, s_ch, st);
          store(nxt, st);
        }
      }
      if (ch == 0 && tid == 0) squeue[(k + 2) & 3] = taken;
      __syncthreads();
      buf ^= 1;
    }

    // epilogue of this tile (its global stores drain while the next tile's k-loop runs).
    // Lane (li, lh) holds pixel qx0 + li of strip m; register group g (r = 4g..4g+3) holds output
    // channels N-tile*32 + 8g + 4lh + {0..3} -> one 16-B store (and residual load) per group.
    // Activation as one max: relu = max(v, 0*v), lrelu = max(v, 0.1*v), none = max(v, 1*v).
    // Pad channels need no select: their weights and bias are 0 and every residual tensor's pad
    // channels are 0, so they come out 0 -- except after exp (POST), which selects them to 0.
    const int qy0 = (tile / tiles_x) * TH, qx0 = (tile % tiles_x) * TWo;
    const bool px_ok = qx0 + li < a.Wq && li < TWo;
    auto pix_of = [&](int m) {  // output pixel index of this lane in strip m
      const unsigned qy = qy0 + wm_ * WM + m;
      return ((unsigned)b * a.Ho + qy * a.sout + a.oy0[cls]) * a.Wo + a.ox0[cls] + (unsigned)(qx0 + li) * a.sout;
    };
    auto voff_of = [&](int m, int n) {
      return pix_of(m) * (unsigned)a.coutp * 4u + (unsigned)((ntw + n) * 32 + 4 * lh) * 4u;
    };
    if constexpr (POST == kPostTap) {
      // Fused tap-partial epilogue (the next layer is a cout <= 4 conv computed as a 1x1 GEMM to
      // P = k*k*cout tap partials per pixel + fvc_tap_gather_nhwc). This wave holds every output
      // channel of its strips (WN = all N-tiles): lane (li, lh) has channel
      // 32n + 8g + 4lh + i of pixel li in register 4g + i of tile (m, n), so registers 8gp..8gp+7
      // of tile n are exactly the B operand of the k16 block kb = 2n + gp (channels
      // 32n + 16gp + {0-3, 8-11 | 4-7, 12-15} for lane half 0 | 1; the tap pack uses the same order).
      // The finished values y are split hi/lo like staged activations and multiplied with the
      // same three MFMAs per block; P = main * 2^-kt + corr * 2^-kt-11.
#pragma unroll
      for (int m = 0; m < WM; ++m) {
        const unsigned pix = pix_of(m);
        const bool row_ok = qy0 + wm_ * WM + m < a.Hq && px_ok;
        f32x16 pa, pc;
#pragma unroll
        for (int r = 0; r < 16; ++r) pa[r] = pc[r] = 0.f;
        // tile by tile: finish y of N-tile n (bias, act, residual), then its two k16 blocks, so
        // only one tile's y is live next to the partial accumulators
#pragma unroll
        for (int n = 0; n < WN; ++n) {
          float yv[16];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float4 rq = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.res) rq = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rr, voff_of(m, n) + 32u * g, 0, 0));
            const float4 bj = *reinterpret_cast<const float4*>(sbias + n * 32 + 8 * g + 4 * lh);
            const float bb[4] = {bj.x, bj.y, bj.z, bj.w};
            const float rr4[4] = {rq.x, rq.y, rq.z, rq.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int r = 4 * g + i;
              const float tv = fmaf(cor[m][n][r], a.osc_c, fmaf(acc[m][n][r], a.osc, bb[i]));
              yv[r] = fmaxf(tv, tv * a.act_slope) + rr4[i];
            }
          }
#pragma unroll
          for (int gp = 0; gp < 2; ++gp) {
            float v8[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) v8[t] = yv[8 * gp + t];
            h8 yh, yl;
            split8(v8, yh, yl, mx);
            const uint4* tw = a.tw + (size_t)((n * 2 + gp) * 2) * 64 + lane;
            const h8 wh = __builtin_bit_cast(h8, tw[0]);
            const h8 wl = __builtin_bit_cast(h8, tw[64]);
            pa = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, yh, pa, 0, 0, 0);
            pc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, yh, pc, 0, 0, 0);
            pc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, yl, pc, 0, 0, 0);
          }
        }
        const unsigned po = pix * (unsigned)a.pcp * 4u + (unsigned)(4 * lh) * 4u;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int p0 = 8 * g + 4 * lh;
          float o[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = fmaf(pc[4 * g + i], a.tosc_c, pa[4 * g + i] * a.tosc);
          const unsigned so = (row_ok && p0 < a.pcp) ? po + 32u * g : kOob;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, make_float4(o[0], o[1], o[2], o[3])), ry, so, 0, 0);
        }
      }
      continue;
    }
    // residual: the 4 groups of output tile t+1 are loaded before tile t is finished and stored,
    // so each wait covers loads issued one tile earlier (vmcnt is in order and counts the stores);
    // WM = WN = 2 has no registers for the second set: its 4 loads are waited for together
    constexpr int NTL = WM * WN;
    constexpr bool kResPipe = NTL < 4;
    float4 rv[2][4];
    auto load_res = [&](int t, float4 (&r)[4]) {
      const unsigned vo = voff_of(t / WN, t % WN);
#pragma unroll
      for (int g = 0; g < 4; ++g)
        r[g] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rr, vo + 32u * g, 0, 0));
    };
    if (a.res && kResPipe) load_res(0, rv[0]);
    // kPostPool: strips 0 and 1 of a wave are output rows 2r and 2r+1 and lanes li, li^1 are
    // columns 2c, 2c+1, so each 2x2 window is in one wave: strip 0's values are kept, strip 1
    // adds them with a DPP quad swap, and the even lanes store the pooled pixel (ATen order
    // ((x00 + x01) + x10) + x11, / 4: the same bits as k_avgpool2)
    float keep[POST == kPostPool ? WN : 1][4][4];
    const __amdgpu_buffer_rsrc_t rpool =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.pool, (short)0, (int)a.pool_bytes, kRsrcFlags);
    auto swap1 = [](float x) {  // value of lane li ^ 1 (quad_perm [1, 0, 3, 2])
      return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, false));
    };
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
      const int m = t / WN, n = t % WN;
      if (a.res) {
        if (!kResPipe) load_res(t, rv[t & 1]);
        else if (t + 1 < NTL) load_res(t + 1, rv[(t + 1) & 1]);
      }
      // pair-tap form: the odd taps' products of this lane's output pixel sit in rows 16-31
      // (register groups 2, 3) of the next lane
      float sh[8];
      if (a.pt) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const float bv = fmaf(cor[m][n][8 + r], a.osc_c, acc[m][n][8 + r] * a.osc);
          sh[r] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(((lane + 1) & 63) * 4, __builtin_bit_cast(int, bv)));
        }
      }
      const unsigned vo = voff_of(m, n);
      const bool row_ok = qy0 + wm_ * WM + m < a.Hq && px_ok;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int jl = 8 * g + 4 * lh;       // channel within the N-tile
        const int j0 = (ntw + n) * 32 + jl;  // first of this lane's 4 channels
        const float4 bj = *reinterpret_cast<const float4*>(sbias + (wg_ * WN + n) * 32 + jl);
        const float bb[4] = {bj.x, bj.y, bj.z, bj.w};
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * g + i;
          float tv = fmaf(cor[m][n][r], a.osc_c, fmaf(acc[m][n][r], a.osc, bb[i]));
          if (a.pt && g < 2) tv += sh[r];
          v[i] = fmaxf(tv, tv * a.act_slope);
        }
        if (a.res) {
          const float4 q4 = rv[t & 1][g];
          v[0] += q4.x; v[1] += q4.y; v[2] += q4.z; v[3] += q4.w;
        }
        if constexpr (POST == FVC_POST_EXP) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = j0 + i < a.cout ? expf(v[i]) : 0.f;
        }
        const unsigned so = (row_ok && j0 < a.coutp) ? vo + 32u * g : kOob;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, make_float4(v[0], v[1], v[2], v[3])),
                                               ry, so, 0, 0);
        if constexpr (POST == kPostPool) {
          if (m == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) keep[n][g][i] = v[i];
          } else {
            // pooled values on the even lanes; groups g (even) and g + 1 go out in one store: the
            // odd lane li + 1 takes group g + 1 of its even neighbour (channels 8 further)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float x00 = keep[n][g][i], x10 = v[i];
              keep[n][g][i] = (((x00 + swap1(x00)) + x10) + swap1(x10)) / 4.f;
            }
            if (g & 1) {
              // the swap runs on every lane (a DPP read from a lane switched off by a branch
              // would return 0), then a bitwise select keeps the branch out
              float pv[4];
              const int odd = -(li & 1);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int sw = __builtin_bit_cast(int, swap1(keep[n][g][i]));
                const int ev = __builtin_bit_cast(int, keep[n][g - 1][i]);
                pv[i] = __builtin_bit_cast(float, (sw & odd) | (ev & ~odd));
              }
              const int Hp = a.Hq >> 1, Wp = a.Wq >> 1;
              const int prow = (qy0 + wm_ * WM) >> 1, pcol = (qx0 + li) >> 1;
              const int jp = (ntw + n) * 32 + 8 * (g - 1 + (li & 1)) + 4 * lh;  // this lane's channels
              const bool pok = prow < Hp && pcol < Wp && jp < a.coutp;
              const unsigned po = (((unsigned)b * Hp + prow) * Wp + pcol) * (unsigned)a.coutp * 4u + (unsigned)jp * 4u;
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, make_float4(pv[0], pv[1], pv[2], pv[3])),
                                                     rpool, pok ? po : kOob, 0, 0);
            }
          }
        }
      }
    }
  }
  if (!(mx < 65000.f) && a.ovf) atomicOr(a.ovf, 1);
  finish();
}

// ------------------------------------------------------------------ host-side geometry
// th / nks / wcls / wtotal (fvc_dx::Plan) describe the direct kernel's tile and pack as well
struct X3Cfg : FvcTaps, fvc_dx::Plan {
  int cinp, coutp, ntp, cc, wm, wn, nw, nchunks;
  int pt;     // pair-tap form (16 output channels, stride 1): (ky, even kx) pairs, see X3Args::pt
  int dx;     // stride-2 transposed conv on fvc_deconv_x3.hip (all classes per staged tile, one chunk)
};
static_assert(kMaxTapsX == kFvcMaxTaps, "X3Args and FvcTaps hold the same tap lists");

// LDS A tile: 2*CC/8 planes (hi octets, then lo octets) of ir*ic 16-B pixel entries. The plane
// stride is the pixel count rounded up to 4 mod 16 entries (64 B mod 256 B), so the staging
// writes of consecutive items (octets of one pixel go to different planes) do not collide, while
// a strip read (32 consecutive pixels of one plane, 16 B each) is conflict-free by construction.
static int x3_plane_pix(int ir, int ic) { return ((ir * ic + 15) & ~15) + 4; }
static size_t x3_tile_bytes(int ir, int ic, int cc) { return (size_t)4 * cc * x3_plane_pix(ir, ic); }

// Geometry and tile choice. Returns false for layers the x3 path does not take (cinp % 8 != 0,
// cout <= 4 -> the VALU small-N kernel, > 128 output channels).
static bool x3_cfg(int cin, int cout, int ks, int stride, int transposed, X3Cfg& c) {
  if (cin <= 0 || cout <= 0) return false;
  c.cinp = fvc_rup(cin, 4);
  c.coutp = fvc_rup(cout, 4);
  // cin padded to 4 (cin 2 / 3: mvEncoder conv1, resEncoder conv1) runs as one zero-extended octet:
  // the staging loads 4 channels per pixel and pads the other 4 with zeros, so no widened copy of
  // the input is needed (FVC_X3_CIN4=0 keeps these layers on the fp32 kernels)
  if (c.cinp % 8 && !(c.cinp == 4 && fvc_env_int("FVC_X3_CIN4", 1))) return false;
  // cout <= 4 (N padded to one 32-wide tile): measured faster than the VALU small-N kernel for the
  // 3x3 / 5x5 layers (Warp_net conv6, mvDecoder conv8, resDecoder deconv4), slower for SpyNet's
  // 7x7 16->2 (scripts/conv_micro.py); FVC_X3_SMALLN=0/1 forces either way
  if (c.coutp <= 4) {
    const int sn = fvc_env_int("FVC_X3_SMALLN", -1);
    if (sn == 0 || (sn < 0 && ks > 5)) return false;
  }
  c.ntp = fvc_cdiv(c.coutp, 32);
  if (c.ntp > 4) return false;
  c.pt = (!transposed && stride == 1 && c.coutp == 16 && ks >= 3 && fvc_env_int("FVC_X3_PT", 1)) ? 1 : 0;
  if (!fvc_taps(ks, stride, transposed, c.pt, c)) return false;
  // the all-classes kernel where it takes the layer; its pack is this pack with one channel chunk
  c.dx = fvc_dx::config(c, c.cinp, c.ntp, kFrag, c) ? 1 : 0;
  if (c.dx) {
    c.cc = c.cinp;
    c.nchunks = 1;
    c.nw = 8;
    c.wm = 2;
    c.wn = 2;
    return true;
  }
  // channel chunk: the largest of 32 / 16 / 8 dividing cinp (shrunk below if the two LDS tile
  // buffers do not fit); FVC_X3_CC overrides for experiments
  c.cc = (c.cinp % 32 == 0) ? 32 : ((c.cinp % 16 == 0) ? 16 : 8);
  const int want_cc = fvc_env_int("FVC_X3_CC", 0);
  if ((want_cc == 8 || want_cc == 16 || want_cc == 32) && c.cinp % want_cc == 0) c.cc = want_cc;
  // block shape: 8 waves x 2 strips (16 output rows x 32 columns), 2 waves per SIMD;
  // FVC_X3_WM=1 forces one strip per wave
  c.nw = 8;
  // stride-2 convs: one strip per wave (measured 0.22 vs 0.35 ms on the 544x960 128-channel layer:
  // two strips double the halo rows each staged chunk carries)
  c.wm = fvc_env_int("FVC_X3_WM", (!transposed && stride == 2) ? 1 : 2) == 1 ? 1 : 2;
  // shrink the channel chunk, then the strips per wave, until two tile buffers fit in LDS
  for (;;) {
    c.th = c.nw * c.wm;
    const int ir = (c.th - 1) * c.sin + 1 + (c.dymax - c.dymin);
    const int ic = 31 * c.sin + 1 + (c.dxmax - c.dxmin);
    if (1024 + 2 * x3_tile_bytes(ir, ic, c.cc) <= 160 * 1024) break;
    if (c.cc > 8 && c.cinp % (c.cc / 2) == 0) c.cc /= 2;
    else if (c.wm > 1) c.wm /= 2;
    else return false;
  }
  c.nchunks = c.cinp == 4 ? 1 : c.cinp / c.cc;
  c.wn = 1;
  long long off = 0;
  for (int cl = 0; cl < c.nclass; ++cl) {
    c.nks[cl] = fvc_cdiv(c.ntaps[cl] * (c.cc / 8), 2);
    c.wcls[cl] = off;
    off += (long long)c.nchunks * c.nks[cl] * c.ntp * kFrag;  // kFrag uint4 per (k-step, N-tile)
  }
  c.wtotal = off;
  return true;
}

template <int CC, int WM, int WN, int IOP, int POST, int NWV>
static int x3_launch(const X3Args& a, dim3 grid, size_t lds, hipStream_t s) {
  return fvc_launch(conv_x3_kernel<CC, WM, WN, IOP, POST, NWV>, grid, dim3(NWV * 64), lds, s, a);
}

// exp after the epilogue is only ever taken with an untransformed input (Synthesis_prior_net
// deconv3, synthesis_prior.py:25,57): instantiated for IN_NONE only
template <int CC, int WM, int WN, int NWV = 8>
static int x3_launch_iop(int iop, int post, const X3Args& a, dim3 grid, size_t lds, hipStream_t s) {
  if (post == kPostPool) {  // fused 2x2 pool epilogue: strip pairs per wave (run_x3)
    if constexpr (WM == 2 && WN <= 2)
      return iop == FVC_IN_NONE ? x3_launch<CC, WM, WN, FVC_IN_NONE, kPostPool, NWV>(a, grid, lds, s) : FVC_EINVAL;
    return FVC_EINVAL;
  }
  if (post == kPostTap) {  // fused tap epilogue: every output channel in one wave (run_x3)
    if constexpr ((WM == 2 && WN <= 2) || (WM == 1 && WN == 4))
      return iop == FVC_IN_NONE ? x3_launch<CC, WM, WN, FVC_IN_NONE, kPostTap, NWV>(a, grid, lds, s) : FVC_EINVAL;
    return FVC_EINVAL;
  }
  if (post == FVC_POST_EXP)
    return iop == FVC_IN_NONE ? x3_launch<CC, WM, WN, FVC_IN_NONE, FVC_POST_EXP, NWV>(a, grid, lds, s) : FVC_EINVAL;
  switch (iop) {
    case FVC_IN_NONE: return x3_launch<CC, WM, WN, FVC_IN_NONE, FVC_POST_NONE, NWV>(a, grid, lds, s);
    case FVC_IN_RELU: return x3_launch<CC, WM, WN, FVC_IN_RELU, FVC_POST_NONE, NWV>(a, grid, lds, s);
    case FVC_IN_ABS: return x3_launch<CC, WM, WN, FVC_IN_ABS, FVC_POST_NONE, NWV>(a, grid, lds, s);
    case FVC_IN_ROUND: return x3_launch<CC, WM, WN, FVC_IN_ROUND, FVC_POST_NONE, NWV>(a, grid, lds, s);
  }
  return FVC_EINVAL;
}

// instantiated wave tiles (8 waves, 2 per SIMD, <= 256 registers: scripts/kres.sh):
// WM, WN in {1, 2} or WM = 1, WN = 4
template <int CC>
static int x3_launch_cc(int nwv, int wm, int wn, int iop, int post, const X3Args& a, dim3 grid, size_t lds,
                        hipStream_t s) {
  if (nwv != 8) return FVC_EINVAL;
  if (wm == 2 && wn == 2) return x3_launch_iop<CC, 2, 2>(iop, post, a, grid, lds, s);
  if (wm == 2 && wn == 1) return x3_launch_iop<CC, 2, 1>(iop, post, a, grid, lds, s);
  if (wm == 1 && wn == 2) return x3_launch_iop<CC, 1, 2>(iop, post, a, grid, lds, s);
  if (wm == 1 && wn == 1) return x3_launch_iop<CC, 1, 1>(iop, post, a, grid, lds, s);
  if (wm == 1 && wn == 4) return x3_launch_iop<CC, 1, 4>(iop, post, a, grid, lds, s);
  return FVC_EINVAL;
}

// call for images [b0, b1) alone: x, y, res and pool advance by b0 images of their own sizes
// (ych = channels of the tensor y points to)
static FvcConvCall x3_images(FvcConvCall call, const X3Cfg& c, const X3Args& a, int ych, int b0, int b1) {
  call.batch = b1 - b0;
  call.x += b0 * ((size_t)a.H * a.W * c.cinp);
  call.y += b0 * ((size_t)a.Ho * a.Wo * ych);
  if (call.res) call.res += b0 * ((size_t)a.Ho * a.Wo * c.coutp);
  if (call.pool) call.pool += b0 * ((size_t)(a.Ho / 2) * (a.Wo / 2) * c.coutp);
  return call;
}

// call.tw != null: fused tap epilogue (y receives P [batch][Ho][Wo][pcp], see kPostTap)
static int run_x3(const FvcConvGeom& g, const FvcConvCall& call) {
  const bool tap = call.tw != nullptr, pool = call.pool != nullptr;
  const int batch = call.batch, h = call.h, w = call.w, in_op = call.in_op;
  int post_op = call.post_op;  // the kernel's: kPostTap / kPostPool for the fused forms
  if (!fvc_tail_ok(call.tail)) return FVC_EINVAL;
  X3Cfg c;
  if (!x3_cfg(g.cin, g.cout, g.ksize, g.stride, g.transposed, c)) return FVC_EINVAL;
  if (!call.x || !call.wpack || !call.bias || !call.y || batch <= 0) return FVC_EINVAL;
  if (tap) {
    // every output channel in one wave: N-tiles 1, 2 (2 strips per wave) or 4 (1 strip); the
    // channel chunk (and so the weight pack) stays what x3_cfg chose: fewer strips only shrink LDS
    if (post_op != FVC_POST_NONE || in_op != FVC_IN_NONE || c.ntp == 3 || c.ntp > 4 || call.pcp <= 0 ||
        call.pcp > 32 || (call.pcp & 3) || (c.dx && c.ntp != 4))
      return FVC_EINVAL;
    if (!c.dx) {
      if (c.ntp == 4) c.wm = 1;
      c.th = c.nw * c.wm;
    }
    post_op = kPostTap;
  }
  if (pool) {
    // y and avg_pool2d(y): stride-1 conv, two strips per wave (rows 2r, 2r + 1), one N-group
    if (tap || g.transposed || g.stride != 1 || post_op != FVC_POST_NONE || in_op != FVC_IN_NONE || c.wm != 2 ||
        c.ntp > 2)
      return FVC_EINVAL;
    post_op = kPostPool;
  }
  const int ych = tap ? call.pcp : c.coutp;  // channels of the tensor y points to
  X3Args a;
  a.x = call.x; a.w = (const uint4*)call.wpack; a.bias = call.bias; a.res = call.res; a.y = call.y;
  a.tw = (const uint4*)call.tw; a.pcp = call.pcp;
  a.tosc = call.tosc; a.tosc_c = fvc_lo_scale(call.tosc);
  a.B = batch; a.H = h; a.W = w; a.cinp = c.cinp;
  a.coutp = c.coutp; a.cout = g.cout;
  if (!fvc_out_dims(h, w, g.stride, g.transposed, a.Ho, a.Wo, a.Hq, a.Wq)) return FVC_EINVAL;
  // y and res are addressed through buffer descriptors with 32-bit offsets: split batches whose
  // output tensor reaches 4 GB into launches over sub-batches
  const unsigned long long ybytes = (unsigned long long)batch * a.Ho * a.Wo * ych * 4ull;
  const unsigned long long rbytes = (unsigned long long)batch * a.Ho * a.Wo * a.coutp * 4ull;
  const long long split_env = fvc_env_int("FVC_X3_SPLIT_BYTES", 0);  // tests: force the split path
  const unsigned long long split_at = split_env > 0 ? (unsigned long long)split_env : (1ull << 32) - 4096;
  if (ybytes >= split_at || (call.res && rbytes >= split_at)) {
    if (batch == 1) return FVC_EINVAL;
    // the halves carry the caller's post_op (none in the tap and pool forms), not the kernel's
    const int rc = run_x3(g, x3_images(call, c, a, ych, 0, batch / 2));
    return rc ? rc : run_x3(g, x3_images(call, c, a, ych, batch / 2, batch));
  }
  a.y_bytes = (unsigned)ybytes;
  a.res_bytes = (unsigned)rbytes;
  a.pool = call.pool;
  a.pool_bytes = (unsigned)((unsigned long long)batch * (a.Ho / 2) * (a.Wo / 2) * c.coutp * 4ull);
  // the input is addressed per image (blockIdx.z) through a 32-bit-range descriptor too
  const unsigned long long xbytes = (unsigned long long)h * w * c.cinp * 4ull;
  if (xbytes >= (1ull << 32) - 4096) return FVC_EINVAL;
  a.x_bytes = (unsigned)xbytes;
  a.ovf = call.tail.ovf;
  if (c.dx) return fvc_dx::run(c, c.cinp, c.coutp, c.ntp, g.cout, c, call, a.y_bytes, a.x_bytes);
  a.sin = c.sin; a.sout = c.sout; a.nclass = c.nclass; a.nchunks = c.nchunks; a.ntp = c.ntp;
  a.dymin = c.dymin; a.dxmin = c.dxmin;
  const int th = c.th;
  a.ir = (th - 1) * c.sin + 1 + (c.dymax - c.dymin);
  a.xcd = fvc_env_int("FVC_X3_XCD", 1) ? 1 : 0;
  a.ic = 31 * c.sin + 1 + (c.dxmax - c.dxmin);
  a.pt = c.pt;
  if (c.pt && (tap || pool)) return FVC_EINVAL;
  a.half = c.sin == 2 ? (a.ic + 1) / 2 : 0;
  a.inv_ic = 1.0f / (float)a.ic;
  a.act_slope = fvc_act_slope(call.act);
  a.in_op = in_op; a.act = call.act; a.post_op = post_op;
  a.osc = call.osc;
  a.osc_c = fvc_lo_scale(call.osc);
  for (int cl = 0; cl < 4; ++cl) {
    const bool v = cl < c.nclass;
    a.nks[cl] = v ? c.nks[cl] : 0;
    a.ntaps[cl] = v ? c.ntaps[cl] : 0;
    a.oy0[cl] = v ? c.oy0[cl] : 0;
    a.ox0[cl] = v ? c.ox0[cl] : 0;
    a.wcls[cl] = v ? c.wcls[cl] : 0;
  }
  a.ps = x3_plane_pix(a.ir, a.ic) * 8;
  for (int cl = 0; cl < 4; ++cl)
    for (int t = 0; t <= kMaxTapsX; ++t) {
      int off = 0;
      if (cl < c.nclass && t < c.ntaps[cl]) {
        const int cdy = c.tdy[cl][t] - c.dymin;
        const int cdx = c.tdx[cl][t] - c.dxmin;
        const int cpos = a.half ? ((cdx & 1) * a.half + (cdx >> 1)) : cdx;
        off = (cdy * a.ic + cpos) * 8;
      }
      a.toff[cl][t] = off;
    }
  const size_t lds = 1024 + 2 * x3_tile_bytes(a.ir, a.ic, c.cc);
  const int tiles_x = fvc_cdiv(a.Wq, 32);
  const int tiles_y = fvc_cdiv(a.Hq, th);
  // N-tiles per block: 2 (each staged input element feeds 64 output channels) unless the layer
  // has too few spatial tiles x N-groups to give every CU of the persistent grid some work
  // stride-2 convs (one strip per wave) with 4 N-tiles take all 128 channels per block: the
  // input tile is staged once instead of twice (3x3 s2 128->128 at 544x960: 0.214 -> 0.191 ms)
  int wn = (c.wm == 1 && !g.transposed && g.stride == 2 && c.ntp % 4 == 0) ? 4 : (c.ntp >= 2 ? 2 : 1);
  const int want_wn = (tap || pool) ? c.ntp : fvc_env_int("FVC_X3_WN", 0);
  if (want_wn == 1 || want_wn == 2 || (want_wn == 4 && c.wm == 1)) wn = want_wn;
  while (wn > 1 && c.ntp % wn) wn >>= 1;
  const long long base = (long long)tiles_x * tiles_y * batch * c.nclass;
  if (!want_wn)
    while (wn > 1 && base * (c.ntp / wn) < 2LL * fvc_num_cus()) wn >>= 1;
  if ((tap || pool) && wn != c.ntp) return FVC_EINVAL;
  if (lds > 160 * 1024) return FVC_EINVAL;
  // persistent grid: ~one 8-wave block per CU, each walking a contiguous run of spatial tiles
  const int ncu = fvc_persistent_cus(call.tail.cu_reserve);
  const long long yz = (long long)(c.ntp / wn) * batch;
  long long gx = ((long long)ncu + yz - 1) / yz;  // blocks over all (tile, class) items
  if (gx > (long long)tiles_x * tiles_y * c.nclass) gx = (long long)tiles_x * tiles_y * c.nclass;
  if (gx < 1) gx = 1;
  dim3 grid((unsigned)gx, c.ntp / wn, batch);
  // dynamic schedule when the caller's scratch holds the group counters (FVC_X3_DYN=0: static runs)
  a.sched = fvc_dyn_sched(call.tail.sched, call.tail.sched_len, 1 + (long long)grid.y * grid.z);
  const hipStream_t s = call.tail.stream;
  switch (c.cc) {
    case 8: return x3_launch_cc<8>(c.nw, c.wm, wn, in_op, post_op, a, grid, lds, s);
    case 16: return x3_launch_cc<16>(c.nw, c.wm, wn, in_op, post_op, a, grid, lds, s);
    case 32: return x3_launch_cc<32>(c.nw, c.wm, wn, in_op, post_op, a, grid, lds, s);
  }
  return FVC_EINVAL;
}

}  // namespace

extern "C" {

int fvc_conv_x3_supported(int cin, int cout, int ksize, int stride, int transposed) {
  X3Cfg c;
  return x3_cfg(cin, cout, ksize, stride, transposed, c) ? 1 : 0;
}

int fvc_deconv_x3_all_classes(int cin, int cout, int ksize, int stride) {
  X3Cfg c;
  return x3_cfg(cin, cout, ksize, stride, 1, c) && c.dx ? 1 : 0;
}

// The pack layout the current configuration gives this geometry (a hash of every X3Cfg field the
// pack's fragment order depends on: kernel family, channel chunk, pair-tap form, taps and k-steps
// per class, total size), or 0 when the x3 path does not take the layer. The env switches that
// choose these (FVC_DX, FVC_X3_PT, FVC_X3_CIN4, FVC_X3_CC, FVC_X3_SMALLN) are read at pack AND at
// launch: callers record the id with a pack and compare it before each launch, so a switch
// flipped in between is refused instead of running on a pack of another layout.
unsigned fvc_conv_x3_layout_id(int cin, int cout, int ksize, int stride, int transposed) {
  X3Cfg c;
  if (!x3_cfg(cin, cout, ksize, stride, transposed, c)) return 0u;
  unsigned h = 2166136261u;
  auto mix = [&](long long v) {
    for (int i = 0; i < 8; ++i) {
      h ^= (unsigned)(v >> (8 * i)) & 0xffu;
      h *= 16777619u;
    }
  };
  mix(c.dx);
  mix(c.cc);
  mix(c.pt);
  mix(c.nchunks);
  mix(c.ntp);
  mix(c.nclass);
  for (int cl = 0; cl < c.nclass; ++cl) {
    mix(c.ntaps[cl]);
    mix(c.nks[cl]);
  }
  mix(c.wtotal);
  return h ? h : 1u;
}

size_t fvc_conv_x3_wpack_bytes(int cin, int cout, int ksize, int stride, int transposed) {
  X3Cfg c;
  if (!x3_cfg(cin, cout, ksize, stride, transposed, c)) return 0;
  return (size_t)c.wtotal * 16;
}

int fvc_conv_x3_pack_weight(const float* w, void* wp, float* osc_out, int cin, int cout, int ks,
                            int stride, int transposed) {
  X3Cfg c;
  if (!x3_cfg(cin, cout, ks, stride, transposed, c) || !w || !wp || !osc_out) return FVC_EINVAL;
  const size_t nw = (size_t)cin * cout * ks * ks;
  const int kw = fvc_split_kw_of(w, nw);
  const float sc = ldexpf(1.f, kw);
  *osc_out = ldexpf(1.f, -kw);
  _Float16* out = (_Float16*)wp;
  const int c8n = c.cc / 8;
  for (long long i = 0; i < c.wtotal * 8; ++i) out[i] = (_Float16)0.f;
  for (int cl = 0; cl < c.nclass; ++cl)
    for (int ch = 0; ch < c.nchunks; ++ch)
      for (int q = 0; q < c.nks[cl]; ++q)
        for (int nt = 0; nt < c.ntp; ++nt)
          for (int lane = 0; lane < 64; ++lane) {
            const int li = lane & 31, lh = lane >> 5;
            const int kb = 2 * q + lh;
            const int t = kb / c8n, o = kb % c8n;
            const int j = nt * 32 + li;
            if (t >= c.ntaps[cl] || (!c.pt && j >= cout)) continue;
            const int ky = c.tky[cl][t];
            const int kx = c.tkx[cl][t] + (c.pt && li >= 16 ? 1 : 0);  // pair-tap: rows 16-31 = odd tap
            const int jo = c.pt ? (li & 15) : j;                          // output channel of row li
            if (kx >= ks || jo >= cout) continue;
            const size_t frag = ((((size_t)c.wcls[cl] + (((size_t)ch * c.nks[cl] + q) * c.ntp + nt) * kFrag)) + lane) * 8;
            for (int e = 0; e < 8; ++e) {
              const int ci = ch * c.cc + o * 8 + e;
              if (ci >= cin) continue;
              const float v = (transposed ? w[(((size_t)ci * cout + jo) * ks + ky) * ks + kx]
                                          : w[(((size_t)jo * cin + ci) * ks + ky) * ks + kx]) * sc;
              fvc_split_store(out + frag + e, out + frag + 64 * 8 + e, v);  // planes 0 (lanes 0..63), 1
            }
          }
  return 0;
}

// tap weights for the fused epilogue: w [np][cin] (np = k*k*cout partials of the next layer,
// row t*cout + co), cin = this conv's cout. Layout [k16 block kb][hi|lo][lane] of 16-B fragments;
// lane (li, lh) of block kb holds row li, channels 16kb + 4lh + {0,1,2,3,8,9,10,11} (the
// accumulator order of the producing tile, kPostTap), scaled by 2^kt like the conv packs.
static int x3_tap_blocks(int cin) { return 2 * fvc_cdiv(fvc_rup(cin, 4), 32); }

size_t fvc_x3_tap_wpack_bytes(int np, int cin) {
  if (np <= 0 || np > 32 || cin <= 0 || cin > 128) return 0;
  return (size_t)x3_tap_blocks(cin) * 2 * 64 * 16;
}

int fvc_x3_tap_pack_weight(const float* w, void* wp, float* osc_out, int np, int cin) {
  if (!w || !wp || !osc_out || !fvc_x3_tap_wpack_bytes(np, cin)) return FVC_EINVAL;
  const int kw = fvc_split_kw_of(w, (size_t)np * cin);
  const float sc = ldexpf(1.f, kw);
  *osc_out = ldexpf(1.f, -kw);
  _Float16* out = (_Float16*)wp;
  const int nkb = x3_tap_blocks(cin);
  for (int kb = 0; kb < nkb; ++kb)
    for (int lane = 0; lane < 64; ++lane) {
      const int li = lane & 31, lh = lane >> 5;
      for (int t = 0; t < 8; ++t) {
        const int ci = 16 * kb + (t < 4 ? t : t + 4) + 4 * lh;
        const float v = (li < np && ci < cin) ? w[(size_t)li * cin + ci] * sc : 0.f;
        fvc_split_store(out + ((size_t)(kb * 2 + 0) * 64 + lane) * 8 + t,
                        out + ((size_t)(kb * 2 + 1) * 64 + lane) * 8 + t, v);
      }
    }
  return 0;
}

int fvc_conv_x3_tap_supported(int cin, int cout, int ksize, int stride, int transposed, int pcp) {
  X3Cfg c;
  if (!x3_cfg(cin, cout, ksize, stride, transposed, c) || c.pt || pcp <= 0 || pcp > 32 || (pcp & 3)) return 0;
  if (c.dx) return c.ntp == 4;  // the all-classes kernel's tap form: 1 strip x 4 N-tiles
  const int wm = c.ntp == 4 ? 1 : c.wm;
  return (wm == 2 && c.ntp <= 2) || (wm == 1 && c.ntp == 4);
}

int fvc_conv2d_nhwc_x3_tap(const float* x, const void* wpack, float osc, const float* bias, const float* res,
                           float* P, int batch, int h, int w, int cin, int cout, int ksize, int stride, int act,
                           const void* tap_wpack, float tap_osc, int pcp, int cu_reserve, int* overflow_flag,
                           int* sched, int sched_len, fvc_stream_t stream) {
  if (!tap_wpack || !fvc_conv_x3_tap_supported(cin, cout, ksize, stride, 0, pcp)) return FVC_EINVAL;
  FvcConvCall c{x, wpack, osc, bias, res, P, batch, h, w, {cu_reserve, overflow_flag, sched, sched_len, stream}};
  c.act = act; c.tw = tap_wpack; c.tosc = tap_osc; c.pcp = pcp;
  return run_x3({cin, cout, ksize, stride, 0}, c);
}

int fvc_deconv2d_nhwc_x3_tap(const float* x, const void* wpack, float osc, const float* bias, const float* res,
                             float* P, int batch, int h, int w, int cin, int cout, int ksize, int stride, int act,
                             const void* tap_wpack, float tap_osc, int pcp, int cu_reserve, int* overflow_flag,
                             int* sched, int sched_len, fvc_stream_t stream) {
  if (!tap_wpack || !fvc_conv_x3_tap_supported(cin, cout, ksize, stride, 1, pcp)) return FVC_EINVAL;
  FvcConvCall c{x, wpack, osc, bias, res, P, batch, h, w, {cu_reserve, overflow_flag, sched, sched_len, stream}};
  c.act = act; c.tw = tap_wpack; c.tosc = tap_osc; c.pcp = pcp;
  return run_x3({cin, cout, ksize, stride, 1}, c);
}

int fvc_conv_x3_pool_supported(int cin, int cout, int ksize) {
  X3Cfg c;
  return x3_cfg(cin, cout, ksize, 1, 0, c) && !c.pt && c.wm == 2 && c.ntp <= 2;
}

int fvc_conv2d_nhwc_x3_pool(const float* x, const void* wpack, float osc, const float* bias, const float* res,
                            float* y, float* pool, int batch, int h, int w, int cin, int cout, int ksize, int act,
                            int cu_reserve, int* overflow_flag, int* sched, int sched_len, fvc_stream_t stream) {
  if (!pool || !fvc_conv_x3_pool_supported(cin, cout, ksize)) return FVC_EINVAL;
  FvcConvCall c{x, wpack, osc, bias, res, y, batch, h, w, {cu_reserve, overflow_flag, sched, sched_len, stream}};
  c.act = act; c.pool = pool;
  return run_x3({cin, cout, ksize, 1, 0}, c);
}

int fvc_conv2d_nhwc_x3(const float* x, const void* wpack, float osc, const float* bias,
                       const float* res, float* y, int batch, int h, int w, int cin, int cout,
                       int ksize, int stride, int in_op, int act, int post_op, int cu_reserve,
                       int* overflow_flag, int* sched, int sched_len, fvc_stream_t stream) {
  FvcConvCall c{x, wpack, osc, bias, res, y, batch, h, w, {cu_reserve, overflow_flag, sched, sched_len, stream}};
  c.in_op = in_op; c.act = act; c.post_op = post_op;
  return run_x3({cin, cout, ksize, stride, 0}, c);
}

int fvc_deconv2d_nhwc_x3(const float* x, const void* wpack, float osc, const float* bias,
                         const float* res, float* y, int batch, int h, int w, int cin, int cout,
                         int ksize, int stride, int in_op, int act, int post_op, int cu_reserve,
                         int* overflow_flag, int* sched, int sched_len, fvc_stream_t stream) {
  FvcConvCall c{x, wpack, osc, bias, res, y, batch, h, w, {cu_reserve, overflow_flag, sched, sched_len, stream}};
  c.in_op = in_op; c.act = act; c.post_op = post_op;
  return run_x3({cin, cout, ksize, stride, 1}, c);
}

}  // extern "C"
