// Per-frame reconstruction digest (include/fvc.h, fvc_frame_digest_f32): a position-dependent sum
// of 64-bit integers over a frame's float32 bit patterns, so the result is exact and independent of
// the order of addition. A streaming kernel shaped like k_sse_u8 (fvc_pixfmt.hip): 16-byte loads
// over the aligned body of each frame, single words for a misaligned head or tail, a grid-stride
// loop under a capped grid with blockIdx.y as the frame, and one integer atomic per block. Atomics
// on one word retire at about 90 per microsecond whatever the grid, so the blocks are few and large
// (1024 lanes, 512 of them in all: two per CU): a 2048 x 256-lane grid per frame spent its time there.
#include "fvc_common.h"

namespace {

constexpr int kBlk = 1024;
constexpr unsigned kMaxBlocks = 512;  // over all frames of a call: the grid-stride loop walks the rest

// the splitmix64 finaliser of (index << 32 | word) + the golden-ratio increment
__device__ __forceinline__ unsigned long long mix(uint32_t i, uint32_t w) {
  unsigned long long z = (((unsigned long long)i << 32) | w) + 0x9e3779b97f4a7c15ull;
  z ^= z >> 30;
  z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27;
  z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

// n < 2^32 (checked by the host), so every word index fits the 32 bits the definition gives it.
__global__ void __launch_bounds__(kBlk)
    k_frame_digest(const uint32_t* __restrict__ x, size_t n, unsigned long long* __restrict__ out) {
  const uint32_t* w = x + (size_t)blockIdx.y * n;
  const size_t tid = blockIdx.x * (size_t)kBlk + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * kBlk;
  // words before the first 16-byte boundary of this frame (0..3; frames of a batch differ when n % 4)
  size_t head = ((16 - ((uintptr_t)w & 15)) & 15) >> 2;
  if (head > n) head = n;
  const size_t nv = (n - head) / 4;
  const uint4* w4 = reinterpret_cast<const uint4*>(w + head);
  unsigned long long acc = 0;
#pragma unroll 2  // 47 VGPRs: 8 waves per SIMD, so both of a CU's blocks are resident (unroll 4 takes 66)
  for (size_t i = tid; i < nv; i += nth) {
    const uint4 p = w4[i];
    const uint32_t k = (uint32_t)(head + 4 * i);
    acc += mix(k, p.x) + mix(k + 1, p.y) + mix(k + 2, p.z) + mix(k + 3, p.w);
  }
  for (size_t i = head + 4 * nv + tid; i < n; i += nth) acc += mix((uint32_t)i, w[i]);
  if (tid < head) acc += mix((uint32_t)tid, w[tid]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ unsigned long long part[kBlk / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < kBlk / 64; ++k) s += part[k];
    atomicAdd(out + blockIdx.y, s);
  }
}

}  // namespace

extern "C" {

int fvc_frame_digest_f32(const float* x, int batch, size_t n, uint64_t* out, fvc_stream_t s) {
  if (!x || !out || batch <= 0 || batch > 65535 || n == 0 || n >= ((size_t)1 << 32)) return FVC_EINVAL;
  if ((uintptr_t)x & 3) return FVC_EINVAL;
  hipError_t e = hipMemsetAsync(out, 0, (size_t)batch * sizeof(uint64_t), (hipStream_t)s);
  if (e != hipSuccess) return -(int)e;
  // one 16-byte word per lane and pass; at most kMaxBlocks / batch (and at least one) blocks a frame
  const unsigned blocks = fvc_blocks(n / 4, kBlk, kMaxBlocks / (unsigned)batch);
  hipLaunchKernelGGL(k_frame_digest, dim3(blocks, (unsigned)batch), dim3(kBlk), 0, (hipStream_t)s,
                     reinterpret_cast<const uint32_t*>(x), n, reinterpret_cast<unsigned long long*>(out));
  FVC_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
