// Host-memory check of the split-precision conv entry points' argument validation: the rejection
// rows of tests/test_abi.py (test_conv_entry_points_reject_bad_arguments) as a stand-alone program,
// to be linked against host objects built with AddressSanitizer / UBSan. Every row is refused
// before anything is launched, so it runs on the CPU; no device is needed.
//
// The sanitizers cover host code only (-Xarch_host); the device code is built as in the product:
//
//   cd fastvideocodec_amd/csrc && S="-Xarch_host -fsanitize=address,undefined"
//   F="--offload-arch=gfx950 -O3 -g -std=c++17 -fPIC -Wno-unused-result $S"
//   for f in fvc_conv_x3 fvc_deconv_x3 fvc_conv_wino fvc_conv_wr7; do hipcc $F -c $f.hip -o /tmp/$f.o; done
//   clang++ -std=c++17 -g -fsanitize=address,undefined -c ../../scripts/abi_reject.cpp -o /tmp/abi_reject.o
//   hipcc --offload-arch=gfx950 $S /tmp/fvc_*.o /tmp/abi_reject.o -o /tmp/abi_reject
//   /tmp/abi_reject        # prints "N rows, 0 not rejected"
#include <stdio.h>

#include "../include/fvc.h"

static int rows = 0, bad = 0;
#define REJECTED(call)                                         \
  do {                                                         \
    const int r__ = (call);                                    \
    ++rows;                                                    \
    if (r__ != FVC_EINVAL) {                                   \
      ++bad;                                                   \
      printf("not rejected (status %d): %s\n", r__, #call);    \
    }                                                          \
  } while (0)

int main() {
  static float buf[16];  // every pointer: validation never dereferences one
  static int flag[4];
  float* const p = buf;
  int* const q = flag;
  const fvc_stream_t st = nullptr;
  for (int t = 0; t < 2; ++t) {  // the launch tail: cu_reserve = -1, then sched_len = -1
    const int cu = t == 0 ? -1 : 0, sl = t == 0 ? 4 : -1;
    REJECTED(fvc_conv2d_nhwc_x3(p, p, 1.f, p, nullptr, p, 1, 8, 8, 64, 64, 3, 1, 0, 0, 0, cu, q, q, sl, st));
    REJECTED(fvc_deconv2d_nhwc_x3(p, p, 1.f, p, nullptr, p, 1, 8, 8, 128, 128, 3, 2, 0, 0, 0, cu, q, q, sl, st));
    REJECTED(fvc_conv2d_nhwc_x3_pool(p, p, 1.f, p, nullptr, p, p, 1, 8, 8, 64, 64, 3, 0, cu, q, q, sl, st));
    REJECTED(fvc_conv2d_nhwc_x3_tap(p, p, 1.f, p, nullptr, p, 1, 8, 8, 64, 64, 3, 1, 0, p, 1.f, 28, cu, q, q, sl, st));
    REJECTED(fvc_conv2d_nhwc_wino(p, p, 1.f, p, nullptr, p, nullptr, 1, 8, 8, 0, 0, cu, q, q, sl, st));
    REJECTED(fvc_conv2d_nhwc_wr7(p, 32, p, 2, 1.f, p, p, 32, 1, 8, 8, 0, 0, cu, q, q, sl, st));
  }
  // x3: null x, null wpack, null y, batch = 0
  REJECTED(fvc_conv2d_nhwc_x3(nullptr, p, 1.f, p, nullptr, p, 1, 8, 8, 64, 64, 3, 1, 0, 0, 0, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_x3(p, nullptr, 1.f, p, nullptr, p, 1, 8, 8, 64, 64, 3, 1, 0, 0, 0, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_x3(p, p, 1.f, p, nullptr, nullptr, 1, 8, 8, 64, 64, 3, 1, 0, 0, 0, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_x3(p, p, 1.f, p, nullptr, p, 0, 8, 8, 64, 64, 3, 1, 0, 0, 0, 0, q, q, 4, st));
  // x3_tap: null tap pack, pcp = 36, pcp = 6, a 96-channel producer (three N-tiles)
  REJECTED(fvc_conv2d_nhwc_x3_tap(p, p, 1.f, p, nullptr, p, 1, 8, 8, 64, 64, 3, 1, 0, nullptr, 1.f, 28, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_x3_tap(p, p, 1.f, p, nullptr, p, 1, 8, 8, 64, 64, 3, 1, 0, p, 1.f, 36, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_x3_tap(p, p, 1.f, p, nullptr, p, 1, 8, 8, 64, 64, 3, 1, 0, p, 1.f, 6, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_x3_tap(p, p, 1.f, p, nullptr, p, 1, 8, 8, 64, 96, 3, 1, 0, p, 1.f, 28, 0, q, q, 4, st));
  // x3_pool: null pool, a 128 -> 128 layer (four N-tiles)
  REJECTED(fvc_conv2d_nhwc_x3_pool(p, p, 1.f, p, nullptr, p, nullptr, 1, 8, 8, 64, 64, 3, 0, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_x3_pool(p, p, 1.f, p, nullptr, p, p, 1, 8, 8, 128, 128, 3, 0, 0, q, q, 4, st));
  // wino: in_op = FVC_IN_ABS, act = 7; wino_tap: pcp = 0; wino_up: odd h, null low; wino128: null osc4
  REJECTED(fvc_conv2d_nhwc_wino(p, p, 1.f, p, nullptr, p, nullptr, 1, 8, 8, FVC_IN_ABS, 0, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_wino(p, p, 1.f, p, nullptr, p, nullptr, 1, 8, 8, 0, 7, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_wino_tap(p, p, 1.f, p, nullptr, p, 1, 8, 8, 0, p, 1.f, 0, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_wino_up(p, p, p, p, 1.f, p, p, 1, 7, 8, 0, 0, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_wino_up(p, nullptr, p, p, 1.f, p, p, 1, 8, 8, 0, 0, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_wino128(p, p, nullptr, p, p, 1, 8, 8, 0, 0, 0, q, q, 4, st));
  // wr7: mode = 3, nt = 3, null bias with mode 0
  REJECTED(fvc_conv2d_nhwc_wr7(p, 32, p, 2, 1.f, p, p, 32, 1, 8, 8, 3, 0, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_wr7(p, 32, p, 3, 1.f, p, p, 32, 1, 8, 8, 0, 0, 0, q, q, 4, st));
  REJECTED(fvc_conv2d_nhwc_wr7(p, 32, p, 2, 1.f, nullptr, p, 32, 1, 8, 8, 0, 0, 0, q, q, 4, st));
  printf("%d rows, %d not rejected\n", rows, bad);
  return bad ? 1 : 0;
}
