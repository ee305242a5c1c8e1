// Internal interface (not exported) between fvc_conv_x3.hip's host dispatcher and the
// all-classes transposed-conv kernel of fvc_deconv_x3.hip, which plans its own launches.
#pragma once
#include "fvc_common.h"
#include "fvc_taps.h"

namespace fvc_dx {

// Does the all-classes kernel take this stride-2 transposed conv (64 / 96 / 128 input channels,
// ntp = 2 or 4 N-tiles of 32 output channels, FVC_DX not 0)? Then th = input rows per work item and
// the layout of its weight pack -- the x3 pack with one channel chunk, frag uint4 per (k-step,
// N-tile): k-steps nks[] and uint4 offset wcls[] of each class, wtotal uint4 in all.
__attribute__((visibility("hidden"))) bool config(const FvcTaps& t, int cinp, int ntp, int frag, int& th, int nks[4],
                                                  long long wcls[4], long long& wtotal);

// One launch of a layer config() took, th / nks / wcls as it gave them. tw != null: the tap form
// (y receives the next layer's partials [batch][2h][2w][pcp]; needs ntp = 4 and no residual).
__attribute__((visibility("hidden"))) int run(const FvcTaps& t, int cinp, int coutp, int ntp, int th, const int nks[4],
                                              const long long wcls[4], const float* x, const void* wpack, float osc,
                                              const float* bias, const float* res, float* y, int batch, int h, int w,
                                              int cout, int in_op, int act, int post_op, int cu_reserve, int* ovf,
                                              int* sched, int sched_len, hipStream_t s, const void* tw, float tosc,
                                              int pcp, unsigned y_bytes, unsigned x_bytes);

}  // namespace fvc_dx
