// Internal interface (not exported) between fvc_conv_x3.hip's host dispatcher and the
// all-classes transposed-conv kernel of fvc_deconv_x3.hip, which plans its own launches.
#pragma once
#include "fvc_split.h"
#include "fvc_taps.h"

namespace fvc_dx {

// th = input rows per work item, and the layout of the weight pack -- the x3 pack with one channel
// chunk, frag uint4 per (k-step, N-tile): k-steps nks[] and uint4 offset wcls[] of each class,
// wtotal uint4 in all.
struct Plan {
  int th, nks[4];
  long long wcls[4], wtotal;
};

// Does the all-classes kernel take this stride-2 transposed conv (64 / 96 / 128 input channels,
// ntp = 2 or 4 N-tiles of 32 output channels, FVC_DX not 0)? Then p is its plan.
__attribute__((visibility("hidden"))) bool config(const FvcTaps& t, int cinp, int ntp, int frag, Plan& p);

// One launch of a layer config() took, p as it gave it. c.tw != null: the tap form (c.y receives
// the next layer's partials [batch][2h][2w][pcp]; needs ntp = 4 and no residual). c.pool is not
// read. y_bytes / x_bytes: the descriptor ranges of c.y and of one image of c.x.
__attribute__((visibility("hidden"))) int run(const FvcTaps& t, int cinp, int coutp, int ntp, int cout, const Plan& p,
                                              const FvcConvCall& c, unsigned y_bytes, unsigned x_bytes);

}  // namespace fvc_dx
