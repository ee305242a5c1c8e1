// The tap geometry of a conv or a strided transposed conv, defined once for every weight pack and
// launch plan (fvc_conv.hip, fvc_conv_x3.hip, fvc_deconv_x3.hip): encoder and decoder stay
// bit-exact only while all of them agree on it. Host-only, plain C++ (no HIP runtime needed).
//
// A conv is one class of ks x ks taps, input offset (ky - pad, kx - pad), input step `stride`.
// A transposed conv with stride s (padding ks / 2, output_padding s - 1) splits into s x s stride-1
// convs, one per output parity (py, px), over disjoint tap subsets: tap (ky, kx) belongs to the
// class with (py + pad - ky) % s == 0 and reads input row q + (py + pad - ky) / s for output row
// s q + py (columns alike).
#pragma once

constexpr int kFvcMaxTaps = 49;

struct FvcTaps {
  int nclass, sin, sout;         // parity classes; input step; output step
  int ntaps[4], oy0[4], ox0[4];  // per class: taps, output parity
  int tky[4][kFvcMaxTaps], tkx[4][kFvcMaxTaps];  // kernel tap (ky, kx)
  int tdy[4][kFvcMaxTaps], tdx[4][kFvcMaxTaps];  // its input offset
  int dymin, dymax, dxmin, dxmax;                // offset range over all classes
};

static inline int fvc_floordiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }

// false unless ks in {1, 3, 5, 7} and stride in {1, 2}. pair_tap (convs only): list every second
// kx -- one entry stands for the pair (ky, kx), (ky, kx + 1) of the x3 pair-tap form.
static inline bool fvc_taps(int ks, int stride, int transposed, int pair_tap, FvcTaps& t) {
  if ((ks != 1 && ks != 3 && ks != 5 && ks != 7) || (stride != 1 && stride != 2)) return false;
  const int pad = ks / 2;
  for (int cl = 0; cl < 4; ++cl) t.ntaps[cl] = t.oy0[cl] = t.ox0[cl] = 0;
  if (!transposed) {
    t.nclass = 1;
    t.sin = stride;
    t.sout = 1;
    for (int ky = 0; ky < ks; ++ky)
      for (int kx = 0; kx < ks; kx += pair_tap ? 2 : 1) {
        const int i = t.ntaps[0]++;
        t.tky[0][i] = ky; t.tkx[0][i] = kx;
        t.tdy[0][i] = ky - pad; t.tdx[0][i] = kx - pad;
      }
  } else {
    t.nclass = stride * stride;
    t.sin = 1;
    t.sout = stride;
    for (int py = 0; py < stride; ++py)
      for (int px = 0; px < stride; ++px) {
        const int cl = py * stride + px;
        t.oy0[cl] = py; t.ox0[cl] = px;
        for (int ky = 0; ky < ks; ++ky) {
          if (((py + pad - ky) % stride + stride) % stride) continue;
          for (int kx = 0; kx < ks; ++kx) {
            if (((px + pad - kx) % stride + stride) % stride) continue;
            const int i = t.ntaps[cl]++;
            t.tky[cl][i] = ky; t.tkx[cl][i] = kx;
            t.tdy[cl][i] = fvc_floordiv(py + pad - ky, stride);
            t.tdx[cl][i] = fvc_floordiv(px + pad - kx, stride);
          }
        }
      }
  }
  t.dymin = t.dxmin = 1 << 20;
  t.dymax = t.dxmax = -(1 << 20);
  for (int cl = 0; cl < t.nclass; ++cl)
    for (int i = 0; i < t.ntaps[cl]; ++i) {
      t.dymin = t.tdy[cl][i] < t.dymin ? t.tdy[cl][i] : t.dymin;
      t.dymax = t.tdy[cl][i] > t.dymax ? t.tdy[cl][i] : t.dymax;
      t.dxmin = t.tdx[cl][i] < t.dxmin ? t.tdx[cl][i] : t.dxmin;
      t.dxmax = t.tdx[cl][i] > t.dxmax ? t.tdx[cl][i] : t.dxmax;
    }
  return true;
}

// Output size (Ho, Wo) of an h x w input and the size (Hq, Wq) of one parity class of it (the
// whole output for a conv, the input size for a transposed conv). false for an empty input and
// for a stride-2 conv of an odd-sized one.
static inline bool fvc_out_dims(int h, int w, int stride, int transposed, int& Ho, int& Wo, int& Hq, int& Wq) {
  if (h <= 0 || w <= 0) return false;
  if (!transposed) {
    if (stride == 2 && ((h & 1) || (w & 1))) return false;
    Ho = Hq = h / stride;
    Wo = Wq = w / stride;
  } else {
    Ho = h * stride; Wo = w * stride;
    Hq = h; Wq = w;
  }
  return true;
}
