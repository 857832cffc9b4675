// Host-side helpers shared by the convolution files (conv_igemm.hip, conv_halo.hip, conv_wgrad.hip): the geometry of
// a "same" conv, the tap word, the magic divisor, the shape rules and the epilogue copy — one definition of each.
#pragma once
#include "common.h"

// "same" convolutions only.  For k = 3 the padding IS the dilation, exactly as conv3x3_group builds them
// (padding = dilation, models/utils/layers.py:20-32): pad = d means taps at (-d, 0, +d)
static inline int conv_dil(int k, int pad) { return k == 3 ? pad : 1; }
static inline int conv_out_sz(int H, int k, int stride, int pad) {
  return (H + 2 * pad - (conv_dil(k, pad) * (k - 1) + 1)) / stride + 1;
}

// tap word of the kernels' tap lists: input pixel offset (dh, dw) and the weight tap index
static inline int pack_tap(int dh, int dw, int widx) { return (dh + 64) | ((dw + 64) << 8) | (widx << 16); }

// n / d for 0 <= n < 2^31 as umulhi(n, mul) >> shr (mul == 0 encodes d == 1): the row -> (image, y, x) split of every
// loader row and every epilogue pixel costs 2 multiplies instead of two ~35-instruction integer divisions.
static inline void fast_div_init(unsigned d, unsigned* mul, unsigned* shr) {
  if (d <= 1) { *mul = 0; *shr = 0; return; }
  unsigned lg = 0;
  while ((1ull << lg) < d) ++lg;             // ceil(log2(d))
  const unsigned p = 31 + lg;
  *mul = (unsigned)(((1ull << p) + d - 1) / d);
  *shr = p - 32;
}

// kernel size, stride, padding and channel counts every conv entry point accepts (forward, input and weight gradient)
static inline int conv_check_rules(int k, int stride, int pad, int Cin, int Cout) {
  TDN_CHECK(k == 1 || k == 3, "kernel size %d not supported (1 or 3)", k);
  TDN_CHECK(stride == 1 || stride == 2, "stride %d not supported (1 or 2)", stride);
  TDN_CHECK((k == 1 && pad == 0) || (k == 3 && pad >= 1 && pad <= 32),
            "pad %d not supported for k=%d (1x1: 0; 3x3: pad = dilation in 1..32)", pad, k);
  TDN_CHECK(Cin % 64 == 0 && Cout % 64 == 0, "channels must be multiples of 64 (Cin=%d Cout=%d)", Cin, Cout);
  return 0;
}

// tdn_epilogue -> the epilogue fields of a kernel parameter struct (GemmParams, HaloParams), validated against the
// output size.  The halo entry points are handed the epilogue conv_igemm.hip has already passed through here for the
// same output size, so their second pass cannot fail.
template <class Params>
static int conv_fill_epilogue(Params& p, const tdn_epilogue* ep, int Hout, int Wout) {
  p.scale = nullptr; p.shift = nullptr; p.addend = nullptr; p.mask = nullptr;
  p.addend_mode = TDN_ADD_NONE; p.addend_h = 0; p.addend_w = 0; p.relu = 0; p.out_f32 = 0;
  if (!ep) return 0;
  p.out_f32 = ep->out_f32 ? 1 : 0;
  p.scale = ep->scale;
  p.shift = ep->shift;
  p.relu = ep->relu;
  p.mask = (const bf16_t*)ep->mask_src;
  if (ep->addend_mode != TDN_ADD_NONE) {
    TDN_CHECK(ep->addend != nullptr, "epilogue: addend_mode %d with NULL addend", ep->addend_mode);
    p.addend = (const bf16_t*)ep->addend;
    p.addend_mode = ep->addend_mode;
    p.addend_h = ep->addend_h;
    p.addend_w = ep->addend_w;
    if (ep->addend_mode == TDN_ADD_UP2X)
      TDN_CHECK(ep->addend_h * 2 == Hout && ep->addend_w * 2 == Wout,
                "epilogue UP2X: addend %dx%d is not half of output %dx%d", ep->addend_h, ep->addend_w, Hout, Wout);
    if (ep->addend_mode == TDN_ADD_SUMPOOL2)
      TDN_CHECK(ep->addend_h == Hout * 2 && ep->addend_w == Wout * 2,
                "epilogue SUMPOOL2: addend %dx%d is not twice the output %dx%d", ep->addend_h, ep->addend_w, Hout, Wout);
    TDN_CHECK(ep->addend_mode >= 0 && ep->addend_mode <= 3, "epilogue: bad addend_mode %d", ep->addend_mode);
  }
  return 0;
}
