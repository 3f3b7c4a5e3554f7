// The bilinear scatter taps of the forward splat (video-interpolation/my_utils/softsplat.py:8-52) and the atomic float add its
// kernels use: shared by the loss operators (flowloss.hip) and the frame synthesis (flowsynth.hip).
#pragma once
#include "common.h"

namespace sininn {

__device__ __forceinline__ void atomic_add_f32(float* p, float v) { unsafeAtomicAdd(p, v); }

struct SplatTaps {
  int nwx, nwy;
  float nw, ne, sw, se;
  bool vnw, vne, vsw, vse;
};

__device__ __forceinline__ SplatTaps splat_taps(float ox, float oy, int H, int W) {
  SplatTaps t;
  t.nwx = (int)floorf(ox); t.nwy = (int)floorf(oy);
  const float sex = (float)(t.nwx + 1), sey = (float)(t.nwy + 1), nwx = (float)t.nwx, nwy = (float)t.nwy;
  t.nw = (sex - ox) * (sey - oy);
  t.ne = (ox - nwx) * (sey - oy);
  t.sw = (sex - ox) * (oy - nwy);
  t.se = (ox - nwx) * (oy - nwy);
  const bool x0 = t.nwx >= 0 && t.nwx < W, x1 = t.nwx + 1 >= 0 && t.nwx + 1 < W;
  const bool y0 = t.nwy >= 0 && t.nwy < H, y1 = t.nwy + 1 >= 0 && t.nwy + 1 < H;
  t.vnw = x0 && y0; t.vne = x1 && y0; t.vsw = x0 && y1; t.vse = x1 && y1;
  return t;
}

}  // namespace sininn
