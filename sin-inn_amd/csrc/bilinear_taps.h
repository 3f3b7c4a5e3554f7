// The four-tap bilinear footprint, once: a pixel displaced by a flow touches the four integer pixels around a real-valued
// coordinate.  Everything the photometric and synthesis kernels share about that footprint lives here:
//   * atomic_add_f32, SplatTaps, splat_taps   the forward splat's scatter taps (video-interpolation/my_utils/softsplat.py:8-52)
//   * resample2d_coord                        the Resample2d sampling coordinate (my_utils/resample2d.py:52-72)
//   * BilinearTaps, bilinear_taps             floor / fraction / the four weights of a gather
//   * tap_inside                              the in-frame predicate of one tap
//   * TapMerge, tap_merge_plan, tap_merge     the wave neighbour merge of the scatters
//   * tap_window_zero, tap_window_flush       the LDS accumulation window of the tiled scatters
//   * frame_byte                              the byte rule of every u8 frame
// Every function is inlined into its caller; none carries an `fp contract` pragma (each call site keeps the contraction it is
// compiled with) and none guards a coordinate: a caller that may see a non-finite or huge one tests it BEFORE bilinear_taps /
// splat_taps convert it to int.
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

// Where Resample2d reads for output pixel (x, y) displaced by (fx, fy): grid = (coords + flow) / (W - 1, H - 1) * 2 - 1, sampled
// with align_corners = False (quirk C-18 kept).  On an axis of length 1 the coordinate is infinite (or 0 / 0).
__device__ __forceinline__ void resample2d_coord(int x, int y, float fx, float fy, int H, int W, float& ix, float& iy) {
  const float gxn = (x + fx) / (float)(W - 1) * 2.f - 1.f, gyn = (y + fy) / (float)(H - 1) * 2.f - 1.f;
  ix = ((gxn + 1.f) * W - 1.f) * 0.5f; iy = ((gyn + 1.f) * H - 1.f) * 0.5f;
}

// The gather footprint of a sampling coordinate: north-west tap (y0, x0), weights wy0 / wy1 for rows y0 / y0 + 1 and wx0 / wx1 for
// columns x0 / x0 + 1.  The coordinate must be finite and below 2^31 in size for the float -> int conversion to be defined.
struct BilinearTaps {
  int x0, y0;
  float wx0, wx1, wy0, wy1;
};

__device__ __forceinline__ BilinearTaps bilinear_taps(float ix, float iy) {
  BilinearTaps t;
  const float flx = floorf(ix), fly = floorf(iy);
  t.x0 = (int)flx; t.y0 = (int)fly;
  t.wx1 = ix - flx; t.wy1 = iy - fly; t.wx0 = 1.f - t.wx1; t.wy0 = 1.f - t.wy1;
  return t;
}

__device__ __forceinline__ bool tap_inside(int yy, int xx, int H, int W) { return yy >= 0 && yy < H && xx >= 0 && xx < W; }

// ---- the wave neighbour merge ----------------------------------------------------------------------------------------------------
// A block is a tile of TAP_TILE_X-pixel rows, one lane per pixel, so a wave is two tile rows: lanes 0..31 one row, lanes 32..63 the
// row below it.  For a locally smooth flow the footprints of neighbouring pixels coincide: the south taps (y0 + 1) of a pixel are
// the north taps (y0) of the pixel below it, its east taps (x0 + 1) the west taps (x0) of its right neighbour.  The contributions
// are summed across lanes first, so an interior pixel issues ONE atomic per channel instead of four, and every lane then adds to a
// different address (no same-address serialisation inside the wave).  A merged value lands where the receiving lane's own tap of
// that slot lands: same address, same validity.
constexpr int TAP_TILE_X = 32;

struct TapMerge {
  bool give_h, give_v, take_h, take_v;    // hand the east / south taps to the neighbour, receive the neighbour's as west / north
};

// valid: this lane has a footprint at all; (x0, y0) its north-west tap.  Wave-wide: every shuffle is executed by all 64 lanes before
// anything is combined (no short-circuit around a cross-lane read), so call it from wave-uniform control flow only.
template <int TILE_X>
__device__ __forceinline__ TapMerge tap_merge_plan(bool valid, int x0, int y0) {
  static_assert(TILE_X == TAP_TILE_X && 2 * TAP_TILE_X == 64, "the lane merges assume 32-pixel tile rows, two to a wave");
  const int lane = threadIdx.x & 63;
  const int vi = valid ? 1 : 0;
  const int v_r = __shfl_down(vi, 1), x0_r = __shfl_down(x0, 1), y0_r = __shfl_down(y0, 1);
  const int v_d = __shfl_down(vi, 32), x0_d = __shfl_down(x0, 32), y0_d = __shfl_down(y0, 32);
  TapMerge m;
  m.give_h = valid && (lane & 31) != 31 && v_r != 0 && x0_r == x0 + 1 && y0_r == y0;
  m.give_v = valid && lane < 32 && v_d != 0 && x0_d == x0 && y0_d == y0 + 1;
  const int gh_l = __shfl_up(m.give_h ? 1 : 0, 1), gv_u = __shfl_up(m.give_v ? 1 : 0, 32);
  m.take_h = (lane & 31) != 0 && gh_l != 0;
  m.take_v = lane >= 32 && gv_u != 0;
  return m;
}

// The four contributions of one channel, north/south = y0 / y0 + 1, west/east = x0 / x0 + 1; zero in a lane without a footprint.
// Wave-wide like the plan.
__device__ __forceinline__ void tap_merge(const TapMerge& m, float& nw, float& ne, float& sw, float& se) {
  const float rsw = __shfl_up(sw, 32), rse = __shfl_up(se, 32);
  if (m.take_v) { nw += rsw; ne += rse; }
  if (m.give_v) { sw = 0.f; se = 0.f; }
  const float sne = __shfl_up(ne, 1), sse = __shfl_up(se, 1);
  if (m.take_h) { nw += sne; sw += sse; }
  if (m.give_h) { ne = 0.f; se = 0.f; }
}

// ---- the LDS accumulation window -------------------------------------------------------------------------------------------------
// win[channels][WY][WX]: the block's tile plus R pixels all round, for cc channels at a time.  Zeroed, filled with LDS atomics by the
// kernel, then flushed once with row-contiguous global atomics.  The caller puts a __syncthreads() after each of the three steps.
// `stride` is the block's thread count (as the kernel names it: a constant or blockDim.x).
__device__ __forceinline__ void tap_window_zero(float* win, int n, int stride) {
  for (int e = threadIdx.x; e < n; e += stride) win[e] = 0.f;
}

// dst: channel 0 of this pass in the destination image; (by0, bx0) the tile's first pixel; add(float*, float) the kernel's atomic.
template <int WY, int WX, int R, class Add>
__device__ __forceinline__ void tap_window_flush(const float* win, int cc, int by0, int bx0, int H, int W, float* dst, int stride,
                                                 Add add) {
  const int64_t HW = (int64_t)H * W;
  for (int e = threadIdx.x; e < cc * WY * WX; e += stride) {
    const float v = win[e];
    if (v != 0.f) {
      const int c = e / (WY * WX), q = e % (WY * WX);
      const int gy = by0 - R + q / WX, gx = bx0 - R + q % WX;
      if (tap_inside(gy, gx, H, W)) add(dst + c * HW + (int64_t)gy * W + gx, v);
    }
  }
}

// The byte of a frame value in [0, 1]: clamp(round-half-even(255 v), 0, 255), the product rounded once; NaN gives 0.
__device__ __forceinline__ float frame_byte(float v) { return fminf(fmaxf(rintf(__fmul_rn(v, 255.f)), 0.f), 255.f); }

}  // namespace sininn
