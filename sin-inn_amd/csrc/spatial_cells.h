// The map from a point's coordinates to the cells of a spatial controller's grid (progressive_controller.py:620-668, interpolate_):
// shared by the flow-network kernels (flownet.hip: the per-point mask) and the trainer's error stash (flowtrain.hip: the loss log).
// Internal linkage, like flownet_tile.h: each file compiles its own copy.
#pragma once
#include "flownet_tile.h"

namespace sininn {

namespace {

constexpr int FN_DOM = 3;           // progressive: the raw coordinates lead the encoded features (two of them at domain_dim = 2)
constexpr int FN_GW = 512 + FN_DOM;  // spatial: floats per row of the mask grid and of the W1 it goes with

// spatial: the mask grid and the map from a coordinate to its cell
struct Spatial {
  const float* grid;       // [res^3][FN_GW]
  int res;
  float span;              // max(res - 2, 1)
  float centre[3], scale[3];
};

struct Corners {
  float w[8];              // (a_t a_y) a_x of corner c: bit 2 of c chooses t's upper index, bit 1 y's, bit 0 x's
  int row[8];              // FN_GW * (i_t + i_y res + i_x res^2), indices clamped to the grid
};

// interpolate_ of the reference in fp32, one rounding per operation as torch makes them: floor and ceil decide as they do there
__device__ __forceinline__ Corners corners_of(const Spatial& sp, const Coord c) {
#pragma clang fp contract(off)
  const float x[3] = {c.t, c.y, c.x};
  float a[3][2];
  int i[3][2];
  const float top = (float)(sp.res - 1);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float xs = (x[d] - sp.centre[d]) * sp.scale[d];
    const float u = ((xs + 1.f) * 0.5f) * sp.span + 0.5f;
    const float f0 = floorf(u), f1 = ceilf(u + 1e-6f);
    a[d][0] = f1 - u;
    a[d][1] = u - f0;
    i[d][0] = (int)fminf(fmaxf(f0, 0.f), top);         // a NaN goes to cell 0
    i[d][1] = (int)fminf(fmaxf(f1, 0.f), top);
  }
  Corners o;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int st = (k >> 2) & 1, sy = (k >> 1) & 1, sx = k & 1;
    o.w[k] = (a[0][st] * a[1][sy]) * a[2][sx];
    o.row[k] = (i[0][st] + (i[1][sy] + i[2][sx] * sp.res) * sp.res) * FN_GW;
  }
  return o;
}

// one axis of corners_of, the loop body above for d alone: the lower and the upper cell of coordinate v along axis d (0: t, 1: y, 2: x)
// and their weights.  A corner of a point is one choice per axis: its weight the product of the three a's, its cell
// i_t + res (i_y + res i_x).  For the kernels that walk the grid axis by axis (the error stash); the same expressions, the same bits.
struct AxisCell {
  float a[2];
  int i[2];
};

__device__ __forceinline__ AxisCell axis_cell(const Spatial& sp, int d, float v) {
#pragma clang fp contract(off)
  const float top = (float)(sp.res - 1);
  const float xs = (v - sp.centre[d]) * sp.scale[d];
  const float u = ((xs + 1.f) * 0.5f) * sp.span + 0.5f;
  const float f0 = floorf(u), f1 = ceilf(u + 1e-6f);
  AxisCell o;
  o.a[0] = f1 - u;
  o.a[1] = u - f0;
  o.i[0] = (int)fminf(fmaxf(f0, 0.f), top);
  o.i[1] = (int)fminf(fmaxf(f1, 0.f), top);
  return o;
}

}  // namespace

}  // namespace sininn
