// What the fused coordinate-network kernels share (flownet.hip, siren.hip): the 64-point tile, its hidden tile in LDS, the grid of
// points, the LDS-tile GEMM on v_mfma_f32_16x16x4_f32 and the launch helpers.  Internal linkage: each file compiles its own copy.
#pragma once
#include "common.h"

namespace sininn {

namespace {

constexpr int FN_P = 64;            // points per tile
constexpr int FN_HID = 256;
constexpr int FN_OUT = 4;
constexpr int FN_HS = FN_HID + 4;   // floats per row of the hidden tile in LDS (16-byte reads of 16 rows hit 64 distinct banks)
constexpr int FN_NTHR = 256;
constexpr int FN_CHAIN_MAX_BLOCKS = 512;
constexpr size_t FN_LDS = (size_t)(FN_P * FN_HS + FN_P * FN_OUT) * sizeof(float);
constexpr int FN_CS = 4;            // floats per row of the packed coordinate columns / of the coordinate tile in LDS

struct Coord { float t, y, x; };

// the coordinates of point p of the (times, ys, xs) grid; Q: a kernel descriptor with T, H, W, N and the axis vectors
template <class Q>
__device__ __forceinline__ Coord point_coord(const Q& q, int p) {
  p = p < q.N ? p : q.N - 1;
  const int hw = q.H * q.W;
  const int t = p / hw, rem = p - t * hw;
  const int y = rem / q.W, x = rem - y * q.W;
  return Coord{q.times[t], q.ys[y], q.xs[x]};
}

// acc[m][n] += A[rows 16 m ..][k] W[cols cw + 16 n ..][k]: A from the LDS tile, W row-major [256][256] from L2
__device__ __forceinline__ void gemm_lds(const float* hs, const float* w, int cw, int li, int kq, f32x4 (&acc)[4][4]) {
#pragma unroll 2
  for (int s = 0; s < FN_HID / 16; ++s) {
    f32x4 bf[4], af[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) bf[n] = *reinterpret_cast<const f32x4*>(w + (size_t)(cw + 16 * n + li) * FN_HID + 16 * s + 4 * kq);
#pragma unroll
    for (int m = 0; m < 4; ++m) af[m] = *reinterpret_cast<const f32x4*>(hs + (16 * m + li) * FN_HS + 16 * s + 4 * kq);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m][j], bf[n][j], acc[m][n], 0, 0, 0);
  }
}

template <int M, int N>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[M][N]) {
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int n = 0; n < N; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// LDS tile -> rows [64 tile, 64 tile + 64) of a [Npad][256] array
__device__ __forceinline__ void copy_tile_out(const float* hs, float* dst, int tile, int tid) {
#pragma unroll 4
  for (int u = 0; u < FN_P * FN_HID / 4 / FN_NTHR; ++u) {
    const int f = tid + FN_NTHR * u;
    const int row = f >> 6, c4 = (f & 63) * 4;
    *reinterpret_cast<f32x4*>(dst + ((size_t)tile * FN_P + row) * FN_HID + c4) = *reinterpret_cast<const f32x4*>(hs + row * FN_HS + c4);
  }
}

int chain_blocks(int ntiles) { return ntiles < FN_CHAIN_MAX_BLOCKS ? ntiles : FN_CHAIN_MAX_BLOCKS; }

template <class K>
int raise_lds(K k, size_t bytes, const char* name) {
  if (bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) { set_error("%s: cannot raise the LDS limit to %zu", name, bytes); return 1; }
  }
  return 0;
}

}  // namespace

}  // namespace sininn
