// What the fused coordinate-network kernels share (flownet.hip, siren.hip).  Internal linkage: each file compiles its own copy.
//   device  the 64-point tile and its hidden tile in LDS; point_coord; the LDS-tile GEMM (gemm_lds) and one K group of four (mfma_k4) on
//           v_mfma_f32_16x16x4_f32; store_acc with its epilogue (Plain, BiasRelu, Phase); copy_tile_out; stage_coord.
//           The output layer, dout, the tile load, the column sums and the coordinate selection stay spelled out in each kernel: moved
//           into a helper, each of them changed the instructions of a hot kernel.  The two transpose kernels stay where they are too
//   host    check_points / check_layers / check_saved / check_forward_buffers / check_backward_buffers: the parts of a descriptor and
//           their refusals that do not depend on the network (check_points: the grid of a call, or, poses != nullptr, its pose list);
//           chain_blocks, raise_lds; Call / check_call / call_name: the call descriptor of an entry point, validated, and the name it
//           refuses under
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

// the coordinates of point p: row p of the pose list [N][3] (q.poses, points mode: a wave-uniform branch on a kernel argument), else point
// p of the (times, ys, xs) grid; Q: a kernel descriptor with T, H, W, N, the axis vectors and poses
template <class Q>
__device__ __forceinline__ Coord point_coord(const Q& q, int p) {
  p = p < q.N ? p : q.N - 1;
  if (q.poses) {
    const float* const r = q.poses + 3 * p;            // N <= 2^22: 3 p fits an int
    return Coord{r[0], r[1], r[2]};
  }
  const int hw = q.H * q.W;
  const int t = p / hw, rem = p - t * hw;
  const int y = rem / q.W, x = rem - y * q.W;
  return Coord{q.times[t], q.ys[y], q.xs[x]};
}

// DIM coordinates per point.  3: point_coord above, as it is.  2 (one frame pair, domain_dim = 2): row p of the pose list [N][2], columns
// (y, x), else point p of the (ys, xs) grid (T = 1, `times` is not read); t is a literal zero that no encoder of this dimension reads
template <int DIM, class Q>
__device__ __forceinline__ Coord point_coord_dim(const Q& q, int p) {
  if constexpr (DIM == 3) {
    return point_coord(q, p);
  } else {
    p = p < q.N ? p : q.N - 1;
    if (q.poses) {
      const float* const r = q.poses + 2 * p;
      return Coord{0.f, r[0], r[1]};
    }
    const int y = p / q.W, x = p - y * q.W;
    return Coord{0.f, q.ys[y], q.xs[x]};
  }
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

// what store_acc does to an accumulator on its way to the LDS tile; col(c): the per-column operand, read once per column
struct Plain {                                         // as it is.  Not flownet.hip's chain kernel: its PlainAddZero stores acc + 0.f (-0 -> +0)
  __device__ __forceinline__ float col(int) const { return 0.f; }
  __device__ __forceinline__ float operator()(float v, float) const { return v; }
};
struct BiasRelu {                                      // max(acc + bias, 0)
  const float* bias;
  __device__ __forceinline__ float col(int c) const { return bias[c]; }
  __device__ __forceinline__ float operator()(float v, float bq) const { return fmaxf(v + bq, 0.f); }
};
struct Phase {                                         // omega (acc + bias), as torch rounds it: the linear layer's sum, then the product
  const float* bias;
  float omega;
  __device__ __forceinline__ float col(int c) const { return bias[c]; }
  __device__ __forceinline__ float operator()(float v, float bq) const { return __fmul_rn(omega, v + bq); }
};

// accumulators -> LDS tile through an epilogue
template <class EPI>
__device__ __forceinline__ void store_acc(float* hs, int cw, int li, int kq, const f32x4 (&acc)[4][4], const EPI epi) {
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const float bq = epi.col(cw + 16 * n + li);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) hs[(16 * m + 4 * kq + r) * FN_HS + cw + 16 * n + li] = epi(acc[m][n][r], bq);
  }
}

// one K group of four on the MFMA (the coordinates: lane group kq holds t, y, x, 0)
__device__ __forceinline__ void mfma_k4(const float (&a)[4], const float (&b)[4], f32x4 (&acc)[4][4]) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[n], acc[m][n], 0, 0, 0);
}

// cs [64][4]: row tid = (t, y, x, 0) of point tid of the tile (tid < 64)
template <class Q>
__device__ __forceinline__ void stage_coord(const Q& q, float* cs, int tile, int tid) {
  const Coord c = point_coord(q, tile * FN_P + tid);
  *reinterpret_cast<f32x4*>(cs + tid * FN_CS) = (f32x4){c.t, c.y, c.x, 0.f};
}

// DIM = 2: row tid = (y, x, 0, 0), the order of the two coordinate columns of a [256][514] layer 1
template <int DIM, class Q>
__device__ __forceinline__ void stage_coord_dim(const Q& q, float* cs, int tile, int tid) {
  if constexpr (DIM == 3) {
    stage_coord(q, cs, tile, tid);
  } else {
    const Coord c = point_coord_dim<2>(q, tile * FN_P + tid);
    *reinterpret_cast<f32x4*>(cs + tid * FN_CS) = (f32x4){c.y, c.x, 0.f, 0.f};
  }
}

// ---- host: the parts of a descriptor that do not depend on the network.  A: the C struct of a call, Q: the kernels' descriptor ----
// the points of a call (`more` / `what`: further pointers refused in the same sentence)
struct PoseList {
  const float* poses;      // device [n][3]
  int64_t n;
};

// pl == nullptr: the grid of the descriptor, T H W in 1 .. 2^22 and the axis vectors.  Else the pose list, n in 1 .. 2^22: the descriptor's
// grid is not read, the kernels see T = H = 1, W = n, which makes [T][4][H][W] the planar [4][n]
template <class A, class Q>
int check_points(const A* a, const char* who, Q& q, const PoseList* pl = nullptr, bool more = true, const char* what = "axis") {
  if (pl) {
    SININN_CHECK(pl->n >= 1 && pl->n <= (int64_t)1 << 22, "%s: %lld points (1 .. 2^22)", who, (long long)pl->n);
    SININN_CHECK(pl->poses != nullptr, "%s: null poses pointer", who);
    SININN_CHECK(more, "%s: null %s pointer", who, what);
    q.T = 1; q.H = 1; q.W = (int)pl->n;
    q.poses = pl->poses;
  } else {
    SININN_CHECK(a->T > 0 && a->H > 0 && a->W > 0 && (int64_t)a->T * a->H * a->W <= (int64_t)1 << 22, "%s: grid %d x %d x %d (1 .. 2^22 points)",
                 who, a->T, a->H, a->W);
    SININN_CHECK(a->times && a->ys && a->xs && more, "%s: null %s pointer", who, what);
    q.T = a->T; q.H = a->H; q.W = a->W;
    q.times = a->times; q.ys = a->ys; q.xs = a->xs;
  }
  q.N = q.T * q.H * q.W;
  q.ntiles = (q.N + FN_P - 1) / FN_P;
  return 0;
}

// the per-point mask of a call: what SPATIAL adds
struct SpatialArgs {
  const float* grid;
  int res;
  const float* centre_scale;   // host [6]
};

// ---- the call descriptor (sininn_flownet_call) as the launch functions take it: validated by check_call, the plain call for a null one ----
enum CallKind { CALL_FORWARD, CALL_BACKWARD, CALL_SAMPLE_MASK };

struct Call {
  sininn_flownet_call c;
  PoseList points;
  SpatialArgs grid;
  std::string name;            // the name the call refuses under: <stem>[_spatial][_points]
  bool has(unsigned bit) const { return (c.mode & bit) != 0; }
  const PoseList* pl() const { return has(SININN_FLOWNET_AT_POINTS) ? &points : nullptr; }
  const SpatialArgs* spatial() const { return has(SININN_FLOWNET_SPATIAL) ? &grid : nullptr; }
  const char* who() const { return name.c_str(); }
};

// the name an entry point refuses under: <net>_<forward | backward[_encgrad | _posegrad]>[_spatial][_points], <net>_sample_mask[_points]
std::string call_name(const char* net, CallKind kind, unsigned mode) {
  const char* const stem = kind == CALL_FORWARD                 ? "_forward"
                           : kind == CALL_SAMPLE_MASK           ? "_sample_mask"
                           : mode & SININN_FLOWNET_POSEGRAD     ? "_backward_posegrad"
                           : mode & SININN_FLOWNET_ENCGRAD      ? "_backward_encgrad"
                                                                : "_backward";
  return std::string(net) + stem + (mode & SININN_FLOWNET_SPATIAL && kind != CALL_SAMPLE_MASK ? "_spatial" : "") +
         (mode & SININN_FLOWNET_AT_POINTS ? "_points" : "");
}

// the head of every run entry point: the call descriptor itself (its size, its bits, its dimension) and the combinations no kernel exists
// for, each refused in one sentence that names it, before the network descriptor is looked at.  net: "flownet" or "siren"
int check_call(const sininn_flownet_call* in, const char* net, CallKind kind, Call& out) {
  const bool siren = net[0] == 's';
  out.c = sininn_flownet_call{};
  out.c.struct_bytes = sizeof(sininn_flownet_call);
  out.c.domain_dim = 3;
  if (in) {
    out.name = call_name(net, kind, 0);
    SININN_CHECK(in->struct_bytes == sizeof(sininn_flownet_call), "%s: call descriptor: struct_bytes is %zu, this library was built with %zu",
                 out.who(), in->struct_bytes, sizeof(sininn_flownet_call));
    out.c = *in;
  }
  const unsigned known = SININN_FLOWNET_AT_POINTS | SININN_FLOWNET_SPATIAL | SININN_FLOWNET_ENCGRAD | SININN_FLOWNET_POSEGRAD;
  const unsigned mode = out.c.mode;
  const int dim = out.c.domain_dim;
  out.name = call_name(net, kind, mode);
  out.points = PoseList{out.c.poses, out.c.n};
  out.grid = SpatialArgs{out.c.grid, out.c.res, out.c.centre_scale};
  const char* const who = out.who();
  SININN_CHECK((mode & ~known) == 0, "%s: call descriptor: unknown mode bits 0x%x (AT_POINTS 1, SPATIAL 2, ENCGRAD 4, POSEGRAD 8)", who,
               mode & ~known);
  if (siren) {
    SININN_CHECK(dim == 3, "%s: domain_dim %d: the SIREN kernels take three coordinates per point", who, dim);
    SININN_CHECK(!out.has(SININN_FLOWNET_SPATIAL), "%s: SPATIAL with SIREN: a per-point mask needs a progressive encoding, SIREN has none", who);
    SININN_CHECK(!out.has(SININN_FLOWNET_ENCGRAD), "%s: ENCGRAD with SIREN: there is no frequency matrix to differentiate", who);
  } else {
    SININN_CHECK(dim == 3 || dim == 2, "%s: domain_dim %d: the kernels take 3 coordinates per point (t, y, x) or 2 (y, x)", who, dim);
  }
  if (kind != CALL_BACKWARD)
    SININN_CHECK(!(mode & (SININN_FLOWNET_ENCGRAD | SININN_FLOWNET_POSEGRAD)),
                 "%s: ENCGRAD / POSEGRAD outside a backward call: the frequency and the coordinate gradient are outputs of the backward pass", who);
  SININN_CHECK(kind != CALL_SAMPLE_MASK || out.has(SININN_FLOWNET_SPATIAL), "%s: sample_mask without SPATIAL: the mask it samples is the grid's", who);
  SININN_CHECK(!out.has(SININN_FLOWNET_POSEGRAD) || out.has(SININN_FLOWNET_AT_POINTS),
               "%s: POSEGRAD without AT_POINTS: the coordinate gradient is one with respect to a pose list", who);
  if (dim == 2) {
    SININN_CHECK(!out.has(SININN_FLOWNET_SPATIAL), "%s: domain_dim 2 with SPATIAL: the mask grid is one over (t, y, x)", who);
    SININN_CHECK(!out.has(SININN_FLOWNET_ENCGRAD), "%s: domain_dim 2 with ENCGRAD: the frequency gradient exists for three coordinates only", who);
    SININN_CHECK(!out.has(SININN_FLOWNET_POSEGRAD), "%s: domain_dim 2 with POSEGRAD: the coordinate gradient exists for three coordinates only", who);
  }
  return 0;
}

template <int NL, class A, class Q>
int check_layers(const A* a, const char* who, Q& q) {
  for (int l = 0; l < NL; ++l) {
    SININN_CHECK(a->w[l] && a->b[l], "%s: null weight / bias %d", who, l);
    SININN_CHECK(aligned16(a->w[l]), "%s: weight %d must be 16-byte aligned", who, l);
    q.w[l] = a->w[l];
    q.b[l] = a->b[l];
  }
  return 0;
}

template <class A>
int check_saved(const A* a, const char* who, size_t need) {
  SININN_CHECK(a->saved_bytes >= need, "%s: saved holds %zu bytes, %zu needed", who, a->saved_bytes, need);
  return 0;
}

// a forward call: flows, and `saved` where the caller wants the training mode
template <class A, class Q>
int check_forward_buffers(const A* a, const char* who, size_t saved_need, Q& q) {
  SININN_CHECK(a->flows != nullptr, "%s: null flows", who);
  q.flows = a->flows;
  if (a->saved) {
    if (int rc = check_saved(a, who, saved_need)) return rc;
    SININN_CHECK(aligned16(a->saved), "%s: saved must be 16-byte aligned", who);
    q.saved = a->saved;
  }
  return 0;
}

// a backward call: dflows, saved, the workspace and NL pairs of gradient pointers
template <int NL, class A, class Q>
int check_backward_buffers(const A* a, const char* who, size_t saved_need, size_t workspace_need, Q& q) {
  SININN_CHECK(a->dflows && a->saved && a->workspace, "%s: null dflows / saved / workspace", who);
  if (int rc = check_saved(a, who, saved_need)) return rc;
  SININN_CHECK(a->workspace_bytes >= workspace_need, "%s: workspace holds %zu bytes, %zu needed", who, a->workspace_bytes, workspace_need);
  SININN_CHECK(aligned16(a->saved) && aligned16(a->workspace), "%s: saved / workspace must be 16-byte aligned", who);
  for (int l = 0; l < NL; ++l) SININN_CHECK(a->gw[l] && a->gb[l], "%s: null gradient pointer %d", who, l);
  q.saved = a->saved;
  q.dflows = a->dflows;
  return 0;
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
