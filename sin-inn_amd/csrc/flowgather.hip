// Frame synthesis by gathering: the flows are taken at the in-between time s, on the grid of the frame being synthesized,
// so both source frames are read through a backward warp -- no accumulator, no zero-fill, no atomics, no holes.
//   q0 = p + c0 G0(p),  q1 = p + c1 G1(p)                        G0 toward the previous frame, G1 toward the next, in pixels
//   (W0, n0) = sample(I0, q0),  (W1, n1) = sample(I1, q1)        exact-geometry bilinear; a tap outside the frame adds 0 to W and to n
//   a0 = 1 - tau, a1 = tau,  L = a0 I0(p) + a1 I1(p)
//   out = (a0 W0 + a1 W1 + e L) / (a0 n0 + a1 n1 + e),  e = 2^-10
// G0 and G1 are channel pairs of time slices of one (T', 4, H, W) tensor, named per (b, k) by a slot table the host has validated:
// six ints a row -- idx0, idx1 (time slice), ch0, ch1 (0 or 2), then the bits of the floats c0, c1.  One launch whatever K is.
// Every operation is rounded once and none is contracted (`flowsynth.gather_composed` evaluates the same expression in torch).
// Each piece of that arithmetic is one helper with its own `fp contract(off)` (the pragma does not reach into a callee), and every
// kernel is made of them, so they agree to the bit: the grid rule (flowgather_kernel), its gradient with respect to the flows (DESIGN 22:
// flowgather_bwd_kernel, flowgather_reduce_kernel) and both at a list of points (flowgather_points_kernel, .._bwd_kernel).
// The occlusion-aware rule (flowgather_kernel<.., VIS = true>) takes two visibility planes per pair, M0 (1 where a pixel of
// frame 0 is visible in frame 1) and M1 (the same for frame 1 in frame 0), and weighs each sample by what the OTHER sample found:
//   o0 = S(1 - M0, q0),  o1 = S(1 - M1, q1)                      the taps and weights of W0, W1; a tap outside the frame adds 0
//   v0 = 1 - o1,  v1 = 1 - o0;   b0 = a0 v0,  b1 = a1 v1
//   out = (b0 W0 + b1 W1 + e L) / (b0 n0 + b1 n1 + e)
// With M0 = M1 = 1 every 1 - M is an exact 0, v = 1, b = a: the plain rule's bits.
#include <type_traits>
#include "common.h"
#include "bilinear_taps.h"

namespace sininn {

constexpr int FG_THREADS = 256;         // one block: 256 consecutive pixels of one frame's flattened H W
constexpr int FG_MAX_K = 64;
constexpr int FG_SLOT_INTS = 6;

static int64_t gather_tiles(int64_t n) { return (n + FG_THREADS - 1) / FG_THREADS; }         // blocks of FG_THREADS lanes over n
// launch(std::integral_constant<int, C>()): the kernels exist for C = 1 and C = 3, and the checks admit no other.
template <typename Launch>
static void gather_per_channels(int C, Launch launch) {
  if (C == 1) launch(std::integral_constant<int, 1>());
  else launch(std::integral_constant<int, 3>());
}

// The four taps of one sample: the offset of the north-west tap and the weights, zero where the tap lies outside the frame.
// n is the sum of the weights inside.  A coordinate that is not finite, or too large for an int, has no tap inside.
// wx0 .. wy1 are the four one-dimensional weights of the cell floor(q) (zero without a tap inside): the backward pass differentiates them.
struct GatherTaps {
  int64_t nw;
  float w00, w01, w10, w11, n;
  float wx0, wx1, wy0, wy1;
  bool v00, v01, v10, v11;
};

// (px, py): the point the sample is displaced from, a pixel of the grid or (flowgather_points_kernel) any fp32 coordinate.
__device__ __forceinline__ GatherTaps gather_taps_at(float px, float py, float c, float gx, float gy, int H, int W) {
#pragma clang fp contract(off)
  GatherTaps t = {};
  const float sx = c * gx, sy = c * gy;                   // the product is rounded, then the sum
  const float qx = px + sx, qy = py + sy;
  if (!(fabsf(qx) < 1e9f) || !(fabsf(qy) < 1e9f)) return t;       // NaN and inf fail the comparison too
  const BilinearTaps b = bilinear_taps(qx, qy);
  const bool xa = b.x0 >= 0 && b.x0 < W, xb = b.x0 + 1 >= 0 && b.x0 + 1 < W, ya = b.y0 >= 0 && b.y0 < H, yb = b.y0 + 1 >= 0 && b.y0 + 1 < H;
  t.v00 = ya && xa; t.v01 = ya && xb; t.v10 = yb && xa; t.v11 = yb && xb;
  t.wx0 = b.wx0; t.wx1 = b.wx1; t.wy0 = b.wy0; t.wy1 = b.wy1;
  t.w00 = t.v00 ? b.wy0 * b.wx0 : 0.f; t.w01 = t.v01 ? b.wy0 * b.wx1 : 0.f;
  t.w10 = t.v10 ? b.wy1 * b.wx0 : 0.f; t.w11 = t.v11 ? b.wy1 * b.wx1 : 0.f;
  t.n = ((t.w00 + t.w01) + t.w10) + t.w11;
  t.nw = (int64_t)b.y0 * W + b.x0;                           // read only through a tap that is inside
  return t;
}

// The four taps of one plane, fetched once: a tap outside the frame is 0 and is not read.
struct GatherTapValues { float t00, t01, t10, t11; };

__device__ __forceinline__ GatherTapValues gather_fetch(const float* __restrict__ plane, const GatherTaps& t, int W) {
  return {t.v00 ? plane[t.nw] : 0.f, t.v01 ? plane[t.nw + 1] : 0.f, t.v10 ? plane[t.nw + W] : 0.f, t.v11 ? plane[t.nw + W + 1] : 0.f};
}

// The taps of the all-ones image: n and its slopes are gather_sample and gather_slopes of these.
__device__ __forceinline__ GatherTapValues gather_ones(const GatherTaps& t) {
  return {t.v00 ? 1.f : 0.f, t.v01 ? 1.f : 0.f, t.v10 ? 1.f : 0.f, t.v11 ? 1.f : 0.f};
}

__device__ __forceinline__ float gather_sample(const GatherTapValues& v, const GatherTaps& t) {
#pragma clang fp contract(off)
  return ((t.w00 * v.t00 + t.w01 * v.t01) + t.w10 * v.t10) + t.w11 * v.t11;
}

// The slopes of one sampled plane along x and y: the derivative of the bilinear interpolant of the zero-padded plane inside
// the cell floor(q) the forward pass took (on a cell border: the right-hand derivative).  A sample without a tap has all weights zero.
__device__ __forceinline__ float2 gather_slopes(const GatherTapValues& v, const GatherTaps& t) {
#pragma clang fp contract(off)
  return {t.wy0 * (v.t01 - v.t00) + t.wy1 * (v.t11 - v.t10), t.wx0 * (v.t10 - v.t00) + t.wx1 * (v.t11 - v.t01)};
}

// One channel of the rule: D = a0 n0 + a1 n1 + e, then out = (a0 W0 + a1 W1 + e (a0 h0 + a1 h1)) / D.  h0, h1 are the two frames at the
// point itself: I0(p), I1(p) in the grid kernels, sample(I0, p), sample(I1, p) in the point kernels.
constexpr float FG_EPS = 0.0009765625f;

__device__ __forceinline__ float gather_den(float a0, float a1, float n0, float n1) {
#pragma clang fp contract(off)
  return (a0 * n0 + a1 * n1) + FG_EPS;
}

// b0, b1 weigh the two samples and (a0, a1) the linear blend L: the same pair in the plain rule, a0 v0 and a1 v1 in the masked one.
__device__ __forceinline__ float gather_blend_weighted(float a0, float a1, float b0, float b1, float den, float w0, float w1, float h0,
                                                       float h1) {
#pragma clang fp contract(off)
  const float lin = a0 * h0 + a1 * h1;
  const float num = (b0 * w0 + b1 * w1) + FG_EPS * lin;
  return __fdiv_rn(num, den);
}

__device__ __forceinline__ float gather_blend(float a0, float a1, float den, float w0, float w1, float h0, float h1) {
  return gather_blend_weighted(a0, a1, a0, a1, den, w0, w1, h0, h1);
}

// 1 - M at the four taps of one sample, for o = S(1 - M, q): a tap outside the frame stays 0 and is not read.  The mask is
// read as a number and nothing is indexed with it.
__device__ __forceinline__ GatherTapValues gather_hidden(const float* __restrict__ mask, const GatherTaps& t, int W) {
#pragma clang fp contract(off)
  const GatherTapValues m = gather_fetch(mask, t, W);
  return {t.v00 ? 1.f - m.t00 : 0.f, t.v01 ? 1.f - m.t01 : 0.f, t.v10 ? 1.f - m.t10 : 0.f, t.v11 ? 1.f - m.t11 : 0.f};
}

// The sample weights of the masked rule: frame 0 is trusted unless the surface found in frame 1 is hidden in frame 0, and conversely.
__device__ __forceinline__ float2 gather_visible_weights(float a0, float a1, float o0, float o1) {
#pragma clang fp contract(off)
  const float v0 = 1.f - o1, v1 = 1.f - o0;
  return {a0 * v0, a1 * v1};
}

// The gradient with respect to the flows, for one of the two samples (W, n, c, a), `w` and `n` the slopes of W_c and of n:
//   dG = c a / D  sum_c g_c (grad_q W_c - out_c grad_q n)
// gather_grad_add takes one channel into the sum, gather_grad_scale closes it.  No gradient to the frames, tau or the coefficients.
__device__ __forceinline__ void gather_grad_add(float g, float v, float2 w, float2 n, float2& s) {
#pragma clang fp contract(off)
  s.x = s.x + g * (w.x - v * n.x); s.y = s.y + g * (w.y - v * n.y);
}

__device__ __forceinline__ float2 gather_grad_scale(float c, float a, float den, float2 s) {
#pragma clang fp contract(off)
  const float k = __fdiv_rn(c * a, den);
  return {k * s.x, k * s.y};
}

// The prologue of the grid kernels.  A block is 256 consecutive pixels of one plane: `frame` counts the blocks' planes (b K + k, with
// KLOOP b, in the reduce kernel 2 target + component), r = y W + x.  False past the plane's last pixel.
struct GatherLane { unsigned frame; int x, y; int64_t r; };

__device__ __forceinline__ bool gather_lane(int tiles, int W, int64_t HW, GatherLane& p) {
  const unsigned pix = (blockIdx.x % (unsigned)tiles) * FG_THREADS + threadIdx.x;         // H W < 2^31: 32-bit divisions only
  p = {blockIdx.x / (unsigned)tiles, (int)(pix % (unsigned)W), (int)(pix / (unsigned)W), pix};
  return pix < HW;
}

// Row (b, k) of the slot table at the lane's pixel: the two tap sets, the coefficients, the blend weights and D.
struct GatherRow { GatherTaps t0, t1; float c0, c1, a0, a1, den; };

__device__ __forceinline__ GatherRow gather_row(const float* __restrict__ flows, int64_t flow_stride, const int* __restrict__ slot,
                                                float tk, const GatherLane& p, int H, int W, int64_t HW) {
#pragma clang fp contract(off)
  GatherRow row;
  const float* g0 = flows + slot[0] * flow_stride + slot[2] * HW + p.r;
  const float* g1 = flows + slot[1] * flow_stride + slot[3] * HW + p.r;
  row.c0 = __int_as_float(slot[4]); row.c1 = __int_as_float(slot[5]);
  row.t0 = gather_taps_at((float)p.x, (float)p.y, row.c0, g0[0], g0[HW], H, W);
  row.t1 = gather_taps_at((float)p.x, (float)p.y, row.c1, g1[0], g1[HW], H, W);
  row.a0 = 1.f - tk; row.a1 = tk;
  row.den = gather_den(row.a0, row.a1, row.t0.n, row.t1.n);
  return row;
}

// The visibility planes of the masked rule, (B, 1, H, W) each; the plain rule carries none.
template <bool VIS> struct GatherVisible {};
template <> struct GatherVisible<true> { const float* m0; const float* m1; };

// KLOOP = false: a block is 256 pixels of one (b, k).  KLOOP = true: a block is 256 pixels of one b and every lane walks k, so I0(p)
// and I1(p) are loaded once for all K.  The slot row and tau are block-uniform either way.  VIS: the masked rule, four more
// tap values per sample from the pair's mask plane, through the taps the sample has already.
template <int C, bool KLOOP, bool VIS>
__global__ __launch_bounds__(FG_THREADS) void flowgather_kernel(const float* __restrict__ i0, const float* __restrict__ i1,
                                                                const float* __restrict__ flows, int64_t flow_stride,
                                                                const int* __restrict__ slots, const float* __restrict__ tau, int K,
                                                                int H, int W, int tiles, float* __restrict__ out,
                                                                uint8_t* __restrict__ out_u8, GatherVisible<VIS> vis) {
  const int64_t HW = (int64_t)H * W;
  GatherLane p;
  if (!gather_lane(tiles, W, HW, p)) return;
  const int64_t r = p.r, b = KLOOP ? p.frame : p.frame / (unsigned)K;
  const float* i0b = i0 + b * C * HW;
  const float* i1b = i1 + b * C * HW;
  float here0[C], here1[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { here0[c] = i0b[c * HW + r]; here1[c] = i1b[c * HW + r]; }
  auto pixel = [&](int64_t bk, float tk) {                 // one output pixel of frame (b, k)
    const GatherRow row = gather_row(flows, flow_stride, slots + bk * FG_SLOT_INTS, tk, p, H, W, HW);
    const int64_t o = bk * C * HW + r;
    float b0 = row.a0, b1 = row.a1, den = row.den;
    if constexpr (VIS) {
      const float o0 = gather_sample(gather_hidden(vis.m0 + b * HW, row.t0, W), row.t0);
      const float o1 = gather_sample(gather_hidden(vis.m1 + b * HW, row.t1, W), row.t1);
      const float2 bw = gather_visible_weights(row.a0, row.a1, o0, o1);
      b0 = bw.x; b1 = bw.y;
      den = gather_den(b0, b1, row.t0.n, row.t1.n);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float w0 = gather_sample(gather_fetch(i0b + c * HW, row.t0, W), row.t0);
      const float w1 = gather_sample(gather_fetch(i1b + c * HW, row.t1, W), row.t1);
      const float v = gather_blend_weighted(row.a0, row.a1, b0, b1, den, w0, w1, here0[c], here1[c]);
      out[o + c * HW] = v;
      if (out_u8) out_u8[o + c * HW] = (uint8_t)frame_byte(v);
    }
  };
  if (KLOOP) for (int k = 0; k < K; ++k) pixel(b * K + k, tau[k]);
  else pixel(p.frame, tau[p.frame % (unsigned)K]);
}

// What the forward and the backward launch both refuse, each under its own name.  `planes`: the most H W planes a (b, k) has in a buffer.
static int flow_gather_check(const char* who, const void* i0, const void* i1, const void* flows, const void* slots, const void* tau,
                             int64_t flow_sample_stride, int B, int K, int C, int H, int W, int planes) {
  SININN_CHECK(i0 && i1 && flows && slots && tau, "%s: null pointer", who);
  SININN_CHECK(B > 0 && H > 0 && W > 0, "%s: bad shape (every size must be positive)", who);
  SININN_CHECK(C == 1 || C == 3, "%s: frames have 1 or 3 channels (got %d)", who, C);
  SININN_CHECK(K >= 1 && K <= FG_MAX_K, "%s: K = %d times in one call, 1 to %d are supported", who, K, FG_MAX_K);
  const int64_t HW = (int64_t)H * W;
  SININN_CHECK(HW <= 0x7fffffff, "%s: H * W = %lld is past an int index", who, (long long)HW);
  SININN_CHECK((int64_t)B * K * gather_tiles(HW) <= 0x7fffffff, "%s: B * K * H * W = %lld needs more blocks than one launch has", who,
               (long long)B * K * HW);
  SININN_CHECK((int64_t)B * K * planes <= INT64_MAX / HW, "%s: B * K * C * H * W is past a 64-bit index", who);
  SININN_CHECK(flow_sample_stride >= 4 * HW, "%s: sample stride %lld is smaller than four channel planes (%lld)", who,
               (long long)flow_sample_stride, (long long)(4 * HW));
  return 0;
}

template <bool VIS>
static int flow_gather_run(const char* who, const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride,
                           const int* slots, const float* tau, int B, int K, int C, int H, int W, int k_loop, float* out,
                           uint8_t* out_u8, GatherVisible<VIS> vis, hipStream_t st) {
  SININN_CHECK(out, "%s: null pointer", who);
  if (flow_gather_check(who, i0, i1, flows, slots, tau, flow_sample_stride, B, K, C, H, W, C)) return 1;
  const int64_t tiles = gather_tiles((int64_t)H * W);
  const dim3 grid((unsigned)((int64_t)B * (k_loop ? 1 : K) * tiles)), block(FG_THREADS);
  gather_per_channels(C, [&](auto ch) {
    constexpr int CH = decltype(ch)::value;
    if (k_loop)
      hipLaunchKernelGGL((flowgather_kernel<CH, true, VIS>), grid, block, 0, st, i0, i1, flows, flow_sample_stride, slots, tau, K, H,
                         W, (int)tiles, out, out_u8, vis);
    else
      hipLaunchKernelGGL((flowgather_kernel<CH, false, VIS>), grid, block, 0, st, i0, i1, flows, flow_sample_stride, slots, tau, K, H,
                         W, (int)tiles, out, out_u8, vis);
  });
  SININN_LAUNCH_CHECK(VIS ? "flowgather_visible" : "flowgather");
  return 0;
}

extern "C" int sininn_flow_gather(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                                  const float* tau, int B, int K, int C, int H, int W, int k_loop, float* out, uint8_t* out_u8, void* stream) {
  return flow_gather_run<false>("flow_gather", i0, i1, flows, flow_sample_stride, slots, tau, B, K, C, H, W, k_loop, out, out_u8, {},
                                ST(stream));
}

// [p, p + n) and [q, q + m) in bytes share nothing
static bool gather_apart(const void* p, int64_t n, const void* q, int64_t m) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a + (uintptr_t)n <= b || b + (uintptr_t)m <= a;
}

// The masked rule: the plain call's checks, then the masks -- present, readable as floats, and not inside what is written.
extern "C" int sininn_flow_gather_visible(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                                          const float* tau, const float* m0, const float* m1, int B, int K, int C, int H, int W, int k_loop,
                                          float* out, uint8_t* out_u8, void* stream) {
  hipStream_t st = ST(stream);
  const char* who = "flow_gather_visible";
  SININN_CHECK(m0 && m1, "%s: a visibility mask is null", who);
  SININN_CHECK(((uintptr_t)m0 & 3) == 0 && ((uintptr_t)m1 & 3) == 0, "%s: the masks are fp32 planes and must be 4-byte aligned", who);
  SININN_CHECK(out, "%s: null pointer", who);
  if (flow_gather_check(who, i0, i1, flows, slots, tau, flow_sample_stride, B, K, C, H, W, C)) return 1;
  const int64_t HW = (int64_t)H * W, mask_bytes = 4 * (int64_t)B * HW, frames = (int64_t)B * K * C * HW;
  SININN_CHECK(gather_apart(m0, mask_bytes, out, 4 * frames) && gather_apart(m1, mask_bytes, out, 4 * frames) &&
                   (!out_u8 || (gather_apart(m0, mask_bytes, out_u8, frames) && gather_apart(m1, mask_bytes, out_u8, frames))),
               "%s: a mask of B * H * W = %lld floats overlaps the output", who, (long long)B * HW);
  return flow_gather_run<true>(who, i0, i1, flows, flow_sample_stride, slots, tau, B, K, C, H, W, k_loop, out, out_u8,
                               GatherVisible<true>{m0, m1}, st);
}

// ---- the gradient with respect to the flows ----
// One lane per (b, k, y, x), the forward kernel's KLOOP = false shape.  The lane recomputes the two tap sets and out_c exactly as the
// forward pass rounds them, reads C words of g and writes four floats: dG0 (x, y), dG1 (x, y).  `dflows` == nullptr: into the per-row
// buffer `rows` (B, K, 4, H, W), which flowgather_reduce_kernel sums per target.  Otherwise straight into channels ch0, ch0 + 1 of
// slice idx0 and ch1, ch1 + 1 of slice idx1 of the contiguous (T, 4, H, W) `dflows`: the host guarantees that no two rows share a
// target.  Either way the addresses of a wave are 64 consecutive floats of one plane.
template <int C>
__global__ __launch_bounds__(FG_THREADS) void flowgather_bwd_kernel(const float* __restrict__ i0, const float* __restrict__ i1,
                                                                    const float* __restrict__ flows, int64_t flow_stride,
                                                                    const int* __restrict__ slots, const float* __restrict__ tau,
                                                                    const float* __restrict__ gout, int K, int H, int W, int tiles,
                                                                    float* __restrict__ rows, float* __restrict__ dflows) {
  const int64_t HW = (int64_t)H * W;
  GatherLane p;
  if (!gather_lane(tiles, W, HW, p)) return;
  const int64_t r = p.r, bk = p.frame, b = p.frame / (unsigned)K;
  const float* i0b = i0 + b * C * HW;
  const float* i1b = i1 + b * C * HW;
  const int* slot = slots + bk * FG_SLOT_INTS;
  const GatherRow row = gather_row(flows, flow_stride, slot, tau[p.frame % (unsigned)K], p, H, W, HW);
  const float2 n0 = gather_slopes(gather_ones(row.t0), row.t0), n1 = gather_slopes(gather_ones(row.t1), row.t1);
  float2 s0 = {0.f, 0.f}, s1 = {0.f, 0.f};
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const GatherTapValues v0 = gather_fetch(i0b + c * HW, row.t0, W), v1 = gather_fetch(i1b + c * HW, row.t1, W);
    const float v = gather_blend(row.a0, row.a1, row.den, gather_sample(v0, row.t0), gather_sample(v1, row.t1), i0b[c * HW + r],
                                 i1b[c * HW + r]);             // out_c, the forward pass's bits
    const float g = gout[(bk * C + c) * HW + r];
    gather_grad_add(g, v, gather_slopes(v0, row.t0), n0, s0);
    gather_grad_add(g, v, gather_slopes(v1, row.t1), n1, s1);
  }
  float* d0;
  float* d1;
  if (dflows) {
    d0 = dflows + (slot[0] * (int64_t)4 + slot[2]) * HW + r;
    d1 = dflows + (slot[1] * (int64_t)4 + slot[3]) * HW + r;
  } else {
    d0 = rows + bk * 4 * HW + r;
    d1 = d0 + 2 * HW;
  }
  const float2 e0 = gather_grad_scale(row.c0, row.a0, row.den, s0), e1 = gather_grad_scale(row.c1, row.a1, row.den, s1);
  d0[0] = e0.x; d0[HW] = e0.y; d1[0] = e1.x; d1[HW] = e1.y;
}

// One lane per element of dflows.  `list`: for each of the 2 T targets (slice, channel pair) -- target 2 slice + pair -- the begin of its
// entries, 2 T + 1 ints, then the entries: 2 (b K + k) + which (0: dG0, 1: dG1), ascending within a target, so the sum has a fixed
// order; the first entry starts the sum (a target with one entry gets that entry's bits, the in-place path's), no entry gives 0.
__global__ __launch_bounds__(FG_THREADS) void flowgather_reduce_kernel(const float* __restrict__ rows, const int* __restrict__ list,
                                                                       int targets, int H, int W, int tiles,
                                                                       float* __restrict__ dflows) {
#pragma clang fp contract(off)
  const int64_t HW = (int64_t)H * W;
  GatherLane p;
  if (!gather_lane(tiles, W, HW, p)) return;
  const unsigned target = p.frame >> 1, comp = p.frame & 1;
  const int begin = list[target], end = list[target + 1];
  const int* entries = list + targets + 1;
  float sum = 0.f;
  for (int i = begin; i < end; ++i) {
    const float v = rows[((int64_t)entries[i] * 2 + comp) * HW + p.r];
    sum = i == begin ? v : sum + v;
  }
  dflows[(int64_t)p.frame * HW + p.r] = sum;
}

extern "C" int64_t sininn_flow_gather_bwd_workspace(int B, int K, int H, int W) {
  if (B <= 0 || K <= 0 || H <= 0 || W <= 0) return 0;
  const int64_t HW = (int64_t)H * W;
  if ((int64_t)B * K * 4 > INT64_MAX / HW) return 0;
  return (int64_t)B * K * 4 * HW;
}

extern "C" int sininn_flow_gather_bwd(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                                      const float* tau, const float* grad_out, int B, int K, int C, int H, int W, int T, const int* reduce_list,
                                      int64_t reduce_ints, float* workspace, int64_t workspace_floats, float* dflows, void* stream) {
  hipStream_t st = ST(stream);
  if (flow_gather_check("flow_gather_bwd", i0, i1, flows, slots, tau, flow_sample_stride, B, K, C, H, W, 4)) return 1;
  SININN_CHECK(grad_out, "flow_gather_bwd: the gradient of the output is null");
  SININN_CHECK(dflows, "flow_gather_bwd: the gradient of the flows is null");
  SININN_CHECK(T > 0, "flow_gather_bwd: bad shape (every size must be positive)");
  const int64_t HW = (int64_t)H * W, tiles = gather_tiles(HW);
  SININN_CHECK((int64_t)T * 4 * tiles <= 0x7fffffff, "flow_gather_bwd: T * 4 * H * W = %lld needs more blocks than one launch has",
               (long long)T * 4 * HW);
  if (reduce_list) {
    SININN_CHECK(workspace, "flow_gather_bwd: the workspace is null");
    SININN_CHECK(workspace_floats >= sininn_flow_gather_bwd_workspace(B, K, H, W),
                 "flow_gather_bwd: the workspace holds %lld floats, %lld are needed", (long long)workspace_floats,
                 (long long)sininn_flow_gather_bwd_workspace(B, K, H, W));
    SININN_CHECK(reduce_ints >= 2 * (int64_t)T + 1 && reduce_ints <= 2 * (int64_t)T + 1 + 2 * (int64_t)B * K,
                 "flow_gather_bwd: a reduce list of %lld ints; 2 T + 1 begins and at most 2 B K entries are expected",
                 (long long)reduce_ints);
  }
  const dim3 grid((unsigned)((int64_t)B * K * tiles)), block(FG_THREADS);
  if (!reduce_list) {       // in place: the targets no row names stay 0
    SININN_CHECK(hipMemsetAsync(dflows, 0, sizeof(float) * 4 * (size_t)T * (size_t)HW, st) == hipSuccess,
                 "flow_gather_bwd: hipMemsetAsync failed");
  }
  gather_per_channels(C, [&](auto ch) {
    hipLaunchKernelGGL((flowgather_bwd_kernel<decltype(ch)::value>), grid, block, 0, st, i0, i1, flows, flow_sample_stride, slots, tau,
                       grad_out, K, H, W, (int)tiles, reduce_list ? workspace : nullptr, reduce_list ? nullptr : dflows);
  });
  SININN_LAUNCH_CHECK("flowgather_bwd");
  if (reduce_list) {
    const dim3 rgrid((unsigned)((int64_t)T * 4 * tiles));
    hipLaunchKernelGGL(flowgather_reduce_kernel, rgrid, block, 0, st, (const float*)workspace, reduce_list, 2 * T, H, W, (int)tiles,
                       dflows);
    SININN_LAUNCH_CHECK("flowgather_reduce");
  }
  return 0;
}

// ---- the rule at a list of points ----
// Point n: p = pix[n] = (py, px), any fp32 coordinate; b = pair[n]; flows (S, 4, N) planar, what a stack of flow_at(.., planar = True)
// holds.  G1 = flows[0, 0:2, n], c1 = 1 - tau[n].  G0 = flows[1, 2:4, n], c0 = tau[n] where S == 2 and not rev[n]; else G0 = G1,
// c0 = -tau[n].  H0, H1 = sample(I0, p), sample(I1, p), the bilinear form of the grid kernels' I0(p), I1(p): on an integer pixel it is
// that value.  R blends a1 = blend[r] (or, per point, tau[n]) over one set of taps:
//   out[r, n, c] = (a0 W0 + a1 W1 + e (a0 H0 + a1 H1)) / (a0 n0 + a1 n1 + e)
// Nothing here is validated on the host: a pair outside [0, B) gives a row of zeros, a coordinate without a tap reads nothing.
constexpr int FGP_MAX_R = 4;
struct GatherBlend { float a1[FGP_MAX_R]; };

struct GatherPoint {
  GatherTaps t0, t1, th;
  float c0, c1, tau;
  bool rev;
};

__device__ __forceinline__ GatherPoint gather_point(const float* __restrict__ flows, const float* __restrict__ pix,
                                                    const float* __restrict__ tau, const uint8_t* __restrict__ rev, int S, int64_t N,
                                                    int64_t n, int H, int W) {
#pragma clang fp contract(off)
  GatherPoint p;
  const float2 yx = reinterpret_cast<const float2*>(pix)[n];      // one 8-byte load: (py, px)
  p.tau = tau[n];
  p.rev = S == 1 || (rev != nullptr && rev[n] != 0);
  const float g1x = flows[n], g1y = flows[N + n];
  float g0x = g1x, g0y = g1y;
  if (!p.rev) { g0x = flows[6 * N + n]; g0y = flows[7 * N + n]; }
  p.c0 = p.rev ? -p.tau : p.tau;
  p.c1 = 1.f - p.tau;
  p.t0 = gather_taps_at(yx.y, yx.x, p.c0, g0x, g0y, H, W);
  p.t1 = gather_taps_at(yx.y, yx.x, p.c1, g1x, g1y, H, W);
  p.th = gather_taps_at(yx.y, yx.x, 0.f, 0.f, 0.f, H, W);
  return p;
}

// One lane per point, 256 points a block.
template <int C>
__global__ __launch_bounds__(FG_THREADS) void flowgather_points_kernel(const float* __restrict__ i0, const float* __restrict__ i1,
                                                                       const float* __restrict__ flows, const float* __restrict__ pix,
                                                                       const int* __restrict__ pair, const float* __restrict__ tau,
                                                                       const uint8_t* __restrict__ rev, GatherBlend blend, int per_point,
                                                                       int R, int S, int64_t N, int B, int H, int W,
                                                                       float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t n = (int64_t)blockIdx.x * FG_THREADS + threadIdx.x;
  if (n >= N) return;
  const int64_t HW = (int64_t)H * W;
  const int b = pair[n];
  if (b < 0 || b >= B) {
#pragma unroll
    for (int r = 0; r < FGP_MAX_R; ++r)
      if (r < R)
#pragma unroll
        for (int c = 0; c < C; ++c) out[(r * N + n) * C + c] = 0.f;
    return;
  }
  const float* i0b = i0 + (int64_t)b * C * HW;
  const float* i1b = i1 + (int64_t)b * C * HW;
  const GatherPoint p = gather_point(flows, pix, tau, rev, S, N, n, H, W);
  float w0[C], w1[C], h0[C], h1[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    w0[c] = gather_sample(gather_fetch(i0b + c * HW, p.t0, W), p.t0); w1[c] = gather_sample(gather_fetch(i1b + c * HW, p.t1, W), p.t1);
    h0[c] = gather_sample(gather_fetch(i0b + c * HW, p.th, W), p.th); h1[c] = gather_sample(gather_fetch(i1b + c * HW, p.th, W), p.th);
  }
#pragma unroll
  for (int r = 0; r < FGP_MAX_R; ++r) {
    if (r < R) {
      const float a1 = per_point ? p.tau : blend.a1[r], a0 = 1.f - a1;
      const float den = gather_den(a0, a1, p.t0.n, p.t1.n);
#pragma unroll
      for (int c = 0; c < C; ++c) out[(r * N + n) * C + c] = gather_blend(a0, a1, den, w0[c], w1[c], h0[c], h1[c]);
    }
  }
}

// The gradient with respect to the flows, by the formulas of flowgather_bwd_kernel.  Lane n writes the 4 S values of column n itself:
// dG1 into flows[0, 0:2], dG0 into flows[1, 2:4], or under rev (and S == 1) added to dG1's pair as dG0 + dG1; the others are 0.  The R
// blends are summed in ascending r, the first starting the sum.  No atomics, no second pass.
template <int C>
__global__ __launch_bounds__(FG_THREADS) void flowgather_points_bwd_kernel(const float* __restrict__ i0, const float* __restrict__ i1,
                                                                           const float* __restrict__ flows,
                                                                           const float* __restrict__ pix, const int* __restrict__ pair,
                                                                           const float* __restrict__ tau,
                                                                           const uint8_t* __restrict__ rev, GatherBlend blend,
                                                                           int per_point, int R, int S, int64_t N, int B, int H, int W,
                                                                           const float* __restrict__ gout, float* __restrict__ dflows) {
#pragma clang fp contract(off)
  const int64_t n = (int64_t)blockIdx.x * FG_THREADS + threadIdx.x;
  if (n >= N) return;
  const int64_t HW = (int64_t)H * W;
  const int b = pair[n];
  float d0x = 0.f, d0y = 0.f, d1x = 0.f, d1y = 0.f;
  bool reversed = S == 1;
  if (b >= 0 && b < B) {
    const float* i0b = i0 + (int64_t)b * C * HW;
    const float* i1b = i1 + (int64_t)b * C * HW;
    const GatherPoint p = gather_point(flows, pix, tau, rev, S, N, n, H, W);
    reversed = p.rev;
    const float2 n0 = gather_slopes(gather_ones(p.t0), p.t0), n1 = gather_slopes(gather_ones(p.t1), p.t1);
    float w0[C], w1[C], h0[C], h1[C];
    float2 g0[C], g1[C];                    // the slopes of W0_c, W1_c
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const GatherTapValues v0 = gather_fetch(i0b + c * HW, p.t0, W), v1 = gather_fetch(i1b + c * HW, p.t1, W);
      w0[c] = gather_sample(v0, p.t0); w1[c] = gather_sample(v1, p.t1);
      h0[c] = gather_sample(gather_fetch(i0b + c * HW, p.th, W), p.th); h1[c] = gather_sample(gather_fetch(i1b + c * HW, p.th, W), p.th);
      g0[c] = gather_slopes(v0, p.t0); g1[c] = gather_slopes(v1, p.t1);
    }
#pragma unroll
    for (int r = 0; r < FGP_MAX_R; ++r) {
      if (r < R) {
        const float a1 = per_point ? p.tau : blend.a1[r], a0 = 1.f - a1;
        const float den = gather_den(a0, a1, p.t0.n, p.t1.n);
        float2 s0 = {0.f, 0.f}, s1 = {0.f, 0.f};
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float v = gather_blend(a0, a1, den, w0[c], w1[c], h0[c], h1[c]);         // out[r, n, c], the forward pass's bits
          const float g = gout[(r * N + n) * C + c];
          gather_grad_add(g, v, g0[c], n0, s0);
          gather_grad_add(g, v, g1[c], n1, s1);
        }
        const float2 e0 = gather_grad_scale(p.c0, a0, den, s0), e1 = gather_grad_scale(p.c1, a1, den, s1);
        d0x = r == 0 ? e0.x : d0x + e0.x; d0y = r == 0 ? e0.y : d0y + e0.y;
        d1x = r == 0 ? e1.x : d1x + e1.x; d1y = r == 0 ? e1.y : d1y + e1.y;
      }
    }
  }
  float* col = dflows + n;
  col[0] = reversed ? d0x + d1x : d1x;
  col[N] = reversed ? d0y + d1y : d1y;
  col[2 * N] = 0.f; col[3 * N] = 0.f;
  if (S == 2) {
    col[4 * N] = 0.f; col[5 * N] = 0.f;
    col[6 * N] = reversed ? 0.f : d0x;
    col[7 * N] = reversed ? 0.f : d0y;
  }
}

static int flow_gather_at_check(const char* who, const void* i0, const void* i1, const void* flows, const void* pix, const void* pair,
                                const void* tau, const float* blend, int R, int S, int64_t N, int B, int C, int H, int W) {
  SININN_CHECK(i0 && i1 && flows && pix && pair && tau, "%s: null pointer", who);
  SININN_CHECK(B > 0 && H > 0 && W > 0, "%s: bad shape (every size must be positive)", who);
  SININN_CHECK(C == 1 || C == 3, "%s: frames have 1 or 3 channels (got %d)", who, C);
  SININN_CHECK(S == 1 || S == 2, "%s: flows is (S, 4, N) with S = 1 or 2 (got %d)", who, S);
  SININN_CHECK(R >= 1 && R <= FGP_MAX_R, "%s: R = %d blends in one call, 1 to %d are supported", who, R, FGP_MAX_R);
  SININN_CHECK(blend || R == 1, "%s: blend == NULL is the per-point blend a1 = tau[n], R = 1 (got R = %d)", who, R);
  SININN_CHECK(N >= 1, "%s: N = %lld points, at least one is needed", who, (long long)N);
  SININN_CHECK(N <= 0x7fffffff, "%s: N = %lld is past an int index", who, (long long)N);
  const int64_t HW = (int64_t)H * W;
  SININN_CHECK(HW <= 0x7fffffff, "%s: H * W = %lld is past an int index", who, (long long)HW);
  SININN_CHECK((int64_t)B * C <= INT64_MAX / HW, "%s: B * C * H * W is past a 64-bit index", who);
  SININN_CHECK(((uintptr_t)pix & 7) == 0, "%s: pix is read as 8-byte (y, x) pairs and must be 8-byte aligned", who);
  return 0;
}

static GatherBlend flow_gather_at_blend(const float* blend, int R) {
  GatherBlend v = {};
  for (int r = 0; blend && r < R; ++r) v.a1[r] = blend[r];
  return v;
}

extern "C" int sininn_flow_gather_at(const float* i0, const float* i1, const float* flows, const float* pix, const int* pair, const float* tau,
                                     const uint8_t* rev, const float* blend, int R, int S, int64_t N, int B, int C, int H, int W, float* out,
                                     void* stream) {
  hipStream_t st = ST(stream);
  if (flow_gather_at_check("flow_gather_at", i0, i1, flows, pix, pair, tau, blend, R, S, N, B, C, H, W)) return 1;
  SININN_CHECK(out, "flow_gather_at: null pointer");
  const dim3 grid((unsigned)gather_tiles(N)), block(FG_THREADS);
  const GatherBlend a1 = flow_gather_at_blend(blend, R);
  gather_per_channels(C, [&](auto ch) {
    hipLaunchKernelGGL((flowgather_points_kernel<decltype(ch)::value>), grid, block, 0, st, i0, i1, flows, pix, pair, tau, rev, a1,
                       blend ? 0 : 1, R, S, N, B, H, W, out);
  });
  SININN_LAUNCH_CHECK("flowgather_points");
  return 0;
}

extern "C" int sininn_flow_gather_at_bwd(const float* i0, const float* i1, const float* flows, const float* pix, const int* pair, const float* tau,
                                         const uint8_t* rev, const float* blend, const float* grad_out, int R, int S, int64_t N, int B, int C,
                                         int H, int W, float* dflows, void* stream) {
  hipStream_t st = ST(stream);
  if (flow_gather_at_check("flow_gather_at_bwd", i0, i1, flows, pix, pair, tau, blend, R, S, N, B, C, H, W)) return 1;
  SININN_CHECK(grad_out, "flow_gather_at_bwd: the gradient of the output is null");
  SININN_CHECK(dflows, "flow_gather_at_bwd: the gradient of the flows is null");
  const dim3 grid((unsigned)gather_tiles(N)), block(FG_THREADS);
  const GatherBlend a1 = flow_gather_at_blend(blend, R);
  gather_per_channels(C, [&](auto ch) {
    hipLaunchKernelGGL((flowgather_points_bwd_kernel<decltype(ch)::value>), grid, block, 0, st, i0, i1, flows, pix, pair, tau, rev, a1,
                       blend ? 0 : 1, R, S, N, B, H, W, grad_out, dflows);
  });
  SININN_LAUNCH_CHECK("flowgather_points_bwd");
  return 0;
}

}  // namespace sininn
