// The three small operators the flow trainer's step needs beyond the losses (video-interpolation/trainer.py:47-132):
//   flow_epe     end-point error against ground truth, trainer.py:58, 97, 110
//   splat_mask   mask * (splat != 0) with the channel broadcast, trainer.py:64, 68
//   flow2img     Middlebury colour coding of a flow field, my_utils/flow_viz.py:6-77, for a batch, on the device
// The formula blocks are in include/sininn.h; DESIGN 16 has the launch plan.
//
// Every reduction is a per-block partial written to a caller-provided buffer and then combined by ONE wave in a fixed order: no
// floating-point atomics, two calls on the same inputs bitwise equal, and the partial buffer needs no initialisation (every slot a
// finish kernel reads has been written by the pass before it).
#include "common.h"

// every operation below is rounded once, as the numpy / torch expressions these kernels restate are: no contraction into FMAs
#pragma clang fp contract(off)

namespace sininn {

namespace {

constexpr int FT_THREADS = 256;          // one pixel per thread: consecutive lanes read consecutive floats of a channel plane
constexpr int FT_WAVES = FT_THREADS / 64;
constexpr int F2I_PIX = 1024;            // pixels of one frame per block in flow2img pass 1 (four per thread)

// sum over the block in a fixed order (xor butterfly inside a wave, then the four waves as (0 + 1) + (2 + 3)); valid in thread 0
__device__ __forceinline__ double ft_block_sum(double v, double* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// ---- end-point error ------------------------------------------------------------------------------------------------------------

// pixel p of the flat (n, h, w) index: sample s = p / hw, r = p % hw.  Per-pixel arithmetic is fp32 with every operation rounded
// once (no contraction into FMAs): the value is what torch's elementwise fp32 ops give; the sum is carried in double from there.
__global__ __launch_bounds__(FT_THREADS) void flow_epe_kernel(const float* __restrict__ flow, int64_t flow_stride,
                                                              const float* __restrict__ gt, int64_t total, int64_t hw,
                                                              double* __restrict__ part) {
  __shared__ double lds[FT_WAVES];
  const int64_t p = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
  double e = 0.0;
  if (p < total) {
    const int64_t s = p / hw, r = p - s * hw;
    const float* f = flow + s * flow_stride + r;
    const float* g = gt + s * 2 * hw + r;
    const float du = f[0] - g[0], dv = f[hw] - g[hw];
    e = (double)sqrtf(du * du + dv * dv);
  }
  const double sum = ft_block_sum(e, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// one wave: lane j adds partials j, j + 64, ... in index order, then the butterfly; mean rounded to fp32 once
__global__ __launch_bounds__(64) void flow_epe_finish_kernel(const double* __restrict__ part, int64_t n_part, double total,
                                                             float* __restrict__ out) {
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n_part; i += 64) acc += part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (threadIdx.x == 0) *out = (float)(acc / total);
}

// ---- mask * (splat != 0) --------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(FT_THREADS) void splat_mask_kernel(const float* __restrict__ mask, int cm, const float* __restrict__ splat,
                                                                int64_t total, int64_t hw, int c, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * FT_THREADS) {
    const int64_t plane = i / hw, r = i - plane * hw;      // plane = n * c + ch
    const int64_t s = plane / c;
    const int ch = (int)(plane - s * c);
    const float m = mask[(s * cm + ch % cm) * hw + r];
    out[i] = m * (splat[i] != 0.f ? 1.f : 0.f);            // a product, not a select: a NaN in the mask stays a NaN, as in torch
  }
}

// ---- flow2img -------------------------------------------------------------------------------------------------------------------

constexpr float F2I_UNKNOWN = 1e7f;
constexpr double F2I_EPS = 2.220446049250313e-16;
constexpr int F2I_NCOLS = 55;

// clip, zero the unknown flows (flow_viz.py:12-20).  fminf / fmaxf would drop a NaN; numpy's clip keeps it.
__device__ __forceinline__ float f2i_clip(float x, float clip) { return x != x ? x : fminf(fmaxf(x, -clip), clip); }
__device__ __forceinline__ void f2i_load(const float* __restrict__ f, int64_t hw, int64_t r, float clip, float& u, float& v, bool& unknown) {
  u = f2i_clip(f[r], clip);
  v = f2i_clip(f[hw + r], clip);
  unknown = fabsf(u) > F2I_UNKNOWN || fabsf(v) > F2I_UNKNOWN;
  if (unknown) u = v = 0.f;
}
__device__ __forceinline__ float f2i_rad(float u, float v) {
  return sqrtf(u * u + v * v);                             // numpy float32: u ** 2, v ** 2, the sum and the root each rounded once
}

// numpy's max: NaN if any element is NaN.  A partial is NaN or the maximum of its elements.
__device__ __forceinline__ float f2i_nanmax(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }

// pass 1: grid (blocks per frame, n); part[frame][block] = nan-propagating max of the radius over F2I_PIX pixels
__global__ __launch_bounds__(FT_THREADS) void flow2img_maxrad_kernel(const float* __restrict__ flow, int64_t hw, float clip,
                                                                     float* __restrict__ part) {
  __shared__ float lds[FT_WAVES];
  const float* f = flow + (int64_t)blockIdx.y * 2 * hw;
  float m = 0.f;                                           // radii are >= 0: 0 is the identity of this maximum
  const int64_t base = (int64_t)blockIdx.x * F2I_PIX;
#pragma unroll
  for (int k = 0; k < F2I_PIX / FT_THREADS; ++k) {
    const int64_t r = base + k * FT_THREADS + threadIdx.x;
    if (r < hw) {
      float u, v; bool unknown;
      f2i_load(f, hw, r, clip, u, v, unknown);
      m = f2i_nanmax(m, f2i_rad(u, v));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = f2i_nanmax(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = f2i_nanmax(f2i_nanmax(lds[0], lds[1]), f2i_nanmax(lds[2], lds[3]));
}

// one wave per frame: maxrad = max(-1, rad.max()) as Python's max evaluates it: a NaN maximum compares false and gives -1
__global__ __launch_bounds__(64) void flow2img_maxrad_finish_kernel(const float* __restrict__ part, int bpf, float* __restrict__ maxrad) {
  const float* p = part + (int64_t)blockIdx.x * bpf;
  float m = 0.f;
  for (int i = threadIdx.x; i < bpf; i += 64) m = f2i_nanmax(m, p[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = f2i_nanmax(m, __shfl_xor(m, o));
  if (threadIdx.x == 0) maxrad[blockIdx.x] = m > -1.f ? m : -1.f;
}

// pass 2: the colour wheel (flow_viz.py:24-32 and compute_color, 35-77).  The division by maxrad is numpy float32; everything from
// the `+ eps` on is float64.  wheel: [55][3] doubles, 0..255.
__global__ __launch_bounds__(FT_THREADS) void flow2img_colour_kernel(const float* __restrict__ flow, int64_t hw, float clip,
                                                                     const float* __restrict__ maxrad, const double* __restrict__ wheel,
                                                                     uint8_t* __restrict__ img) {
  __shared__ double w[F2I_NCOLS * 3];
  for (int i = threadIdx.x; i < F2I_NCOLS * 3; i += FT_THREADS) w[i] = wheel[i];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
  if (r >= hw) return;
  const float* f = flow + (int64_t)blockIdx.y * 2 * hw;
  uint8_t* o = img + (int64_t)blockIdx.y * 3 * hw + r;
  float uf, vf; bool unknown;
  f2i_load(f, hw, r, clip, uf, vf, unknown);
  const float mr = maxrad[blockIdx.y];
  double u = (double)(uf / mr) + F2I_EPS, v = (double)(vf / mr) + F2I_EPS;
  const bool isnan = u != u || v != v;
  if (isnan) u = v = 0.0;
  const double rad = sqrt(u * u + v * v);
  const double a = atan2(-v, -u) / 3.141592653589793;
  const double fk = (a + 1.0) / 2.0 * (double)(F2I_NCOLS - 1) + 1.0;
  int k0 = (int)floor(fk);
  int k1 = k0 + 1;
  if (k1 == F2I_NCOLS + 1) k1 = 1;
  const double fr = fk - (double)k0;
  k0 = min(max(k0, 1), F2I_NCOLS);                         // fk lies in [1, 55]; the clamps only keep a table index in range
  k1 = min(max(k1, 1), F2I_NCOLS);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double col0 = w[(k0 - 1) * 3 + c] / 255.0, col1 = w[(k1 - 1) * 3 + c] / 255.0;
    double col = (1.0 - fr) * col0 + fr * col1;
    if (rad <= 1.0) col = 1.0 - rad * (1.0 - col); else col = col * 0.75;
    const double level = floor(255.0 * col * (isnan ? 0.0 : 1.0));
    o[(int64_t)c * hw] = unknown ? (uint8_t)0 : (uint8_t)(int)level;
  }
}

constexpr int64_t FT_MAX_PIXELS = (int64_t)1 << 40;

static inline int ft_dims_ok(int n, int h, int w) { return n > 0 && h > 0 && w > 0 && (int64_t)n * h * w <= FT_MAX_PIXELS; }

}  // namespace

int64_t flow_epe_partials(int n, int h, int w) {
  if (!ft_dims_ok(n, h, w)) return 0;
  return ((int64_t)n * h * w + FT_THREADS - 1) / FT_THREADS;
}

int flow_epe_launch(const float* flow, int64_t flow_sample_stride, const float* gt, int n, int h, int w, double* partials,
                    int64_t n_partials, float* out, hipStream_t st) {
  SININN_CHECK(flow && gt && partials && out, "flow_epe: null pointer");
  SININN_CHECK(ft_dims_ok(n, h, w), "flow_epe: bad extents n=%d h=%d w=%d", n, h, w);
  const int64_t hw = (int64_t)h * w, total = (int64_t)n * hw;
  SININN_CHECK(flow_sample_stride >= 2 * hw, "flow_epe: sample stride %lld is smaller than two channel planes (%lld)",
               (long long)flow_sample_stride, (long long)(2 * hw));
  const int64_t blocks = flow_epe_partials(n, h, w);
  SININN_CHECK(blocks <= 0x7fffffff, "flow_epe: %lld pixels need more blocks than one launch has", (long long)total);
  SININN_CHECK(n_partials >= blocks, "flow_epe: the partial-sum buffer holds %lld doubles, needs %lld", (long long)n_partials,
               (long long)blocks);
  SININN_CHECK((reinterpret_cast<uintptr_t>(partials) & 7u) == 0 && (reinterpret_cast<uintptr_t>(flow) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(gt) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0, "flow_epe: misaligned pointer");
  hipLaunchKernelGGL(flow_epe_kernel, dim3((unsigned)blocks), dim3(FT_THREADS), 0, st, flow, flow_sample_stride, gt, total, hw, partials);
  SININN_LAUNCH_CHECK("flow_epe");
  hipLaunchKernelGGL(flow_epe_finish_kernel, dim3(1), dim3(64), 0, st, partials, blocks, (double)total, out);
  SININN_LAUNCH_CHECK("flow_epe_finish");
  return 0;
}

int splat_mask_launch(const float* mask, int mask_channels, const float* splat, int n, int c, int h, int w, float* out, hipStream_t st) {
  SININN_CHECK(mask && splat && out, "splat_mask: null pointer");
  SININN_CHECK(ft_dims_ok(n, h, w), "splat_mask: bad extents n=%d h=%d w=%d", n, h, w);
  SININN_CHECK(c == 3, "splat_mask: the splat has 3 channels (got %d)", c);
  SININN_CHECK(mask_channels == 1 || mask_channels == 3, "splat_mask: the mask has 1 or 3 channels (got %d)", mask_channels);
  const int64_t hw = (int64_t)h * w, total = (int64_t)n * c * hw;
  int64_t blocks = (total + FT_THREADS - 1) / FT_THREADS;
  if (blocks > 8192) blocks = 8192;                        // grid-stride beyond that: 32 blocks per CU
  hipLaunchKernelGGL(splat_mask_kernel, dim3((unsigned)blocks), dim3(FT_THREADS), 0, st, mask, mask_channels, splat, total, hw, c, out);
  SININN_LAUNCH_CHECK("splat_mask");
  return 0;
}

int64_t flow2img_workspace_floats(int n, int h, int w) {
  if (!ft_dims_ok(n, h, w)) return 0;
  const int64_t bpf = ((int64_t)h * w + F2I_PIX - 1) / F2I_PIX;
  return (int64_t)n * bpf + n;                             // the partial maxima, then maxrad per frame
}

int flow2img_launch(const float* flow, int n, int h, int w, float clip, const double* wheel, int wheel_rows, float* workspace,
                    int64_t workspace_floats, uint8_t* img, hipStream_t st) {
  SININN_CHECK(flow && wheel && workspace && img, "flow2img: null pointer");
  SININN_CHECK(ft_dims_ok(n, h, w), "flow2img: bad extents n=%d h=%d w=%d", n, h, w);
  SININN_CHECK(wheel_rows == F2I_NCOLS, "flow2img: the colour wheel has %d rows (got %d)", F2I_NCOLS, wheel_rows);
  SININN_CHECK(clip >= 0.f, "flow2img: clip must be >= 0 (got %g)", (double)clip);
  SININN_CHECK((reinterpret_cast<uintptr_t>(wheel) & 7u) == 0 && (reinterpret_cast<uintptr_t>(flow) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "flow2img: misaligned pointer");
  const int64_t hw = (int64_t)h * w;
  const int64_t bpf = (hw + F2I_PIX - 1) / F2I_PIX, cblocks = (hw + FT_THREADS - 1) / FT_THREADS;
  SININN_CHECK(n <= 65535, "flow2img: at most 65535 frames per call (got %d)", n);
  SININN_CHECK(cblocks <= 0x7fffffff, "flow2img: a frame of %lld pixels needs more blocks than one launch has", (long long)hw);
  const int64_t need = flow2img_workspace_floats(n, h, w);
  SININN_CHECK(workspace_floats >= need, "flow2img: workspace holds %lld floats, needs %lld", (long long)workspace_floats, (long long)need);
  float* part = workspace;
  float* maxrad = workspace + (int64_t)n * bpf;
  hipLaunchKernelGGL(flow2img_maxrad_kernel, dim3((unsigned)bpf, (unsigned)n), dim3(FT_THREADS), 0, st, flow, hw, clip, part);
  SININN_LAUNCH_CHECK("flow2img_maxrad");
  hipLaunchKernelGGL(flow2img_maxrad_finish_kernel, dim3((unsigned)n), dim3(64), 0, st, part, (int)bpf, maxrad);
  SININN_LAUNCH_CHECK("flow2img_maxrad_finish");
  hipLaunchKernelGGL(flow2img_colour_kernel, dim3((unsigned)cblocks, (unsigned)n), dim3(FT_THREADS), 0, st, flow, hw, clip, maxrad, wheel, img);
  SININN_LAUNCH_CHECK("flow2img_colour");
  return 0;
}

}  // namespace sininn
