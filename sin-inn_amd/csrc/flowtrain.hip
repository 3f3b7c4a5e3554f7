// The three small operators the flow trainer's step needs beyond the losses (video-interpolation/trainer.py:47-132):
//   flow_epe     end-point error against ground truth, trainer.py:58, 97, 110
//   splat_mask   mask * (splat != 0) with the channel broadcast, trainer.py:64, 68
//   flow2img     Middlebury colour coding of a flow field, my_utils/flow_viz.py:6-77, for a batch, on the device
// and the one a spatial controller needs after the step:
//   flow_error_stash   the per-pixel photometric error, added cell by cell to the controller's loss log (progressive_controller.py:596-618)
// The formula blocks are in include/sininn.h; DESIGN 16 has the launch plan.
//
// Every reduction is a per-block partial written to a caller-provided buffer and then combined by ONE wave in a fixed order: no
// floating-point atomics, two calls on the same inputs bitwise equal, and the partial buffer needs no initialisation (every slot a
// finish kernel reads has been written by the pass before it).
#include "common.h"
#include "spatial_cells.h"

// every operation below is rounded once, as the numpy / torch expressions these kernels restate are: no contraction into FMAs
#pragma clang fp contract(off)

namespace sininn {

namespace {

constexpr int FT_THREADS = 256;          // one pixel per thread: consecutive lanes read consecutive floats of a channel plane
constexpr int FT_WAVES = FT_THREADS / 64;
constexpr int F2I_PIX = 1024;            // pixels of one frame per block in flow2img pass 1 (four per thread)

static_assert(FT_WAVES == 4, "block_sum_f64 adds four waves");

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
  const double sum = block_sum_f64(e, lds);
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

// ---- the per-pixel photometric error and its stash into a spatial controller's loss log -----------------------------
//
//   E[b][y][x]        = 0.5 (mean_c |m1 S1 - m1 I1| + mean_c |m2 S2 - m2 I2|)
//   log_buffer[cell] += sum over points p = (b, y, x) and corners k with cell(p, k) == cell of alpha(p, k) E[p]
//   log_counter[cell] += the same sum of alpha(p, k)
//
// A corner is one choice of the lower or upper cell per axis (axis_cell, spatial_cells.h); alpha = a_t a_y a_x and
// cell = i_t + res (i_y + res i_x), so both sums factor axis by axis and three launches walk them from the inside out:
//   1  error_rows     one block per (x tile, y, b): E of ES_TX pixels of a row, written once (if asked for), and
//                     R1[b][y][tile][ix] = sum_x a_x E over the pixels whose lower / upper x cell is ix
//   2  error_columns  one block per (iy, b): R2[b][iy][ix] = sum_y a_y sum_tile R1[b][y][tile][ix]; the extra row of blocks b == B
//                     sums the weights of the two pixel axes, Cy[iy] and Cx[ix]
//   3  error_frames   one thread per cell: log_buffer += sum_b a_t R2[b][iy][ix], log_counter += (Ct[it] Cy[iy]) Cx[ix], b in index order
// Every sum has a fixed order: a lane adds its terms in index order, then the xor butterfly, then the waves as (0 + 1) + (2 + 3).  No
// atomics.  Nothing depends on the axes being monotone: a cell is found by comparing indices, and the 64-pixel chunks a cell cannot
// occur in (its index outside the chunk's range of cells, which for a monotone axis leaves two or three chunks) are skipped whole.
constexpr int ES_TX = 1024;                  // pixels of one row per block: four per thread
constexpr int ES_CHUNKS = ES_TX / 64;
constexpr int ES_MAX_RES = 1024;             // res^3 cells fit an int; a cell index fits the 16-bit halves of the packed pair

struct StashDev {
  const float *s1, *i1, *m1, *s2, *i2, *m2;
  const float *times, *ys, *xs;
  int cm, B, H, W, ntiles;
  Spatial sp;
};

// mean over the channels of |m S - m I| at pixel r of sample b: each product, difference and sum rounded once, ((d0 + d1) + d2) / C.
// 64-bit: (b C + c) H W + r reaches 2^31 from 179 M pixels on.
template <int C>
__device__ __forceinline__ float es_direction(const float* __restrict__ s, const float* __restrict__ i, const float* __restrict__ m,
                                              int cm, int64_t b, int64_t hw, int64_t r) {
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float mk = m[(b * cm + (cm == 1 ? 0 : c)) * hw + r];
    const int64_t at = (b * C + c) * hw + r;
    const float d = fabsf(s[at] * mk - i[at] * mk);
    sum = c == 0 ? d : sum + d;
  }
  return sum / (float)C;
}

template <int C>
__global__ __launch_bounds__(FT_THREADS) void error_rows_kernel(const StashDev q, float* __restrict__ r1, float* __restrict__ e_out) {
  __shared__ float v0[ES_TX], v1[ES_TX];     // a_x E towards the lower and the upper x cell of each pixel
  __shared__ int cells[ES_TX];               // lower | upper << 16; -1 past the end of the row
  __shared__ int clo[ES_CHUNKS], chi[ES_CHUNKS];
  const int tile = blockIdx.x, y = blockIdx.y, b = blockIdx.z;
  const int x0 = tile * ES_TX, n = min(ES_TX, q.W - x0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t hw = (int64_t)q.H * q.W, row = (int64_t)y * q.W + x0;
#pragma unroll
  for (int j = 0; j < ES_TX / FT_THREADS; ++j) {
    const int l = j * FT_THREADS + threadIdx.x;
    float e0 = 0.f, e1 = 0.f;
    int packed = -1, lo = ES_MAX_RES, hi = -1;
    if (l < n) {
      const int64_t r = row + l;
      const float e = 0.5f * (es_direction<C>(q.s1, q.i1, q.m1, q.cm, b, hw, r) + es_direction<C>(q.s2, q.i2, q.m2, q.cm, b, hw, r));
      if (e_out) e_out[(int64_t)b * hw + r] = e;
      const AxisCell cx = axis_cell(q.sp, 2, q.xs[x0 + l]);
      e0 = cx.a[0] * e;
      e1 = cx.a[1] * e;
      packed = cx.i[0] | (cx.i[1] << 16);
      lo = min(cx.i[0], cx.i[1]);
      hi = max(cx.i[0], cx.i[1]);
    }
    v0[l] = e0;
    v1[l] = e1;
    cells[l] = packed;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o));
      hi = max(hi, __shfl_xor(hi, o));
    }
    if (lane == 0) { clo[j * FT_WAVES + wave] = lo; chi[j * FT_WAVES + wave] = hi; }   // wave `wave` filled chunk j * FT_WAVES + wave
  }
  __syncthreads();
  float* out = r1 + (((int64_t)b * q.H + y) * q.ntiles + tile) * q.sp.res;
  for (int ix = wave; ix < q.sp.res; ix += FT_WAVES) {
    float acc = 0.f;
    for (int k = 0; k < ES_CHUNKS; ++k) {
      if (ix < clo[k] || ix > chi[k]) continue;            // wave-uniform
      const int l = k * 64 + lane, c = cells[l];
      acc += ((c & 0xffff) == ix ? v0[l] : 0.f) + ((c >> 16) == ix ? v1[l] : 0.f);   // c == -1: neither half is a cell
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) out[ix] = acc;
  }
}

// the sum of the weights along one pixel axis towards cell `cell`: lane j adds coordinates j, j + 64, ... in index order, then the butterfly
__device__ __forceinline__ float es_axis_weight(const Spatial& sp, int d, const float* __restrict__ axis, int n, int cell, int lane) {
  float acc = 0.f;
  for (int p = lane; p < n; p += 64) {
    const AxisCell c = axis_cell(sp, d, axis[p]);
    acc += (c.i[0] == cell ? c.a[0] : 0.f) + (c.i[1] == cell ? c.a[1] : 0.f);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}

// grid (res, B + 1).  Thread (slot, part) = (threadIdx.x & 63, threadIdx.x >> 6): x cells slot, slot + 64, ...; rows part, part + 4, ...
__global__ __launch_bounds__(FT_THREADS) void error_columns_kernel(const StashDev q, const float* __restrict__ r1, float* __restrict__ r2,
                                                                   float* __restrict__ cy, float* __restrict__ cx) {
  __shared__ float lds[FT_WAVES][64];
  const int iy = blockIdx.x, b = blockIdx.y, res = q.sp.res;
  const int slot = threadIdx.x & 63, part = threadIdx.x >> 6;
  if (b == q.B) {                                          // the weights of the pixel axes: wave 0 the rows, wave 1 the columns
    if (part == 0) { const float s = es_axis_weight(q.sp, 1, q.ys, q.H, iy, slot); if (slot == 0) cy[iy] = s; }
    if (part == 1) { const float s = es_axis_weight(q.sp, 2, q.xs, q.W, iy, slot); if (slot == 0) cx[iy] = s; }
    return;
  }
  for (int base = 0; base < res; base += 64) {             // block-uniform trip count: the barriers below are reached by every thread
    const int ix = base + slot;
    float acc = 0.f;
    for (int y = part; y < q.H; y += FT_WAVES) {
      const AxisCell c = axis_cell(q.sp, 1, q.ys[y]);
      if (c.i[0] != iy && c.i[1] != iy) continue;          // wave-uniform: y and iy are
      if (ix < res) {
        const float* p = r1 + (((int64_t)b * q.H + y) * q.ntiles) * res + ix;
        float row = p[0];
        for (int t = 1; t < q.ntiles; ++t) row += p[(int64_t)t * res];
        if (c.i[0] == iy) acc += c.a[0] * row;
        if (c.i[1] == iy) acc += c.a[1] * row;
      }
    }
    lds[part][slot] = acc;
    __syncthreads();
    if (part == 0 && ix < res) r2[((int64_t)b * res + iy) * res + ix] = (lds[0][slot] + lds[1][slot]) + (lds[2][slot] + lds[3][slot]);
    __syncthreads();
  }
}

// one thread per cell, i_t fastest (the layout of the log): consecutive lanes write consecutive floats and read one R2 value
__global__ __launch_bounds__(FT_THREADS) void error_frames_kernel(const StashDev q, const float* __restrict__ r2, const float* __restrict__ cy,
                                                                  const float* __restrict__ cx, float* __restrict__ log_buffer,
                                                                  float* __restrict__ log_counter) {
  const int res = q.sp.res, cell = blockIdx.x * FT_THREADS + threadIdx.x;
  if (cell >= res * res * res) return;
  const int it = cell % res, rest = cell / res;            // rest = i_y + res i_x
  const int iy = rest % res, ix = rest / res;
  float acc = 0.f, ct = 0.f;
  for (int b = 0; b < q.B; ++b) {
    const AxisCell c = axis_cell(q.sp, 0, q.times[b]);
    if (c.i[0] != it && c.i[1] != it) continue;
    const float v = r2[((int64_t)b * res + iy) * res + ix];
    if (c.i[0] == it) { acc += c.a[0] * v; ct += c.a[0]; }
    if (c.i[1] == it) { acc += c.a[1] * v; ct += c.a[1]; }
  }
  log_buffer[cell] += acc;
  log_counter[cell] += (ct * cy[iy]) * cx[ix];
}

static inline int64_t es_tiles(int w) { return ((int64_t)w + ES_TX - 1) / ES_TX; }

}  // namespace

extern "C" int64_t sininn_flow_epe_partials(int n, int h, int w) {
  if (!ft_dims_ok(n, h, w)) return 0;
  return ((int64_t)n * h * w + FT_THREADS - 1) / FT_THREADS;
}

extern "C" int sininn_flow_epe(const float* flow, int64_t flow_sample_stride, const float* gt, int n, int h, int w, double* partials,
                               int64_t n_partials, float* out, void* stream) {
  hipStream_t st = ST(stream);
  SININN_CHECK(flow && gt && partials && out, "flow_epe: null pointer");
  SININN_CHECK(ft_dims_ok(n, h, w), "flow_epe: bad extents n=%d h=%d w=%d", n, h, w);
  const int64_t hw = (int64_t)h * w, total = (int64_t)n * hw;
  SININN_CHECK(flow_sample_stride >= 2 * hw, "flow_epe: sample stride %lld is smaller than two channel planes (%lld)",
               (long long)flow_sample_stride, (long long)(2 * hw));
  const int64_t blocks = sininn_flow_epe_partials(n, h, w);
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

extern "C" int sininn_splat_mask(const float* mask, int mask_channels, const float* splat, int n, int c, int h, int w, float* out, void* stream) {
  hipStream_t st = ST(stream);
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

extern "C" int64_t sininn_flow_error_stash_workspace_floats(int B, int H, int W, int res) {
  if (!ft_dims_ok(B, H, W) || res < 3 || res > ES_MAX_RES) return 0;
  return (int64_t)B * H * es_tiles(W) * res + (int64_t)B * res * res + 2 * (int64_t)res;   // R1, R2, Cy, Cx
}

extern "C" int sininn_flow_error_stash(const float* softmax1, const float* frame1, const float* mask1, const float* softmax2,
                                       const float* frame2, const float* mask2, int mask_channels, int B, int C, int H, int W,
                                       const float* times, const float* ys, const float* xs, int res, float centre_t, float centre_y,
                                       float centre_x, float scale_t, float scale_y, float scale_x, float* log_buffer, float* log_counter,
                                       float* e_out, float* workspace, int64_t workspace_floats, void* stream) {
  hipStream_t st = ST(stream);
  const float centre[3] = {centre_t, centre_y, centre_x}, scale[3] = {scale_t, scale_y, scale_x};
  SININN_CHECK(softmax1 && frame1 && mask1 && softmax2 && frame2 && mask2 && times && ys && xs && log_buffer && log_counter && workspace,
               "flow_error_stash: null pointer");
  SININN_CHECK(ft_dims_ok(B, H, W), "flow_error_stash: bad extents B=%d H=%d W=%d", B, H, W);
  SININN_CHECK(res >= 3 && res <= ES_MAX_RES, "flow_error_stash: res must be 3..%d (got %d)", ES_MAX_RES, res);
  SININN_CHECK(C == 1 || C == 3, "flow_error_stash: the frames have 1 or 3 channels (got %d)", C);
  SININN_CHECK(mask_channels == 1 || mask_channels == C, "flow_error_stash: the masks have 1 or %d channels (got %d)", C, mask_channels);
  SININN_CHECK(H <= 65535 && B < 65535, "flow_error_stash: at most 65535 rows and 65534 frames per call (got H=%d B=%d)", H, B);
  const int64_t need = sininn_flow_error_stash_workspace_floats(B, H, W, res);
  SININN_CHECK(workspace_floats >= need, "flow_error_stash: workspace holds %lld floats, needs %lld", (long long)workspace_floats,
               (long long)need);
  const float* const ptrs[] = {softmax1, frame1, mask1, softmax2, frame2, mask2, times, ys, xs, log_buffer, log_counter, e_out, workspace};
  for (const float* p : ptrs) SININN_CHECK((reinterpret_cast<uintptr_t>(p) & 3u) == 0, "flow_error_stash: misaligned pointer");
  StashDev q{softmax1, frame1, mask1, softmax2, frame2, mask2, times, ys, xs, mask_channels, B, H, W, (int)es_tiles(W),
             Spatial{nullptr, res, (float)(res - 2 > 1 ? res - 2 : 1), {centre[0], centre[1], centre[2]}, {scale[0], scale[1], scale[2]}}};
  float* r1 = workspace;
  float* r2 = r1 + (int64_t)B * H * q.ntiles * res;
  float* cy = r2 + (int64_t)B * res * res;
  float* cx = cy + res;
  const dim3 rows((unsigned)q.ntiles, (unsigned)H, (unsigned)B);
  if (C == 3) hipLaunchKernelGGL(error_rows_kernel<3>, rows, dim3(FT_THREADS), 0, st, q, r1, e_out);
  else hipLaunchKernelGGL(error_rows_kernel<1>, rows, dim3(FT_THREADS), 0, st, q, r1, e_out);
  SININN_LAUNCH_CHECK("flow_error_rows");
  hipLaunchKernelGGL(error_columns_kernel, dim3((unsigned)res, (unsigned)B + 1), dim3(FT_THREADS), 0, st, q, r1, r2, cy, cx);
  SININN_LAUNCH_CHECK("flow_error_columns");
  const int cells = res * res * res;
  hipLaunchKernelGGL(error_frames_kernel, dim3((unsigned)((cells + FT_THREADS - 1) / FT_THREADS)), dim3(FT_THREADS), 0, st, q, r2, cy, cx,
                     log_buffer, log_counter);
  SININN_LAUNCH_CHECK("flow_error_frames");
  return 0;
}

extern "C" int64_t sininn_flow2img_workspace_floats(int n, int h, int w) {
  if (!ft_dims_ok(n, h, w)) return 0;
  const int64_t bpf = ((int64_t)h * w + F2I_PIX - 1) / F2I_PIX;
  return (int64_t)n * bpf + n;                             // the partial maxima, then maxrad per frame
}

extern "C" int sininn_flow2img(const float* flow, int n, int h, int w, float clip, const double* wheel, int wheel_rows, float* workspace,
                               int64_t workspace_floats, uint8_t* img, void* stream) {
  hipStream_t st = ST(stream);
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
  const int64_t need = sininn_flow2img_workspace_floats(n, h, w);
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
