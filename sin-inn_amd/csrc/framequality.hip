// Frame quality: PSNR and mean SSIM (Wang et al. 2004) of predicted frames against real ones, per frame.
//   sqerr[b] = sum_{c,y,x} (p - t)^2                     difference and square each rounded once in fp32, the sum carried in double
//   mse = sqerr / (C H W),  psnr = 10 log10(1 / mse)     data range 1; +inf where mse == 0
//   ssim[b]  = mean over channels and the (H - 10)(W - 10) valid 11 x 11 windows of
//              ((2 mu_p mu_t + C1)(2 s_pt + C2)) / ((mu_p^2 + mu_t^2 + C1)(s_p + s_t + C2)),   C1 = 0.01^2, C2 = 0.03^2
//              mu, E[pp], E[tt], E[pt]: the Gaussian-filtered moments (sigma 1.5, separable, horizontal then vertical),
//              s_p = E[pp] - mu_p^2, s_t = E[tt] - mu_t^2, s_pt = E[pt] - mu_p mu_t
// Two launches.  A block takes one FQ_TY x FQ_TX tile of windows of one (b, c) plane: it stages the tile and its 10-pixel halo of
// both frames in LDS once, filters rows, then columns, evaluates SSIM, and writes ONE partial (two doubles) to the workspace; the
// finish kernel adds a frame's partials in index order.  No atomics: equal inputs give equal bits, and a frame's results depend
// on nothing but that frame.  Pixel (y, x) is counted in sqerr by the tile (min(y / FQ_TY, tiles_y - 1), min(x / FQ_TX, tiles_x - 1)):
// the last tile row and column also own the frame's last 10 rows and columns (all inside their halo), every pixel exactly once.
// No loop is grid-strided: one block per tile.
#include "common.h"
#include "bilinear_taps.h"

namespace sininn {

constexpr int FQ_TY = 16, FQ_TX = 32;                 // the window tile of one block
constexpr int FQ_WIN = 11, FQ_HALO = FQ_WIN - 1;
constexpr int FQ_SY = FQ_TY + FQ_HALO, FQ_SX = FQ_TX + FQ_HALO, FQ_SP = FQ_SX + 1;   // staged rows, columns, row pitch
constexpr int FQ_THREADS = 256;
constexpr int FQ_FINISH_THREADS = 256;
static_assert(FQ_THREADS == FQ_TX * FQ_TY / 2, "a thread evaluates two vertically adjacent windows");

struct FqWindow { float g[FQ_WIN]; };

// a fixed-order sum over the block: the tree is the same whatever the data
__device__ __forceinline__ double fq_block_sum(double v, double* red, int tid, int threads) {
  red[tid] = v;
  __syncthreads();
  for (int s = threads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

__global__ __launch_bounds__(FQ_THREADS) void frame_quality_tile_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                        int H, int W, int tiles_y, int tiles_x, int quantize,
                                                                        FqWindow win, double* __restrict__ partials,
                                                                        float* __restrict__ ssim_map) {
  __shared__ float sp[FQ_SY][FQ_SP], st[FQ_SY][FQ_SP];
  __shared__ float hz[5][FQ_SY][FQ_TX];
  __shared__ double red[FQ_THREADS];
  const int tid = threadIdx.x;
  int64_t q = blockIdx.x;
  const int tx = (int)(q % tiles_x); q /= tiles_x;
  const int ty = (int)(q % tiles_y);
  const int64_t plane = q / tiles_y;                    // b * C + c
  const int y0 = ty * FQ_TY, x0 = tx * FQ_TX;
  const int wins_y = H - FQ_HALO, wins_x = W - FQ_HALO;
  const float* pp = pred + plane * H * W;
  const float* tp = target + plane * H * W;
  // what this tile owns of the frame for the squared error: its FQ_TY x FQ_TX pixels, and in the last tile row / column everything
  // up to the frame's edge
  const int own_y = ty == tiles_y - 1 ? FQ_SY : FQ_TY, own_x = tx == tiles_x - 1 ? FQ_SX : FQ_TX;

  double sq = 0.0;
  for (int i = tid; i < FQ_SY * FQ_SX; i += FQ_THREADS) {
    const int ly = i / FQ_SX, lx = i % FQ_SX;
    const int y = y0 + ly, x = x0 + lx;
    float p = 0.f, t = 0.f;
    if (y < H && x < W) {
      p = pp[(int64_t)y * W + x];
      t = tp[(int64_t)y * W + x];
      if (quantize) {
        const float bp = frame_byte(p), bt = frame_byte(t);
        if (ly < own_y && lx < own_x) {
          const int d = (int)bp - (int)bt;
          sq += (double)(d * d);                        // integers: every sum of them below 2^53 is exact
        }
        p = __fdiv_rn(bp, 255.f);
        t = __fdiv_rn(bt, 255.f);
      } else if (ly < own_y && lx < own_x) {
        const float d = __fsub_rn(p, t);
        sq += (double)__fmul_rn(d, d);
      }
    }
    sp[ly][lx] = p;
    st[ly][lx] = t;
  }
  __syncthreads();

  // rows: the five moments of every staged row at every window column of the tile
  for (int i = tid; i < FQ_SY * FQ_TX; i += FQ_THREADS) {
    const int r = i / FQ_TX, x = i % FQ_TX;
    float mp = 0.f, mt = 0.f, epp = 0.f, ett = 0.f, ept = 0.f;
#pragma unroll
    for (int k = 0; k < FQ_WIN; ++k) {
      const float p = sp[r][x + k], t = st[r][x + k], g = win.g[k];
      mp = __fmaf_rn(g, p, mp);
      mt = __fmaf_rn(g, t, mt);
      epp = __fmaf_rn(g, __fmul_rn(p, p), epp);
      ett = __fmaf_rn(g, __fmul_rn(t, t), ett);
      ept = __fmaf_rn(g, __fmul_rn(p, t), ept);
    }
    hz[0][r][x] = mp; hz[1][r][x] = mt; hz[2][r][x] = epp; hz[3][r][x] = ett; hz[4][r][x] = ept;
  }
  __syncthreads();

  // columns: a thread takes window rows 2 j and 2 j + 1 of one window column, which share 10 of their 12 filtered rows
  const int lx = tid % FQ_TX, j = tid / FQ_TX;
  float m[2][5];
#pragma unroll
  for (int w = 0; w < 2; ++w)
#pragma unroll
    for (int a = 0; a < 5; ++a) m[w][a] = 0.f;
#pragma unroll
  for (int k = 0; k <= FQ_WIN; ++k) {
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      const float v = hz[a][2 * j + k][lx];
      if (k < FQ_WIN) m[0][a] = __fmaf_rn(win.g[k], v, m[0][a]);
      if (k > 0) m[1][a] = __fmaf_rn(win.g[k - 1], v, m[1][a]);
    }
  }
  const float c1 = 1e-4f, c2 = 9e-4f;                   // 0.01^2 and 0.03^2, each rounded to fp32 once
  double ssum = 0.0;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const int wy = y0 + 2 * j + w, wx = x0 + lx;
    if (wy < wins_y && wx < wins_x) {
      // every operation rounded once, nothing contracted: for pred == target numerator and denominator are the same bits
      const float mp = m[w][0], mt = m[w][1];
      const float mpp = __fmul_rn(mp, mp), mtt = __fmul_rn(mt, mt), mpt = __fmul_rn(mp, mt);
      const float s_p = __fsub_rn(m[w][2], mpp), s_t = __fsub_rn(m[w][3], mtt), s_pt = __fsub_rn(m[w][4], mpt);
      const float a1 = __fadd_rn(__fmul_rn(2.f, mpt), c1), a2 = __fadd_rn(__fmul_rn(2.f, s_pt), c2);
      const float b1 = __fadd_rn(__fadd_rn(mpp, mtt), c1), b2 = __fadd_rn(__fadd_rn(s_p, s_t), c2);
      const float s = __fdiv_rn(__fmul_rn(a1, a2), __fmul_rn(b1, b2));
      ssum += (double)s;
      if (ssim_map) ssim_map[(plane * wins_y + wy) * wins_x + wx] = s;
    }
  }
  const double sq_all = fq_block_sum(sq, red, tid, FQ_THREADS);
  const double ss_all = fq_block_sum(ssum, red, tid, FQ_THREADS);
  if (tid == 0) {
    partials[2 * (int64_t)blockIdx.x] = sq_all;
    partials[2 * (int64_t)blockIdx.x + 1] = ss_all;
  }
}

// One block per frame: the frame's partials in index order (a thread takes every FQ_FINISH_THREADS-th, then the block's fixed tree).
__global__ __launch_bounds__(FQ_FINISH_THREADS) void frame_quality_finish_kernel(const double* __restrict__ partials, int per_frame,
                                                                                 double pixels, double windows, int quantize, int B,
                                                                                 double* __restrict__ sqerr, float* __restrict__ out) {
  __shared__ double red[FQ_FINISH_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* part = partials + 2 * (int64_t)b * per_frame;
  double sq = 0.0, ss = 0.0;
  for (int i = tid; i < per_frame; i += FQ_FINISH_THREADS) {
    sq += part[2 * i];
    ss += part[2 * i + 1];
  }
  sq = fq_block_sum(sq, red, tid, FQ_FINISH_THREADS);
  ss = fq_block_sum(ss, red, tid, FQ_FINISH_THREADS);
  if (tid == 0) {
    const double mse = quantize ? sq / (65025.0 * pixels) : sq / pixels;
    sqerr[b] = sq;
    out[b] = (float)mse;
    out[B + b] = mse == 0.0 ? INFINITY : (float)(10.0 * log10(1.0 / mse));
    out[2 * B + b] = (float)(ss / windows);
  }
}

static bool fq_shape_ok(int B, int C, int H, int W) {
  if (B <= 0 || (C != 1 && C != 3) || H < FQ_WIN || W < FQ_WIN) return false;
  return (int64_t)B * C * H * W <= 0x7fffffff;
}

static int64_t fq_blocks(int B, int C, int H, int W) {
  const int64_t tiles_y = (H - FQ_HALO + FQ_TY - 1) / FQ_TY, tiles_x = (W - FQ_HALO + FQ_TX - 1) / FQ_TX;
  return (int64_t)B * C * tiles_y * tiles_x;
}

extern "C" int64_t sininn_frame_quality_workspace_floats(int B, int C, int H, int W) {
  if (!fq_shape_ok(B, C, H, W)) return 0;
  return 4 * fq_blocks(B, C, H, W);                     // two doubles per block
}

extern "C" int sininn_frame_quality(const float* pred, const float* target, int B, int C, int H, int W, int quantize, const float* window,
                                    float* workspace, int64_t workspace_floats, double* sqerr, float* out, float* ssim_map, void* stream) {
  hipStream_t st = ST(stream);
  SININN_CHECK(pred && target && window && workspace && sqerr && out, "frame_quality: null pointer");
  SININN_CHECK(B > 0, "frame_quality: bad shape (B = %d must be positive)", B);
  SININN_CHECK(C == 1 || C == 3, "frame_quality: frames have 1 or 3 channels (got %d)", C);
  SININN_CHECK(H >= FQ_WIN && W >= FQ_WIN, "frame_quality: frames of %d x %d are smaller than the 11 x 11 window", H, W);
  SININN_CHECK(fq_shape_ok(B, C, H, W), "frame_quality: B * C * H * W = %lld is past an int index", (long long)B * C * H * W);
  const int64_t need = sininn_frame_quality_workspace_floats(B, C, H, W);
  SININN_CHECK(workspace_floats >= need, "frame_quality: workspace of %lld floats, need %lld", (long long)workspace_floats,
               (long long)need);
  SININN_CHECK((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(sqerr) & 7u) == 0,
               "frame_quality: workspace and sqerr hold doubles and must be 8-byte aligned");
  FqWindow win;
  for (int k = 0; k < FQ_WIN; ++k) win.g[k] = window[k];
  const int tiles_y = (H - FQ_HALO + FQ_TY - 1) / FQ_TY, tiles_x = (W - FQ_HALO + FQ_TX - 1) / FQ_TX;
  const int64_t blocks = fq_blocks(B, C, H, W);         // <= B C H W <= 2^31 - 1
  double* partials = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(frame_quality_tile_kernel, dim3((unsigned)blocks), dim3(FQ_THREADS), 0, st, pred, target, H, W, tiles_y, tiles_x,
                     quantize ? 1 : 0, win, partials, ssim_map);
  SININN_LAUNCH_CHECK("frame_quality_tile");
  hipLaunchKernelGGL(frame_quality_finish_kernel, dim3((unsigned)B), dim3(FQ_FINISH_THREADS), 0, st, partials, C * tiles_y * tiles_x,
                     (double)C * H * W, (double)C * (H - FQ_HALO) * (W - FQ_HALO), quantize ? 1 : 0, B, sqerr, out);
  SININN_LAUNCH_CHECK("frame_quality_finish");
  return 0;
}

}  // namespace sininn
