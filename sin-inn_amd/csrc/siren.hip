// The SIREN flow network (reference: video-interpolation/model.py:123-171, SineLayer / SirenModel with the ModelParams defaults, evaluated
// by FlowTrainer.forward, video-interpolation/trainer.py:37-45):
//     h0 = (t, y, x) of meshgrid(times, ys, xs)                                  N = t h w points
//     u_l = omega (W_l h_{l-1} + b_l),  h_l = sin(u_l)      l = 1 .. 4           W_1 [256][3], W_2..4 [256][256]     (model.py:145-146)
//     out = W_5 h_4 + b_5                                                        W_5 [4][256]                        (model.py:167-171)
//     flows[t][c][y][x] = out[p][c] * scale                                                                          (trainer.py:44)
// fp32 on v_mfma_f32_16x16x4_f32, on the tile, the LDS GEMM and the weight-gradient kernels of flownet.hip (flownet_tile.h).  There is no
// encoding: layer 1 is ONE K group of four, (t, y, x, 0), on the MFMA.  The sine is sinf / sincosf, the accurate full-range functions:
// phases are some 40 rad at initialisation and grow with training.  omega is a run-time argument.
//
// forward   siren_fwd_kernel: block = 256 threads, grid-stride over 64-point tiles, wave w owns hidden columns [64 w, 64 w + 64).  A layer
//           leaves its PHASES u_l in the LDS tile; sine_tile then turns them into h_l in place, 16 bytes per thread at a time, and in
//           training mode copies them to `saved` ([4][Npad][256], all four layers) on the way.  Inference and training run the same code, so
//           their flows are bitwise equal.  Layer 5 is 256 dot products on the vector ALU.
// backward  siren_bwd_chain_kernel, per tile:  dout = dflows * scale;  (sin, cos)(u_4): gW5 / gb5 partials, dz_4 = omega (dout W5) cos(u_4);
//           l = 3, 2, 1:  dh_l = dz_{l+1} W_{l+1} with the forward's GEMM loop on transposed weights, (sin, cos)(u_l): h_l -> workspace (the
//           operand of the next layer's weight gradient), dz_l = omega dh_l cos(u_l) -> workspace (l > 1);  gW1 [256][3] / gb1 partials from
//           the dz_1 tile and the tile's coordinates.  gW_l = dz_l^T h_{l-1}, gb_l (l = 2 .. 4) are flownet.hip's split-over-points kernel and
//           reduce; siren_reduce_kernel adds the chain kernel's per-block partial sums in block order (gb5: each block's double sum
//           travels as two floats and is rounded once, after the blocks are added).  No floating-point atomics: two calls are bitwise
//           equal.
// structure: what this file has of its own is the sine (sine_tile, the sincosf steps of the chain kernel), its descriptor and its partial
//           sums.  From flownet_tile.h come the tile, gemm_lds, mfma_k4 for layer 1, store_acc with the Phase / Plain epilogues, copy_tile_out,
//           stage_coord and the host checks of the point grid, the layers, `saved` and the
//           buffers of a forward / backward call; from flownet.hip the hidden layers' weight gradient (hidden_wgrad_launch).  The output
//           layer, dout, the tile load, the column sums and the transpose kernel match flownet.hip's text but stay spelled out: as helpers
//           they changed the instructions, or the placement, of these kernels.
// points    (SININN_FLOWNET_AT_POINTS) point_coord reads row p of a caller's pose list [N][3] instead of the axis vectors; T = H = 1, W = N makes
//           flows / dflows the planar [4][N].  The same kernels, nothing else differs (see flownet.hip)
// pose gradient (SININN_FLOWNET_POSEGRAD) siren_bwd_chain_kernel<true> also writes g_poses[p][d] = sum_j dz_1[p][j] W1[j][d] from the
//           dz_1 tile it holds at the end of a tile; <false> is the kernel as it was, instruction for instruction
// Rows of the last tile beyond N are computed on a clamped point in the forward pass and carry dout = 0 in the backward pass, so every
// saved / workspace row is written before it is read and contributes exact zeros to every sum.
#include "flownet_tile.h"

namespace sininn {

namespace {

constexpr int SR_IN = 3;
constexpr int SR_SINES = 4;                            // sine layers; SR_SINES + 1 nn.Linears
constexpr size_t SR_LDS = (size_t)(FN_P * FN_HS + FN_P * FN_OUT + FN_P * FN_CS) * sizeof(float);
// one chain block's partial sums: gW1 [256][3], gb1 [256], gW5 [4][256], gb5 [4] as (hi [4], lo [4]): the block's double sum in two
// floats, so that the reduce kernel adds the blocks' sums unrounded
constexpr int SR_PART_GB1 = FN_HID * SR_IN, SR_PART_GW5 = SR_PART_GB1 + FN_HID, SR_PART_GB5 = SR_PART_GW5 + FN_OUT * FN_HID;
constexpr int SR_PART = SR_PART_GB5 + 2 * FN_OUT;

struct SirenDev {
  int T, H, W, N, ntiles;
  float scale, omega;
  const float *times, *ys, *xs;
  const float* poses;      // points mode: [N][3], the coordinates of point p; nullptr: the grid above
  const float* w[SR_SINES + 1];
  const float* b[SR_SINES + 1];
  float* flows;
  float* saved;            // [4][ntiles * 64][256]: the phases u_1 .. u_4, or nullptr (inference)
  const float* dflows;
  float* dz;               // [3][ntiles * 64][256]: dz_2 .. dz_4
  float* hin;              // [3][ntiles * 64][256]: h_1 .. h_3
  const float* wt;         // W2^T, W3^T, W4^T
  float* part;
};

// the descriptor of the chain kernel that also writes the gradient of the coordinates
struct SirenPoseDev : SirenDev {
  float* g_poses;          // [N][3]
};

// acc = W1 (t, y, x) for the tile's points: one K group, k = kq: t, y, x, 0
__device__ __forceinline__ void layer1(const SirenDev& q, int tile, int cw, int li, int kq, f32x4 (&acc)[4][4]) {
  float a[4], b[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const Coord c = point_coord(q, tile * FN_P + 16 * m + li);
    a[m] = kq == 0 ? c.t : kq == 1 ? c.y : kq == 2 ? c.x : 0.f;
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) b[n] = kq < SR_IN ? q.w[0][(cw + 16 * n + li) * SR_IN + kq] : 0.f;
  zero_acc(acc);
  mfma_k4(a, b, acc);
}

// the LDS tile holds phases: (dst != nullptr) copy them to rows [64 tile, 64 tile + 64) of a [Npad][256] array; their sines in place
__device__ __forceinline__ void sine_tile(float* hs, float* dst, int tile, int tid) {
#pragma unroll 2
  for (int u = 0; u < FN_P * FN_HID / 4 / FN_NTHR; ++u) {
    const int f = tid + FN_NTHR * u;
    const int row = f >> 6, c4 = (f & 63) * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(hs + row * FN_HS + c4);
    if (dst) *reinterpret_cast<f32x4*>(dst + ((size_t)tile * FN_P + row) * FN_HID + c4) = v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = sinf(v[j]);
    *reinterpret_cast<f32x4*>(hs + row * FN_HS + c4) = v;
  }
}

__global__ __launch_bounds__(FN_NTHR, 2) void siren_fwd_kernel(SirenDev q) {
  extern __shared__ __attribute__((aligned(16))) float fn_smem[];
  float* const hs = fn_smem;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kq = lane >> 4;
  const int cw = wave * 64;
  const size_t lstride = (size_t)q.ntiles * FN_P * FN_HID;
  const int hw = q.H * q.W;

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    f32x4 acc[4][4];
    layer1(q, tile, cw, li, kq, acc);
    __syncthreads();                       // the previous tile's layer 5 has read hs
    store_acc(hs, cw, li, kq, acc, Phase{q.b[0], q.omega});
    __syncthreads();
    sine_tile(hs, q.saved, tile, tid);
    __syncthreads();
    // ---- layers 2 .. 4 ----
#pragma unroll 1
    for (int l = 1; l < SR_SINES; ++l) {
      zero_acc(acc);
      gemm_lds(hs, q.w[l], cw, li, kq, acc);
      __syncthreads();                     // every wave has read the whole tile
      store_acc(hs, cw, li, kq, acc, Phase{q.b[l], q.omega});
      __syncthreads();
      sine_tile(hs, q.saved ? q.saved + l * lstride : nullptr, tile, tid);
      __syncthreads();
    }
    // ---- layer 5 on the vector ALU: thread = (channel tid / 64, point tid % 64) ----
    {
      const int c = tid >> 6, pl = tid & 63;
      const float* w5 = q.w[SR_SINES] + c * FN_HID;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
      for (int k = 0; k < FN_HID; k += 4) {
        const f32x4 h = *reinterpret_cast<const f32x4*>(hs + pl * FN_HS + k);
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w5 + k);
        a0 = fmaf(h[0], wv[0], a0);
        a1 = fmaf(h[1], wv[1], a1);
        a2 = fmaf(h[2], wv[2], a2);
        a3 = fmaf(h[3], wv[3], a3);
      }
      const int p = tile * FN_P + pl;
      if (p < q.N) {
        const int t = p / hw, rem = p - t * hw;
        q.flows[((size_t)t * FN_OUT + c) * hw + rem] = (((a0 + a1) + (a2 + a3)) + q.b[SR_SINES][c]) * q.scale;
      }
    }
  }
}

// out[k][j] = in[j][k] for W2, W3 and W4 (blockIdx.y): the data-gradient GEMMs then read 16-byte rows like the forward pass does
__global__ __launch_bounds__(FN_NTHR) void siren_transpose_kernel(const float* w2, const float* w3, const float* w4, float* wt) {
  const float* in = blockIdx.y == 0 ? w2 : blockIdx.y == 1 ? w3 : w4;
  float* out = wt + (size_t)blockIdx.y * FN_HID * FN_HID;
  const int j = blockIdx.x, k = threadIdx.x;
  out[k * FN_HID + j] = in[j * FN_HID + k];
}

// POSEGRAD: also g_poses[p][d] = sum_j dz_1[p][j] W1[j][d] from the dz_1 tile (dz_1 = omega v, v the gradient of the layer-1 phase):
// thread = (coordinate tid / 64, point tid % 64), four strided partial sums of 64 terms each, (a0 + a1) + (a2 + a3); rows p >= N are
// not written.  Not POSEGRAD: the kernel as it has always been
template <bool POSEGRAD>
__global__ __launch_bounds__(FN_NTHR, 2) void siren_bwd_chain_kernel(std::conditional_t<POSEGRAD, SirenPoseDev, SirenDev> q) {
  extern __shared__ __attribute__((aligned(16))) float fn_smem[];
  float* const hs = fn_smem;
  float* const dos = fn_smem + FN_P * FN_HS;           // [64][4]: dout of the tile
  float* const cs = dos + FN_P * FN_OUT;               // [64][4]: coordinates of the tile's points
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kq = lane >> 4;
  const int cw = wave * 64;
  const size_t lstride = (size_t)q.ntiles * FN_P * FN_HID;
  const int hw = q.H * q.W;

  float w5k[4], gw5[4] = {0.f, 0.f, 0.f, 0.f}, gw1[SR_IN] = {0.f, 0.f, 0.f}, gb1 = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) w5k[c] = q.w[SR_SINES][c * FN_HID + tid];
  double gb5 = 0.0;                                    // as gb4 of flownet_bwd_chain_kernel: in double

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    __syncthreads();                                   // the previous tile is done with hs / dos / cs
#pragma unroll 4
    for (int u = 0; u < FN_P * FN_HID / 4 / FN_NTHR; ++u) {
      const int f = tid + FN_NTHR * u;
      const int row = f >> 6, c4 = (f & 63) * 4;
      *reinterpret_cast<f32x4*>(hs + row * FN_HS + c4) =
          *reinterpret_cast<const f32x4*>(q.saved + (SR_SINES - 1) * lstride + ((size_t)tile * FN_P + row) * FN_HID + c4);
    }
    {
      const int c = tid >> 6, pl = tid & 63;
      const int p = tile * FN_P + pl;
      float v = 0.f;
      if (p < q.N) {
        const int t = p / hw, rem = p - t * hw;
        v = q.dflows[((size_t)t * FN_OUT + c) * hw + rem] * q.scale;
      }
      dos[pl * FN_OUT + c] = v;
    }
    if (tid < FN_P) stage_coord(q, cs, tile, tid);
    __syncthreads();
    // gW5 += dout^T sin(u4);  dz4 = omega (dout W5) cos(u4) in place: thread = hidden column tid
#pragma unroll 2
    for (int p = 0; p < FN_P; ++p) {
      const f32x4 d = *reinterpret_cast<const f32x4*>(dos + p * FN_OUT);
      float sn, co;
      sincosf(hs[p * FN_HS + tid], &sn, &co);
      float v = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        gw5[c] = fmaf(d[c], sn, gw5[c]);
        v = fmaf(d[c], w5k[c], v);
      }
      hs[p * FN_HS + tid] = q.omega * v * co;
    }
    if (tid < FN_OUT) {
      double s = 0.0;
      for (int p = 0; p < FN_P; ++p) s += (double)dos[p * FN_OUT + tid];
      gb5 += s;
    }
    __syncthreads();
    copy_tile_out(hs, q.dz + (SR_SINES - 2) * lstride, tile, tid);
    // sine layer l + 1 = 3, 2, 1:  dh = dz_{l+2} W_{l+2},  h_{l+1} = sin(u_{l+1}) -> hin[l],  dz_{l+1} = omega dh cos(u_{l+1}) -> dz[l - 1]
#pragma unroll 1
    for (int l = SR_SINES - 2; l >= 0; --l) {
      f32x4 acc[4][4];
      zero_acc(acc);
      gemm_lds(hs, q.wt + (size_t)l * FN_HID * FN_HID, cw, li, kq, acc);
      __syncthreads();
      store_acc(hs, cw, li, kq, acc, Plain{});
      __syncthreads();
#pragma unroll 2
      for (int u = 0; u < FN_P * FN_HID / 4 / FN_NTHR; ++u) {
        const int f = tid + FN_NTHR * u;
        const int row = f >> 6, c4 = (f & 63) * 4;
        const size_t g = ((size_t)tile * FN_P + row) * FN_HID + c4;
        const f32x4 ph = *reinterpret_cast<const f32x4*>(q.saved + l * lstride + g);
        f32x4 v = *reinterpret_cast<const f32x4*>(hs + row * FN_HS + c4), h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float sn, co;
          sincosf(ph[j], &sn, &co);
          h[j] = sn;
          v[j] = q.omega * v[j] * co;
        }
        *reinterpret_cast<f32x4*>(q.hin + l * lstride + g) = h;
        if (l) *reinterpret_cast<f32x4*>(q.dz + (l - 1) * lstride + g) = v;
        *reinterpret_cast<f32x4*>(hs + row * FN_HS + c4) = v;
      }
      __syncthreads();
    }
    // gW1 += dz1^T (t, y, x), gb1 += sum_p dz1: thread = hidden column tid
    {
      float s = 0.f, st = 0.f, sy = 0.f, sx = 0.f;
#pragma unroll 8
      for (int p = 0; p < FN_P; ++p) {
        const float d = hs[p * FN_HS + tid];
        const f32x4 c = *reinterpret_cast<const f32x4*>(cs + p * FN_CS);
        s += d;
        st = fmaf(d, c[0], st);
        sy = fmaf(d, c[1], sy);
        sx = fmaf(d, c[2], sx);
      }
      gb1 += s;
      gw1[0] += st;
      gw1[1] += sy;
      gw1[2] += sx;
    }
    if constexpr (POSEGRAD) {
      const int d = tid >> 6, pl = tid & 63;
      const int p = tile * FN_P + pl;
      if (d < SR_IN && p < q.N) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
        for (int k = 0; k < FN_HID; k += 4) {
          const f32x4 h = *reinterpret_cast<const f32x4*>(hs + pl * FN_HS + k);
          a0 = fmaf(h[0], q.w[0][k * SR_IN + d], a0);
          a1 = fmaf(h[1], q.w[0][(k + 1) * SR_IN + d], a1);
          a2 = fmaf(h[2], q.w[0][(k + 2) * SR_IN + d], a2);
          a3 = fmaf(h[3], q.w[0][(k + 3) * SR_IN + d], a3);
        }
        q.g_poses[(size_t)p * SR_IN + d] = (a0 + a1) + (a2 + a3);
      }
    }
  }
  float* const out = q.part + (size_t)blockIdx.x * SR_PART;
#pragma unroll
  for (int d = 0; d < SR_IN; ++d) out[tid * SR_IN + d] = gw1[d];
  out[SR_PART_GB1 + tid] = gb1;
#pragma unroll
  for (int c = 0; c < 4; ++c) out[SR_PART_GW5 + c * FN_HID + tid] = gw5[c];
  if (tid < FN_OUT) {
    const float hi = (float)gb5;
    out[SR_PART_GB5 + tid] = hi;
    out[SR_PART_GB5 + FN_OUT + tid] = (float)(gb5 - (double)hi);
  }
}

// the chain kernel's partial sums, blocks in index order, into gW1 [256][3], gb1 [256], gW5 [4][256], gb5 [4]
__global__ __launch_bounds__(FN_NTHR) void siren_reduce_kernel(const float* part, int nparts, float* gw1, float* gb1, float* gw5, float* gb5) {
  const int i = blockIdx.x * FN_NTHR + threadIdx.x;
  if (i >= SR_PART) return;
  if (i >= SR_PART_GB5) {                              // the output bias: block sums that largely cancel, added in double, rounded once
    if (i >= SR_PART_GB5 + FN_OUT) return;             // the lo halves are read with their hi halves
    double d = 0.0;
    for (int c = 0; c < nparts; ++c) d += (double)part[(size_t)c * SR_PART + i] + (double)part[(size_t)c * SR_PART + i + FN_OUT];
    gb5[i - SR_PART_GB5] = (float)d;
    return;
  }
  float s = 0.f;
  for (int c = 0; c < nparts; ++c) s += part[(size_t)c * SR_PART + i];
  if (i < SR_PART_GB1) gw1[i] = s;
  else if (i < SR_PART_GW5) gb1[i - SR_PART_GB1] = s;
  else gw5[i - SR_PART_GW5] = s;
}

size_t part_floats(int ntiles) {
  const size_t h = hidden_wgrad_part_floats(ntiles), c = (size_t)chain_blocks(ntiles) * SR_PART;
  return h > c ? h : c;
}

}  // namespace

// the support table; a refusal leaves its reason, with the table, as the library's last error
static int siren_supported(const sininn_siren_args* a, const char* who) {
  if (a == nullptr || a->struct_bytes != sizeof(sininn_siren_args)) return 0;
  const bool ok = a->in_dim == SR_IN && a->hidden == FN_HID && a->layers == SR_SINES - 1 && a->out_dim == FN_OUT && a->omega > 0.f &&
                  a->omega <= 3.4028234664e38f;   // finite and positive: a NaN fails both comparisons
  if (!ok)
    set_error("%s: unsupported network (%d -> %d x (1 + %d) -> %d, omega %g; built for %d -> %d x (1 + %d) -> %d and a finite omega > 0)", who,
              a->in_dim, a->hidden, a->layers, a->out_dim, (double)a->omega, SR_IN, FN_HID, SR_SINES - 1, FN_OUT);
  return ok;
}
extern "C" int sininn_siren_supported(const sininn_siren_args* a) { return siren_supported(a, "sininn_siren_supported"); }

extern "C" size_t sininn_siren_saved_bytes(int64_t n) {
  if (n <= 0) return 0;
  return (size_t)SR_SINES * (size_t)((n + FN_P - 1) / FN_P) * FN_P * FN_HID * sizeof(float);
}

extern "C" size_t sininn_siren_workspace_bytes(int64_t n) {
  if (n <= 0 || n > ((int64_t)1 << 22)) return 0;
  const int ntiles = (int)((n + FN_P - 1) / FN_P);
  const size_t lstride = (size_t)ntiles * FN_P * FN_HID;
  return ((size_t)2 * (SR_SINES - 1) * lstride + (size_t)(SR_SINES - 1) * FN_HID * FN_HID + part_floats(ntiles)) * sizeof(float);
}

// pl != nullptr: the points are that pose list, not the descriptor's grid
static int check_args(const sininn_siren_args* a, const char* who, SirenDev& q, const PoseList* pl) {
  SININN_CHECK(a != nullptr, "%s: null args", who);
  SININN_CHECK(a->struct_bytes == sizeof(sininn_siren_args), "%s: struct_bytes is %zu, this library was built with %zu", who, a->struct_bytes,
               sizeof(sininn_siren_args));
  if (!siren_supported(a, who)) return 1;
  q = SirenDev{};
  if (int rc = check_points(a, who, q, pl)) return rc;
  if (int rc = check_layers<SR_SINES + 1>(a, who, q)) return rc;
  q.scale = a->scale;
  q.omega = a->omega;
  return 0;
}

extern "C" int sininn_siren_forward(const sininn_siren_args* a, const sininn_flownet_call* call, void* stream) {
  hipStream_t st = ST(stream);
  Call c;
  if (int rc = check_call(call, "siren", CALL_FORWARD, c)) return rc;
  SirenDev q;
  const char* const who = c.who();
  if (int rc = check_args(a, who, q, c.pl())) return rc;
  if (int rc = check_forward_buffers(a, who, sininn_siren_saved_bytes(q.N), q)) return rc;
  if (raise_lds(siren_fwd_kernel, SR_LDS, "siren_forward")) return 1;
  hipLaunchKernelGGL(siren_fwd_kernel, dim3(chain_blocks(q.ntiles)), dim3(FN_NTHR), SR_LDS, st, q);   // two resident blocks per CU
  SININN_LAUNCH_CHECK("siren_forward");
  return 0;
}

// POSEGRAD (with a pose list): the chain kernel that also writes the gradient of the coordinates; everything else is the same
extern "C" int sininn_siren_backward(const sininn_siren_args* a, const sininn_flownet_call* call, void* stream) {
  hipStream_t st = ST(stream);
  Call c;
  if (int rc = check_call(call, "siren", CALL_BACKWARD, c)) return rc;
  SirenPoseDev q;
  const char* const who = c.who();
  float* const g_poses = c.has(SININN_FLOWNET_POSEGRAD) ? c.c.g_poses : nullptr;
  SININN_CHECK(!c.has(SININN_FLOWNET_POSEGRAD) || g_poses != nullptr, "%s: null g_poses", who);
  if (int rc = check_args(a, who, q, c.pl())) return rc;
  q.g_poses = g_poses;
  if (int rc = check_backward_buffers<SR_SINES + 1>(a, who, sininn_siren_saved_bytes(q.N), sininn_siren_workspace_bytes(q.N), q)) return rc;
  const size_t lstride = (size_t)q.ntiles * FN_P * FN_HID;
  float* const ws = static_cast<float*>(a->workspace);
  float* const wt = ws + 2 * (SR_SINES - 1) * lstride;
  q.dz = ws;
  q.hin = ws + (SR_SINES - 1) * lstride;
  q.wt = wt;
  q.part = wt + (size_t)(SR_SINES - 1) * FN_HID * FN_HID;

  hipLaunchKernelGGL(siren_transpose_kernel, dim3(FN_HID, SR_SINES - 1), dim3(FN_NTHR), 0, st, a->w[1], a->w[2], a->w[3], wt);
  SININN_LAUNCH_CHECK("siren_transpose");
  const int cb = chain_blocks(q.ntiles);
  if (g_poses) {
    if (raise_lds(siren_bwd_chain_kernel<true>, SR_LDS, "siren_backward")) return 1;
    hipLaunchKernelGGL(siren_bwd_chain_kernel<true>, dim3(cb), dim3(FN_NTHR), SR_LDS, st, q);
  } else {
    if (raise_lds(siren_bwd_chain_kernel<false>, SR_LDS, "siren_backward")) return 1;
    hipLaunchKernelGGL(siren_bwd_chain_kernel<false>, dim3(cb), dim3(FN_NTHR), SR_LDS, st, static_cast<const SirenDev&>(q));
  }
  SININN_LAUNCH_CHECK("siren_bwd_chain");
  hipLaunchKernelGGL(siren_reduce_kernel, dim3((SR_PART + FN_NTHR - 1) / FN_NTHR), dim3(FN_NTHR), 0, st, (const float*)q.part, cb, a->gw[0], a->gb[0],
                     a->gw[SR_SINES], a->gb[SR_SINES]);
  SININN_LAUNCH_CHECK("siren_reduce");
  for (int l = SR_SINES - 1; l >= 1; --l)                // gW_{l+1} = dz_{l+1}^T h_l
    if (int rc = hidden_wgrad_launch(q.ntiles, q.dz + (l - 1) * lstride, q.hin + (l - 1) * lstride, q.part, a->gw[l], a->gb[l], st)) return rc;
  return 0;
}

}  // namespace sininn
