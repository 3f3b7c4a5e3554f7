// Frame synthesis from a fitted pair of flows: softmax-splat both frames to K in-between times and blend them.
//   Z0 = -20 mean_c |I0 - warp(I1, F01)|,  Z1 = -20 mean_c |I1 - warp(I0, F10)|          (trainer.py:61-68, Resample2d warp)
//   S0 = softmax-splat(I0, tau F01, Z0),   S1 = softmax-splat(I1, (1 - tau) F10, Z1)     (softsplat.py:331-358)
//   out = ((1 - tau) [N0 != 0] S0 + tau [N1 != 0] S1) / ((1 - tau) [N0 != 0] + tau [N1 != 0]),  (1 - tau) I0 + tau I1 where both
//   splats are empty;  N = the splatted exp(Z) channel.
// Two launches whatever K is: the scatter reads frame, flow and metric once and reuses them for every time; Z, the warped frame,
// exp(Z) and the concatenated splat inputs never exist in HBM.  Both kernels are HBM / atomic bound.
#include "common.h"
#include "bilinear_taps.h"

namespace sininn {

constexpr int FS_TX = 32, FS_TY = 8;               // source tile of one block: a wave is two rows of 32 pixels
constexpr int FS_SCATTER_MAX_BLOCKS = 2048;   // the scatter launch: at most this many blocks, block-stride over the source tiles
constexpr int FS_MAX_K = 64;

// The Resample2d sample of img[b, c] at pixel (x, y) + flow (resample2d_coord, zeros outside): false where it has no tap inside the
// frame at all -- on an axis of length 1 the coordinate is infinite (or 0 / 0) -- or the coordinate is too large for an int.
__device__ __forceinline__ bool warp_taps(int x, int y, float fx, float fy, int H, int W, BilinearTaps& t) {
  t = {};
  if (H < 2 || W < 2) return false;
  float ix, iy;
  resample2d_coord(x, y, fx, fy, H, W, ix, iy);
  if (!(fabsf(ix) < 1e9f) || !(fabsf(iy) < 1e9f)) return false;      // the float -> int conversions stay defined
  t = bilinear_taps(ix, iy);
  return true;
}

// Landing coordinate p + fl(t * f): the flow is scaled, rounded, then added to the pixel -- the same two roundings as splatting the
// tensor t * F.  hipcc's __fmul_rn is a plain product, which -ffp-contract=fast fuses into the add that follows (one rounding, a
// coordinate one ulp off the definition's); the pragma is what keeps the two apart.
__device__ __forceinline__ float landing(int p, float t, float f) {
#pragma clang fp contract(off)
  const float scaled = t * f;
  return (float)p + scaled;
}

// One lane per source pixel (b, y, x) of one source frame (side 0: I0 along F01, side 1: I1 along F10).
// acc[B][K][2][C + 1][H][W], zeroed by the caller: channels 0..C-1 the splatted I * exp(Z), channel C the splatted exp(Z).
template <int C>
__global__ __launch_bounds__(FS_TX * FS_TY) void flowsynth_scatter_kernel(const float* __restrict__ i0, const float* __restrict__ i1,
                                                                          const float* __restrict__ f01, const float* __restrict__ f10,
                                                                          const float* __restrict__ tau, int B, int K, int H, int W,
                                                                          float* __restrict__ acc) {
  const int tiles_x = (W + FS_TX - 1) / FS_TX, tiles_y = (H + FS_TY - 1) / FS_TY;
  const int64_t HW = (int64_t)H * W, ntiles = (int64_t)2 * B * tiles_y * tiles_x;
  const int lx = threadIdx.x % FS_TX, ly = threadIdx.x / FS_TX;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {         // block-uniform: every shuffle below is wave-wide
    int64_t q = tile;
    const int tx = (int)(q % tiles_x); q /= tiles_x;
    const int ty = (int)(q % tiles_y); q /= tiles_y;
    const int b = (int)(q % B), side = (int)(q / B);
    const int x = tx * FS_TX + lx, y = ty * FS_TY + ly;
    const bool live = x < W && y < H;
    const int64_t r = live ? (int64_t)y * W + x : 0;
    const float* src = (side ? i1 : i0) + (int64_t)b * C * HW;
    const float* oth = (side ? i0 : i1) + (int64_t)b * C * HW;
    const float* flow = (side ? f10 : f01) + (int64_t)b * 2 * HW;
    float v[C + 1], fx = 0.f, fy = 0.f;
#pragma unroll
    for (int c = 0; c <= C; ++c) v[c] = 0.f;
    if (live) {
      fx = flow[r]; fy = flow[HW + r];
      BilinearTaps wt;
      const bool ok = warp_taps(x, y, fx, fy, H, W, wt);
      float l1 = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float* base = oth + c * HW;
        auto tap = [&](int yy, int xx) -> float { return (ok && tap_inside(yy, xx, H, W)) ? base[(int64_t)yy * W + xx] : 0.f; };
        const float t00 = tap(wt.y0, wt.x0), t10 = tap(wt.y0 + 1, wt.x0), t01 = tap(wt.y0, wt.x0 + 1), t11 = tap(wt.y0 + 1, wt.x0 + 1);
        const float warped = t00 * wt.wy0 * wt.wx0 + t01 * wt.wy0 * wt.wx1 + t10 * wt.wy1 * wt.wx0 + t11 * wt.wy1 * wt.wx1;
        v[c] = src[c * HW + r];
        l1 += fabsf(v[c] - warped);
      }
      const float w = expf(__fmul_rn(-20.f, l1 / (float)C));
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = __fmul_rn(v[c], w);
      v[C] = w;
    }
    for (int k = 0; k < K; ++k) {
      const float tk = tau[k], t = side ? 1.f - tk : tk;
      SplatTaps tp = {};
      bool any = false;
      if (live) {
        const float ox = landing(x, t, fx), oy = landing(y, t, fy);
        if (ox == ox && oy == oy && fabsf(ox) < 1e9f && fabsf(oy) < 1e9f) { tp = splat_taps(ox, oy, H, W); any = true; }
      }
      const TapMerge mg = tap_merge_plan<FS_TX>(any, tp.nwx, tp.nwy);       // neighbouring sources share taps (bilinear_taps.h)
      const int64_t o_nw = (int64_t)tp.nwy * W + tp.nwx;
      float* plane = acc + ((((int64_t)b * K + k) * 2 + side) * (C + 1)) * HW;
#pragma unroll
      for (int c = 0; c <= C; ++c) {
        float cnw = 0.f, cne = 0.f, csw = 0.f, cse = 0.f;
        if (any) {
          cnw = tp.vnw ? v[c] * tp.nw : 0.f; cne = tp.vne ? v[c] * tp.ne : 0.f;
          csw = tp.vsw ? v[c] * tp.sw : 0.f; cse = tp.vse ? v[c] * tp.se : 0.f;
        }
        tap_merge(mg, cnw, cne, csw, cse);
        if (any) {
          float* o = plane + c * HW;
          if (tp.vnw && cnw != 0.f) atomic_add_f32(o + o_nw, cnw);
          if (tp.vne && cne != 0.f) atomic_add_f32(o + o_nw + 1, cne);
          if (tp.vsw && csw != 0.f) atomic_add_f32(o + o_nw + W, csw);
          if (tp.vse && cse != 0.f) atomic_add_f32(o + o_nw + W + 1, cse);
        }
      }
    }
  }
}

// One lane per output pixel (b, k, y, x): normalise both splats, form the hole masks and the blend; -0.0 counts as a hole.
template <int C>
__global__ void flowsynth_blend_kernel(const float* __restrict__ i0, const float* __restrict__ i1, const float* __restrict__ tau,
                                       const float* __restrict__ acc, int B, int K, int H, int W, float* __restrict__ out,
                                       uint8_t* __restrict__ out_u8) {
  const int64_t HW = (int64_t)H * W, total = (int64_t)B * K * HW;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int64_t r = idx % HW, bk = idx / HW;
  const int k = (int)(bk % K), b = (int)(bk / K);
  const float tk = tau[k], sk = 1.f - tk;
  const float* a0 = acc + (bk * 2 + 0) * (C + 1) * HW + r;
  const float* a1 = acc + (bk * 2 + 1) * (C + 1) * HW + r;
  const float n0 = a0[C * HW], n1 = a1[C * HW];
  const float w0 = __fmul_rn(sk, n0 != 0.f ? 1.f : 0.f), w1 = __fmul_rn(tk, n1 != 0.f ? 1.f : 0.f);
  const float den = __fadd_rn(w0, w1);
  const float d0 = n0 == 0.f ? 1.f : n0, d1 = n1 == 0.f ? 1.f : n1;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float o;
    // every operation rounded once, no contraction: the expression `flowsynth.composed` evaluates in torch
    if (den != 0.f) {
      o = __fdiv_rn(__fadd_rn(__fmul_rn(w0, __fdiv_rn(a0[c * HW], d0)), __fmul_rn(w1, __fdiv_rn(a1[c * HW], d1))), den);
    } else {
      const int64_t p = ((int64_t)b * C + c) * HW + r;
      o = __fadd_rn(__fmul_rn(sk, i0[p]), __fmul_rn(tk, i1[p]));
    }
    const int64_t q = (bk * C + c) * HW + r;
    out[q] = o;
    if (out_u8) out_u8[q] = (uint8_t)frame_byte(o);
  }
}

extern "C" int64_t sininn_flow_synth_workspace(int B, int K, int C, int H, int W) {
  if (B <= 0 || K <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return (int64_t)B * K * 2 * (C + 1) * H * W;
}

extern "C" int sininn_flow_synth(const float* i0, const float* i1, const float* f01, const float* f10, const float* tau, int B, int K, int C,
                                 int H, int W, float* workspace, int64_t workspace_floats, float* out, uint8_t* out_u8, void* stream) {
  hipStream_t st = ST(stream);
  SININN_CHECK(i0 && i1 && f01 && f10 && tau && workspace && out, "flow_synth: null pointer");
  SININN_CHECK(B > 0 && K > 0 && C > 0 && H > 0 && W > 0, "flow_synth: bad shape (every size must be positive)");
  SININN_CHECK(K <= FS_MAX_K, "flow_synth: K = %d times in one call, at most %d", K, FS_MAX_K);
  SININN_CHECK(C == 1 || C == 3, "flow_synth: frames have 1 or 3 channels (got %d)", C);
  const int64_t need = sininn_flow_synth_workspace(B, K, C, H, W);
  SININN_CHECK(workspace_floats >= need, "flow_synth: workspace of %lld floats, need %lld", (long long)workspace_floats,
               (long long)need);
  const int64_t total = (int64_t)B * K * H * W;
  SININN_CHECK((total + 255) / 256 < ((int64_t)1 << 31), "flow_synth: B * K * H * W too large for one launch");
  hipError_t e = hipMemsetAsync(workspace, 0, (size_t)need * sizeof(float), st);
  SININN_CHECK(e == hipSuccess, "flow_synth: zeroing the workspace failed: %s", hipGetErrorString(e));
  const int64_t ntiles = (int64_t)2 * B * ((H + FS_TY - 1) / FS_TY) * ((W + FS_TX - 1) / FS_TX);
  const int blocks = (int)(ntiles < FS_SCATTER_MAX_BLOCKS ? ntiles : FS_SCATTER_MAX_BLOCKS);
  const dim3 bgrid((unsigned)((total + 255) / 256));
  if (C == 1) {
    hipLaunchKernelGGL(flowsynth_scatter_kernel<1>, dim3(blocks), dim3(FS_TX * FS_TY), 0, st, i0, i1, f01, f10, tau, B, K, H, W,
                       workspace);
    SININN_LAUNCH_CHECK("flowsynth_scatter");
    hipLaunchKernelGGL(flowsynth_blend_kernel<1>, bgrid, dim3(256), 0, st, i0, i1, tau, workspace, B, K, H, W, out, out_u8);
  } else {
    hipLaunchKernelGGL(flowsynth_scatter_kernel<3>, dim3(blocks), dim3(FS_TX * FS_TY), 0, st, i0, i1, f01, f10, tau, B, K, H, W,
                       workspace);
    SININN_LAUNCH_CHECK("flowsynth_scatter");
    hipLaunchKernelGGL(flowsynth_blend_kernel<3>, bgrid, dim3(256), 0, st, i0, i1, tau, workspace, B, K, H, W, out, out_u8);
  }
  SININN_LAUNCH_CHECK("flowsynth_blend");
  return 0;
}

}  // namespace sininn
