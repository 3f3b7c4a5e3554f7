// Helpers of the mixed-precision IRN DenseBlock executor (dense_exec.cpp, sininn_dense_forward_bf16 / _backward_bf16;
// reference archs.py:74-98): the fp32 -> bf16 copy of the block input into the feature buffer, and the batched bf16 weight
// packs with the feature buffer's input-channel gap.  The convolutions themselves run on conv_bf16.hip.
#include "common.h"

namespace sininn {

typedef __bf16 dbf16x4 __attribute__((ext_vector_type(4)));

// out[m][c] = bf16(c < C ? in[m][c] : 0) for c < Cpad (C, Cpad multiples of 4; round to nearest even, once)
__global__ void copy_channels_bf16_kernel(const float* __restrict__ in, int in_stride, __bf16* __restrict__ out, int out_stride,
                                          int64_t M, int C4, int Cpad4) {
  const int64_t total = M * Cpad4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % Cpad4);
    const int64_t m = i / Cpad4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (c4 < C4) v = *reinterpret_cast<const f32x4*>(in + m * in_stride + c4 * 4);
    const dbf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    *reinterpret_cast<dbf16x4*>(out + m * out_stride + c4 * 4) = o;
  }
}

int copy_channels_bf16_launch(const float* in, int in_stride, void* out, int out_stride, int64_t M, int C, int Cpad, hipStream_t st) {
  SININN_CHECK(in && out && M > 0 && C > 0 && C % 4 == 0 && Cpad % 4 == 0 && Cpad >= C, "copy_channels_bf16: bad arguments");
  SININN_CHECK(in_stride % 4 == 0 && out_stride % 4 == 0 && out_stride >= Cpad && aligned16(in) && aligned16(out),
               "copy_channels_bf16: alignment");
  const int64_t total = M * (Cpad / 4);
  const int64_t blocks = (total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192;
  hipLaunchKernelGGL(copy_channels_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, st, in, in_stride, static_cast<__bf16*>(out),
                     out_stride, M, C / 4, Cpad / 4);
  SININN_LAUNCH_CHECK("copy_channels_bf16");
  return 0;
}

// ---- batched bf16 packs ---------------------------------------------------------------------------------------------
// sininn_pack_desc read with the bf16 layouts of sininn_pack_conv_weights_bf16: w_fwd [taps][Np][Kp] (Kp = Cin rounded up to
// 16), w_dgrad [taps][Cdp][Kd] (Kd = N rounded up to 16), both bf16; b_fwd [Np] fp32.  N / Cin are the PACKED dimensions and
// src_n / gap_begin / gap_len describe the source weight as in the fp32 batched pack (elementwise.hip).
__host__ __device__ static inline void pack_regions_bf16(const sininn_pack_desc& d, int& nf, int& nd, int& nb) {
  const int taps = d.ksize * d.ksize, kp = (d.Cin + 15) / 16 * 16, kd = (d.N + 15) / 16 * 16;
  nf = d.w_fwd ? taps * d.Np * kp : 0;
  nd = d.w_dgrad ? taps * d.Cdp * kd : 0;
  nb = d.b_fwd ? d.Np : 0;
}

extern "C" int sininn_pack_work_items_bf16(const sininn_pack_desc* d) {
  if (!d || d->wino_fwd || d->wino_dgrad || d->N <= 0 || d->Cin <= 0 || (d->ksize != 1 && d->ksize != 3)) return 0;
  int nf, nd, nb;
  pack_regions_bf16(*d, nf, nd, nb);
  return nf + nd + nb;
}

// packed (output nn, packed input channel c, tap t) -> source weight element, 0 in the channel gap and beyond src_n
__device__ __forceinline__ float pack_src_bf16(const sininn_pack_desc& d, int nn, int c, int t, int taps) {
  int sc = c;
  if (d.gap_len > 0) {
    if (c >= d.gap_begin + d.gap_len) sc = c - d.gap_len;
    else if (c >= d.gap_begin) return 0.f;
  }
  if (nn >= (d.src_n > 0 ? d.src_n : d.N)) return 0.f;
  return d.w[((size_t)nn * (d.Cin - d.gap_len) + sc) * taps + t];
}

__global__ void pack_batch_bf16_kernel(const sininn_pack_desc* __restrict__ descs, int n, int total) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int lo = 0, hi = n - 1;                              // last descriptor with work_begin <= idx
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].work_begin <= idx) lo = mid; else hi = mid - 1;
  }
  const sininn_pack_desc d = descs[lo];
  int k = idx - d.work_begin;
  int nf, nd, nb;
  pack_regions_bf16(d, nf, nd, nb);
  const int taps = d.ksize * d.ksize, kp = (d.Cin + 15) / 16 * 16, kd = (d.N + 15) / 16 * 16;
  if (k < nf) {
    const int c = k % kp, q = (k / kp) % d.Np, t = k / (kp * d.Np);
    const int nn = d.colmap ? d.colmap[q] : q;
    const float v = (nn >= 0 && nn < d.N && c < d.Cin) ? pack_src_bf16(d, nn, c, t, taps) : 0.f;
    reinterpret_cast<__bf16*>(d.w_fwd)[k] = (__bf16)v;
    return;
  }
  k -= nf;
  if (k < nd) {
    const int nn = k % kd, c = (k / kd) % d.Cdp, t = k / (kd * d.Cdp);
    const float v = (c < d.Cin && nn < d.N) ? pack_src_bf16(d, nn, c, taps - 1 - t, taps) : 0.f;
    reinterpret_cast<__bf16*>(d.w_dgrad)[k] = (__bf16)v;
    return;
  }
  k -= nd;
  if (k < nb) {
    const int nn = d.colmap ? d.colmap[k] : k;
    d.b_fwd[k] = (d.bias && nn >= 0 && nn < (d.src_n > 0 ? d.src_n : d.N)) ? d.bias[nn] : 0.f;
  }
}

extern "C" int sininn_pack_batch_bf16(const sininn_pack_desc* descs, int n, int total, void* stream) {
  hipStream_t st = ST(stream);
  SININN_CHECK(descs != nullptr && n > 0 && total > 0, "pack_batch_bf16: bad arguments");
  hipLaunchKernelGGL(pack_batch_bf16_kernel, dim3((total + 255) / 256), dim3(256), 0, st, descs, n, total);
  SININN_LAUNCH_CHECK("pack_batch_bf16");
  return 0;
}

}  // namespace sininn
