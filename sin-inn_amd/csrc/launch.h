// The internal functions of libsininn that one translation unit defines and another calls: each declared here once, under
// the file that defines it.  common.h includes this header, so every definition is compiled in sight of its declaration and a
// signature that drifts is a compile error, not a new overload.  The C entry points themselves are declared by
// include/sininn.h and defined beside their kernels; library code calls them by their sininn_* names.
#pragma once

// the stream of an entry point (void* in the C ABI) as HIP takes it
#define ST(s) static_cast<hipStream_t>(s)

namespace sininn {

struct ConvDev;    // conv_mfma_impl.h
struct ConvDevB;   // conv_bf16_types.h

// ---- api.cpp ----
void set_error(const char* fmt, ...);

// ---- conv_mfma.hip: argument validation + device-side descriptor of one fp32 conv ----
int conv_prepare(const sininn_conv_args* a, ConvDev& d);

// ---- conv_mfma_k1.hip / conv_mfma_k3.hip: the instantiations of the conv engine, one translation unit per kernel size ----
int conv_dispatch_k1(ConvDev& d, hipStream_t st, int force_cfg);
int conv32_dispatch_k1(ConvDev& d, hipStream_t st, int force_cfg, bool must);
int conv_dispatch_k3(ConvDev& d, hipStream_t st, int force_cfg);
int conv32_dispatch_k3(ConvDev& d, hipStream_t st, int force_cfg, bool must);
int wino_dispatch_k3(ConvDev& d, hipStream_t st, int cg2);

// ---- conv_bf16.hip ----
int conv_bf16_prepare(const sininn_conv_args* a, ConvDevB& q);
int conv_bf16_launch(const sininn_conv_args* a, hipStream_t st);

// ---- conv_pair_k1.hip ----
void conv_pair_k1_enable(int on);
int conv_pair_k1_preferred(const sininn_conv_args* f);

// ---- conv_pair_bf16.hip: the mixed-precision twin of the fused 1x1 pair ----
int conv_pair_bf16_supported(const sininn_conv_args* f, const sininn_conv_args* s);
int conv_pair_bf16_launch(const sininn_conv_args* f, const sininn_conv_args* s, hipStream_t st);

// ---- conv_sub1.hip: the whole backward of a fp32 1x1 subnet in one persistent launch (h recomputed, dh on chip) ----
void conv_sub1_bwd_enable(int on);
int conv_sub1_bwd_shape_supported(int ksize, int dtype, int cond_cin, int co);
int conv_sub1_bwd_launch(const sininn_conv_args* rc, const sininn_conv_args* d2, const sininn_conv_args* d1, int no_dx, void* ws,
                         size_t ws_bytes, int* slabs_out, hipStream_t st);
int conv_sub1_bwd_reduce(int cond_cin, int co, const void* ws, int slabs, float* gw2, float* gb2, float* gw1, float* gb1, hipStream_t st);

// ---- conv_sub1_bf16.hip: the mixed-precision twins (bf16 weight packs, fp32 tensors), and for a wide (level-1) subnet the
// persistent forward, the data gradients with conv1's weight gradient riding along, and conv2's weight gradient ----
bool conv_sub1_bf16_enabled();
void conv_sub1_bf16_enable(int on);
int conv_sub1_bf16_bwd_launch(const sininn_conv_args* rc, const sininn_conv_args* d2, const sininn_conv_args* d1, int no_dx, void* ws,
                              size_t ws_bytes, int* slabs_out, hipStream_t st);
int conv_sub1_bf16_fwd_supported(const sininn_conv_args* f, const sininn_conv_args* s);
int conv_sub1_bf16_fwd_launch(const sininn_conv_args* f, const sininn_conv_args* s, hipStream_t st);
int conv_sub1_bf16_wide_fwd_supported(const sininn_conv_args* f, const sininn_conv_args* s);
int conv_sub1_bf16_wide_fwd_launch(const sininn_conv_args* f, const sininn_conv_args* s, hipStream_t st);
int conv_sub1_bf16_wide_bwd_supported(const sininn_conv_args* d2, const sininn_conv_args* d1);
int conv_sub1_bf16_wide_bwd_launch(const sininn_conv_args* d2, const sininn_conv_args* d1, hipStream_t st);
size_t conv_sub1_bf16_wide_ws_bytes(int ksize, int dtype, int cond_cin, int co);
int conv_sub1_bf16_wide_bwd_wg1_launch(const sininn_conv_args* d2, const sininn_conv_args* d1, const float* x, int x_stride, void* ws,
                                       size_t ws_bytes, int* slabs_out, hipStream_t st);
int conv_sub1_bf16_wide_reduce(const void* ws, int slabs, float* gw1, float* gb1, hipStream_t st);
size_t conv_sub1_bf16_wide_wg2_ws_bytes(int ksize, int dtype, int cond_cin, int co);
int conv_sub1_bf16_wide_wg2_launch(const float* dr, int dr_stride, const void* h, int h_stride, int B, int H, int W, void* ws,
                                   size_t ws_bytes, float* gw2, float* gb2, hipStream_t st);

// ---- conv_sub3_bf16.hip ----
bool sub3_fusion_enabled();
void sub3_fusion_set(int on);

// ---- conv3_smallk_bf16.hip: the small-K 3x3 convs of a level-0 subnet; `bits` = the ReLU gates as a bit mask [pixel][8] words, or NULL ----
void conv3_smallk_enable(int on);
int conv3_smallk_bf16_launch_bits(const sininn_conv_args* a, unsigned* bits, hipStream_t st);

// ---- wgrad_mfma.hip ----
bool wgrad_grouping_enabled();
int wgrad_group_mode();
size_t wgrad_group_mixed_workspace_bytes(const sininn_wgrad_item* items, int n, int B, int H, int W, int ksize);
int wgrad_group_mixed_launch(const sininn_wgrad_item* items, int n, int B, int H, int W, int ksize, void* ws, size_t ws_bytes,
                             hipStream_t st);

// ---- elementwise.hip: sininn_irn_coupling_bwd with the row stride and the zero padding of dG spelled out ----
int irn_coupling_bwd_launch(const float* dy, int dy_stride, const float* vy, int vy_stride, const float* hval, int64_t M,
                            int Co, float clamp, int inverse, float* dG, int dG_stride, int dG_pad, float* dh, float* dv,
                            int dv_stride, hipStream_t st);

// ---- hbm_fast.hip ----
bool sample_windows_dense_try(const uint8_t* hr_clip, const uint8_t* lr_clip, const int* idx, int n, int T, int H, int W, int h,
                              int w, int win, float* hr_out, const int64_t hs[4], float* lr_out, const int64_t ls[4],
                              hipStream_t st);
int copy_channels_launch(const float* in, int in_stride, float* out, int out_stride, int64_t M, int C, int Cpad, hipStream_t st);

// ---- dense_bf16.hip ----
int copy_channels_bf16_launch(const float* in, int in_stride, void* out, int out_stride, int64_t M, int C, int Cpad, hipStream_t st);

// ---- flownet.hip: gW [256][256] and gb [256] of one hidden layer, shared with siren.hip ----
size_t hidden_wgrad_part_floats(int ntiles);
int hidden_wgrad_launch(int ntiles, const float* dh, const float* in, float* part, float* gw, float* gb, hipStream_t st);

// ---- glow_exec.cpp: the per-device event ring, and the per-class launch brackets of bench.py's roofline.classes ----
int order_after(hipStream_t waiter, hipStream_t producer);
hipEvent_t class_scope_open(int cls, int ksize, double flops, hipStream_t st);
void class_scope_close(hipEvent_t end, hipStream_t st);

}  // namespace sininn
