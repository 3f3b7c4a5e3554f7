// extern "C" surface of libsininn.so (see include/sininn.h for the contract).
#include <stdarg.h>
#include <string.h>

#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "common.h"

namespace sininn {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int conv_launch(const sininn_conv_args* a, hipStream_t st);
int conv_pair_k1_supported(const sininn_conv_args* f, const sininn_conv_args* s);
size_t conv_sub1_bwd_workspace_bytes(int cond_cin, int co);
int conv_sub1_bwd_launch(const sininn_conv_args* rc, const sininn_conv_args* d2, const sininn_conv_args* d1, int no_dx, void* ws,
                         size_t ws_bytes, int* slabs_out, hipStream_t st);
int conv_sub1_bwd_reduce(int cond_cin, int co, const void* ws, int slabs, float* gw2, float* gb2, float* gw1, float* gb1, hipStream_t st);
void conv_sub1_bwd_enable(int on);
void conv3_smallk_enable(int on);
size_t conv_sub1_bf16_wide_ws_bytes(int ksize, int dtype, int cond_cin, int co);
int conv_sub1_bf16_wide_bwd_supported(const sininn_conv_args* d2, const sininn_conv_args* d1);
int conv_sub1_bf16_wide_bwd_launch(const sininn_conv_args* d2, const sininn_conv_args* d1, hipStream_t st);
int conv_sub1_bf16_wide_bwd_wg1_launch(const sininn_conv_args* d2, const sininn_conv_args* d1, const float* x, int x_stride, void* ws, size_t ws_bytes,
                                       int* slabs_out, hipStream_t st);
int conv_sub1_bf16_wide_reduce(const void* ws, int slabs, float* gw1, float* gb1, hipStream_t st);
size_t conv_sub1_bf16_wide_wg2_ws_bytes(int ksize, int dtype, int cond_cin, int co);
int conv_sub1_bf16_wide_wg2_launch(const float* dr, int dr_stride, const void* h, int h_stride, int B, int H, int W, void* ws, size_t ws_bytes,
                                   float* gw2, float* gb2, hipStream_t st);
int conv3_smallk_bf16_supported(const sininn_conv_args* a);
int conv3_smallk_bf16_launch_bits(const sininn_conv_args* a, unsigned* bits, hipStream_t st);
int conv_sub1_fwd_supported(const sininn_conv_args* f, const sininn_conv_args* s);
int conv_sub1_fwd_launch(const sininn_conv_args* f, const sininn_conv_args* s, hipStream_t st);
int conv_pair_k1_launch(const sininn_conv_args* f, const sininn_conv_args* s, hipStream_t st);
void conv_pair_k1_enable(int on);
int conv_sub3_bf16_supported(const sininn_conv_args* f, const sininn_conv_args* s);
int conv_sub3_bf16_launch(const sininn_conv_args* f, const sininn_conv_args* s, hipStream_t st);
void sub3_fusion_set(int on);
void conv_set_test_hooks(int force_cfg, int force_ck);
void wgrad_set_force16(int on);
size_t wgrad_workspace_bytes(int N, int Cin, int ksize, int B, int H, int W);
int wgrad_launch(const float* in, int in_stride, int Cin, const float* dout, int dout_stride, int N, int B, int H, int W,
                 int ksize, float* gw, float* gb, void* ws, size_t ws_bytes, hipStream_t st);
size_t wgrad_group_workspace_bytes(const sininn_wgrad_item* items, int n, int B, int H, int W, int ksize);
int wgrad_group_launch(const sininn_wgrad_item* items, int n, int B, int H, int W, int ksize, void* ws, size_t ws_bytes,
                       hipStream_t st);
int pack_launch(const float* w, const float* bias, int N, int Cin, int ksize, const int* colmap, int Np, float* w_fwd,
                float* b_fwd, int Cdp, float* w_dgrad, hipStream_t st);
int coupling_bwd_launch(const float* dy, int dy_stride, const int* dy_map, const float* vy, int vy_stride,
                        const int* vy_map, const float* s, const float* gld, int B, int HW, int Co, float clamp,
                        int inverse, float* dr, float* dv, int dv_stride, hipStream_t st);
int squeeze_launch(const float* in, const int64_t is[4], float* out, const int64_t os[4], int B, int C, int H, int W,
                   int levels, int inverse, const int* chan_map, int map_on_out, hipStream_t st);
int permute_launch(const float* in, int in_stride, float* out, int out_stride, int64_t M, int C, const int* idx,
                   hipStream_t st);
int sqdiff_sum_launch(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4], int B, int C, int H,
                      int W, float* out, hipStream_t st);
int sqdiff_bwd_launch(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4], int B, int C, int H,
                      int W, const float* scale, float gscale, float* gx, const int64_t gxs[4], float* gy,
                      const int64_t gys[4], hipStream_t st);
int mmd_gram_launch(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4], int B, int C, int H,
                    int W, float* g, hipStream_t st);
int mmd_finish_launch(const float* g, int B, int rev, float* out, float* coef, hipStream_t st);
int mmd_bwd_launch(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4], int B, int C, int H, int W,
                   const float* coef, const float* scale, float* gx, const int64_t gxs[4], float* gy,
                   const int64_t gys[4], hipStream_t st);
int affine_warp_launch(const float* img, const int64_t is[4], const float* theta, int B, int C, int H, int W, float* out,
                       const int64_t os[4], const float* ref, const int64_t rs[4], float* sse, hipStream_t st);
int affine_warp_bwd_launch(const float* gout, const int64_t gs[4], const float* theta, int B, int C, int H, int W,
                           float* gimg, const int64_t gis[4], hipStream_t st);
int flow_warp_l1_launch(const float* img, const float* flow, const float* target, int B, int C, int H, int W,
                        float* warped, float* metric, hipStream_t st);
int flow_warp_l1_bwd_launch(const float* img, const float* flow, const float* target, const float* warped,
                            const float* gwarped, const float* gmetric, int B, int C, int H, int W, float* gimg,
                            float* gflow, hipStream_t st);
int flow_warp_l1_bf16_launch(const void* img, const float* flow, const void* target, int B, int C, int H, int W,
                             void* warped, float* metric, hipStream_t st);
int flow_warp_l1_bwd_bf16_launch(const void* img, const float* flow, const void* target, const void* warped,
                                 const void* gwarped, const float* gmetric, int B, int C, int H, int W, float* gimg,
                                 float* gflow, hipStream_t st);
int sample_windows_launch(const uint8_t* hr_clip, const uint8_t* lr_clip, const int* idx, int n, int T, int H, int W,
                          int h, int w, int win, float* hr_out, const int64_t hs[4], float* lr_out,
                          const int64_t ls[4], hipStream_t st);
int adam_launch(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                float wd, int step, float gscale, hipStream_t st);
int haar_launch(const float* in, const int64_t is[4], float* out, const int64_t os[4], int B, int C, int H, int W,
                int inverse, hipStream_t st);
int lrelu_bwd_launch(float* g, int g_stride, const float* f, int f_stride, int64_t M, int n, float slope, hipStream_t st);
int irn_tail_launch(const float* v, int v_stride, const float* h, const float* g, int64_t M, int Co, float clamp, int inverse,
                    float* out, int out_stride, hipStream_t st);
int irn_coupling_bwd_launch(const float* dy, int dy_stride, const float* vy, int vy_stride, const float* hval, int64_t M,
                            int Co, float clamp, int inverse, float* dG, int dG_stride, int dG_pad, float* dh, float* dv,
                            int dv_stride, hipStream_t st);
int squeeze_rows_launch(const float* in, float* out, int B, int C, int H, int W, int levels, int inverse, const int* map,
                        hipStream_t st);
int pack_bf16_launch(const float* w, const float* bias, int N, int Cin, int ksize, const int* colmap, int Np, void* wb_fwd,
                     float* b_fwd, int Cdp, void* wb_dgrad, hipStream_t st);
int frames_to_u8_launch(const float* in, const int64_t is[4], uint8_t* out, int B, int C, int H, int W, int wrap,
                        hipStream_t st);
size_t dense_workspace_bytes(int B, int H, int W, int cin, int cout);
int dense_forward(const sininn_dense_args* a, hipStream_t st);
int dense_backward(const sininn_dense_args* a, hipStream_t st, hipStream_t wst);
size_t dense_bf16_workspace_bytes(int B, int H, int W, int cin, int cout);
int dense_forward_bf16(const sininn_dense_bf16_args* a, hipStream_t st);
int dense_backward_bf16(const sininn_dense_bf16_args* a, hipStream_t st, hipStream_t wst);
int pack_work_items_bf16(const sininn_pack_desc* d);
int pack_batch_bf16_launch(const sininn_pack_desc* descs, int n, int total, hipStream_t st);
void profile_classes_begin();
int profile_classes_end(int n, double* ms, double* flops, int* launches);
int profile_classes_bytes(int n, double* bytes);
void profile_begin(int h, unsigned long long* stamps, int max_launches);
int profile_end(int* count, float* total_ms);
int flownet_supported(const sininn_flownet_args* a, const char* who);
int flownet_supported_dim(const sininn_flownet_args* a, int dim, const char* who);
size_t flownet_saved_bytes(int64_t n);
size_t flownet_workspace_bytes(int64_t n);
size_t flownet_forward_workspace_bytes(const sininn_flownet_args* a);
int flownet_forward_launch(const sininn_flownet_args* a, const sininn_flownet_call* call, hipStream_t st);
int flownet_backward_launch(const sininn_flownet_args* a, const sininn_flownet_call* call, hipStream_t st);
int flownet_sample_mask_launch(const sininn_flownet_args* a, const sininn_flownet_call* call, float* out, hipStream_t st);
size_t flownet_encgrad_workspace_bytes(const sininn_flownet_args* a);
size_t flownet_posegrad_workspace_bytes(const sininn_flownet_args* a, int with_enc_grad);
size_t flownet_jacobian_saved_bytes(int64_t n, int n_dirs);
size_t flownet_jacobian_workspace_bytes(const sininn_flownet_args* a, int64_t n, int n_dirs);
int flownet_jacobian_forward_launch(const sininn_flownet_args* a, const sininn_flownet_call* call, unsigned dirs, float* jac, float* tsaved,
                                    size_t tsaved_bytes, hipStream_t st);
int flownet_jacobian_backward_launch(const sininn_flownet_args* a, const sininn_flownet_call* call, unsigned dirs, const float* djac,
                                     const float* tsaved, size_t tsaved_bytes, void* jac_workspace, size_t jac_workspace_bytes, hipStream_t st);
int siren_supported(const sininn_siren_args* a, const char* who);
size_t siren_saved_bytes(int64_t n);
size_t siren_workspace_bytes(int64_t n);
int siren_forward_launch(const sininn_siren_args* a, const sininn_flownet_call* call, hipStream_t st);
int siren_backward_launch(const sininn_siren_args* a, const sininn_flownet_call* call, hipStream_t st);
size_t lamb_workspace_bytes(int64_t n_chunks, int n_tensors);
int lamb_grad_norm_launch(const sininn_lamb_args* a, hipStream_t st);
int lamb_step_launch(const sininn_lamb_args* a, hipStream_t st);
int64_t flow_epe_partials(int n, int h, int w);
int flow_epe_launch(const float* flow, int64_t flow_sample_stride, const float* gt, int n, int h, int w, double* partials,
                    int64_t n_partials, float* out, hipStream_t st);
int splat_mask_launch(const float* mask, int mask_channels, const float* splat, int n, int c, int h, int w, float* out, hipStream_t st);
int64_t flow2img_workspace_floats(int n, int h, int w);
int64_t flow_error_stash_workspace_floats(int B, int H, int W, int res);
int flow_error_stash_launch(const float* softmax1, const float* frame1, const float* mask1, const float* softmax2, const float* frame2,
                            const float* mask2, int mask_channels, int B, int C, int H, int W, const float* times, const float* ys,
                            const float* xs, int res, const float* centre, const float* scale, float* log_buffer, float* log_counter,
                            float* e_out, float* workspace, int64_t workspace_floats, hipStream_t st);
int flow2img_launch(const float* flow, int n, int h, int w, float clip, const double* wheel, int wheel_rows, float* workspace,
                    int64_t workspace_floats, uint8_t* img, hipStream_t st);
int64_t flow_synth_workspace(int B, int K, int C, int H, int W);
int flow_synth_launch(const float* i0, const float* i1, const float* f01, const float* f10, const float* tau, int B, int K, int C,
                      int H, int W, float* workspace, int64_t workspace_floats, float* out, uint8_t* out_u8, hipStream_t st);
int64_t frame_quality_workspace_floats(int B, int C, int H, int W);
int frame_quality_launch(const float* pred, const float* target, int B, int C, int H, int W, int quantize, const float* window,
                         float* workspace, int64_t workspace_floats, double* sqerr, float* out, float* ssim_map, hipStream_t st);
int flow_gather_launch(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                       const float* tau, int B, int K, int C, int H, int W, int k_loop, float* out, uint8_t* out_u8, hipStream_t st);
int flow_gather_visible_launch(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                               const float* tau, const float* m0, const float* m1, int B, int K, int C, int H, int W, int k_loop,
                               float* out, uint8_t* out_u8, hipStream_t st);
int64_t flow_gather_bwd_workspace(int B, int K, int H, int W);
int flow_gather_bwd_launch(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                           const float* tau, const float* grad_out, int B, int K, int C, int H, int W, int T, const int* reduce_list,
                           int64_t reduce_ints, float* workspace, int64_t workspace_floats, float* dflows, hipStream_t st);
int flow_gather_at_launch(const float* i0, const float* i1, const float* flows, const float* pix, const int* pair, const float* tau,
                          const uint8_t* rev, const float* blend, int R, int S, int64_t N, int B, int C, int H, int W, float* out,
                          hipStream_t st);
int flow_gather_at_bwd_launch(const float* i0, const float* i1, const float* flows, const float* pix, const int* pair, const float* tau,
                              const uint8_t* rev, const float* blend, const float* grad_out, int R, int S, int64_t N, int B, int C,
                              int H, int W, float* dflows, hipStream_t st);
int softsplat_fwd_launch(const float* in, const float* flow, int B, int C, int H, int W, float* out, hipStream_t st);
int softsplat_bwd_launch(const float* in, const float* flow, const float* gout, int B, int C, int H, int W, float* gin,
                         float* gflow, hipStream_t st);
int occlusion_wang_launch(const float* flow21, int B, int H, int W, float thresh, float* corr_zeroed, float* mask,
                          hipStream_t st);
int census_fwd_launch(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int H, int W,
                      int max_distance, float weight, float* acc_zeroed, float* out, hipStream_t st);
int census_bwd_launch(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int H, int W,
                      int max_distance, float weight, const float* acc, const float* gscale, float* g1, float* g2,
                      hipStream_t st);
int masked_l1_fwd_launch(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int C, int H, int W,
                         float weight, float* acc_zeroed, float* out, hipStream_t st);
int masked_l1_bwd_launch(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int C, int H, int W,
                         float weight, const float* acc, const float* gscale, float* g1, float* g2, hipStream_t st);
int brox_mask_launch(const float* fw, const float* warped_bw, int B, int H, int W, uint8_t* mask, hipStream_t st);
int ssim_fwd_launch(const float* im1, const float* im2, const float* mask, int MC, int B, int C, int H, int W, int md,
                    float weight, float* acc_zeroed, float* out, hipStream_t st);
int ssim_bwd_launch(const float* im1, const float* im2, const float* mask, int MC, int B, int C, int H, int W, int md,
                    float weight, const float* acc, const float* gscale, float* g1, float* g2, hipStream_t st);
int smooth_fwd_launch(const float* img, const float* flow, int B, int C, int H, int W, int order, int gauss, float k,
                      float weight, float* acc_zeroed, float* out, hipStream_t st);
int smooth_bwd_launch(const float* img, const float* flow, int B, int C, int H, int W, int order, int gauss, float k,
                      float weight, const float* gscale, float* gflow, hipStream_t st);
int pack_work_items(const sininn_pack_desc* d);
int pack_batch_launch(const sininn_pack_desc* descs, int n, int total, hipStream_t st);
int pack_winograd_launch(const float* w, int N, int Cin, const int* colmap, int Np, float* u_fwd, int Cdp,
                         float* u_dgrad, hipStream_t st);
int sample_pairs_planar_launch(const uint8_t* clip, const int* idx, int n, int T, int H, int W, int gap, void* out0, void* out1,
                               int bf16, hipStream_t st);
int bayer_demosaic_launch(const uint8_t* hr, uint8_t* rgb, int T, int H, int W, int scale, int reduce_sum, hipStream_t st);
int bayer_bin_launch(const uint8_t* hr, uint8_t* lr, int T, int H, int W, int scale, int reduce_sum, hipStream_t st);
size_t glow_saved_floats(int B, int H, int W, int C, int dtype);
size_t glow_scratch_bytes(int B, int H, int W, int C, int ksize, int dtype);
int glow_forward(const sininn_glow_args* a, hipStream_t st);
int glow_backward(const sininn_glow_args* a, hipStream_t st, hipStream_t wst);
int glow_hidden_gates(const sininn_glow_args* a, int which, unsigned char* gates, hipStream_t st);
bool group_major_fits(size_t M, int W);
}  // namespace sininn

using namespace sininn;
#define ST(s) static_cast<hipStream_t>(s)

extern "C" {

int sininn_version(void) { return SININN_ABI_VERSION; }
const char* sininn_last_error(void) { return g_err; }
// HIP streams at a priority torch.cuda.Stream cannot express (it clamps to {high, normal}): lower number = higher priority,
// the device's range is reported by sininn_stream_priority_range.  The handle is wrapped with torch.cuda.ExternalStream.
int sininn_stream_priority_range(int* least, int* greatest) {
  if (!least || !greatest) { set_error("stream_priority_range: null argument"); return 1; }
  hipError_t e = hipDeviceGetStreamPriorityRange(least, greatest);
  if (e != hipSuccess) { set_error("stream_priority_range: %s", hipGetErrorString(e)); return (int)e; }
  return 0;
}
int sininn_stream_create(int priority, void** stream) {
  if (!stream) { set_error("stream_create: null argument"); return 1; }
  hipStream_t s = nullptr;
  hipError_t e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority);
  if (e != hipSuccess) { set_error("stream_create(priority %d): %s", priority, hipGetErrorString(e)); return (int)e; }
  *stream = s;
  return 0;
}

/* Capture diagnostics: for each of `n` streams, is it part of the stream capture that `origin` started and is its work joined
 * back into origin?  flags[i] = 0 not capturing (or another capture), 1 capturing and every node at its frontier is an ancestor of
 * (or is at) origin's frontier, 2 capturing and UNJOINED: ending the capture now would fail (hipErrorStreamCaptureUnjoined).
 * Walks the graph under construction (hipStreamGetCaptureInfo_v2 + hipGraphGetEdges); launches nothing. */
int sininn_capture_unjoined(void* origin, void** streams, int n, int* flags) {
  if (!streams || !flags || n < 0) { set_error("capture_unjoined: null argument"); return 1; }
  hipStreamCaptureStatus st0 = hipStreamCaptureStatusNone;
  unsigned long long id0 = 0;
  hipGraph_t graph = nullptr;
  const hipGraphNode_t* deps0 = nullptr;
  size_t nd0 = 0;
  hipError_t e = hipStreamGetCaptureInfo_v2((hipStream_t)origin, &st0, &id0, &graph, &deps0, &nd0);
  if (e != hipSuccess) { set_error("capture_unjoined: %s", hipGetErrorString(e)); return (int)e; }
  for (int i = 0; i < n; ++i) flags[i] = 0;
  if (st0 != hipStreamCaptureStatusActive) return 0;
  size_t ne = 0;
  e = hipGraphGetEdges(graph, nullptr, nullptr, &ne);
  if (e != hipSuccess) { set_error("capture_unjoined: hipGraphGetEdges: %s", hipGetErrorString(e)); return (int)e; }
  std::vector<hipGraphNode_t> from(ne), to(ne);
  if (ne) {
    e = hipGraphGetEdges(graph, from.data(), to.data(), &ne);
    if (e != hipSuccess) { set_error("capture_unjoined: hipGraphGetEdges: %s", hipGetErrorString(e)); return (int)e; }
  }
  // ancestors of origin's frontier (reverse reachability)
  std::unordered_map<hipGraphNode_t, std::vector<hipGraphNode_t>> preds;
  for (size_t k = 0; k < ne; ++k) preds[to[k]].push_back(from[k]);
  std::unordered_set<hipGraphNode_t> anc;
  std::vector<hipGraphNode_t> stack(deps0, deps0 + nd0);
  while (!stack.empty()) {
    hipGraphNode_t v = stack.back(); stack.pop_back();
    if (!anc.insert(v).second) continue;
    auto it = preds.find(v);
    if (it != preds.end()) for (hipGraphNode_t p : it->second) stack.push_back(p);
  }
  for (int i = 0; i < n; ++i) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    const hipGraphNode_t* deps = nullptr;
    size_t nd = 0;
    hipGraph_t g = nullptr;
    if (hipStreamGetCaptureInfo_v2((hipStream_t)streams[i], &st, &id, &g, &deps, &nd) != hipSuccess) { (void)hipGetLastError(); continue; }
    if (st != hipStreamCaptureStatusActive || id != id0) continue;
    flags[i] = 1;
    for (size_t k = 0; k < nd; ++k)
      if (!anc.count(deps[k])) { flags[i] = 2; break; }
  }
  return 0;
}

size_t sininn_sizeof(int which) {
  switch (which) {
    case 0: return sizeof(sininn_conv_args);
    case 1: return sizeof(sininn_wgrad_item);
    case 2: return sizeof(sininn_dense_args);
    case 3: return sizeof(sininn_glow_args);
    case 4: return sizeof(sininn_subnet);
    case 5: return sizeof(sininn_pack_desc);
    case 6: return sizeof(sininn_dense_bf16_args);
    case 7: return sizeof(sininn_flownet_args);
    case 8: return sizeof(sininn_lamb_args);
    case 9: return sizeof(sininn_siren_args);
    case 10: return sizeof(sininn_flownet_call);
    default: return 0;
  }
}

int sininn_pack_conv_weights(const float* w_oihw, const float* bias, int N, int Cin, int ksize, const int* colmap,
                             int Np, float* w_fwd, float* b_fwd, int Cdp, float* w_dgrad, void* stream) {
  return pack_launch(w_oihw, bias, N, Cin, ksize, colmap, Np, w_fwd, b_fwd, Cdp, w_dgrad, ST(stream));
}

int sininn_softsplat(const float* in, const float* flow, int B, int C, int H, int W, float* out, void* stream) {
  return softsplat_fwd_launch(in, flow, B, C, H, W, out, ST(stream));
}
int sininn_softsplat_bwd(const float* in, const float* flow, const float* gout, int B, int C, int H, int W, float* gin,
                         float* gflow, void* stream) {
  return softsplat_bwd_launch(in, flow, gout, B, C, H, W, gin, gflow, ST(stream));
}
int sininn_occlusion_wang(const float* flow21, int B, int H, int W, float thresh, float* corr, float* mask, void* stream) {
  return occlusion_wang_launch(flow21, B, H, W, thresh, corr, mask, ST(stream));
}
int sininn_census(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int H, int W,
                  int max_distance, float weight, float* acc, float* out, void* stream) {
  return census_fwd_launch(im1, im2, mask, mask_channels, B, H, W, max_distance, weight, acc, out, ST(stream));
}
int sininn_census_bwd(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int H, int W,
                      int max_distance, float weight, const float* acc, const float* gscale, float* g1, float* g2,
                      void* stream) {
  return census_bwd_launch(im1, im2, mask, mask_channels, B, H, W, max_distance, weight, acc, gscale, g1, g2, ST(stream));
}
int sininn_masked_l1(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int C, int H, int W,
                     float weight, float* acc, float* out, void* stream) {
  return masked_l1_fwd_launch(im1, im2, mask, mask_channels, B, C, H, W, weight, acc, out, ST(stream));
}
int sininn_masked_l1_bwd(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int C, int H,
                         int W, float weight, const float* acc, const float* gscale, float* g1, float* g2, void* stream) {
  return masked_l1_bwd_launch(im1, im2, mask, mask_channels, B, C, H, W, weight, acc, gscale, g1, g2, ST(stream));
}
int sininn_occlusion_brox(const float* fw, const float* warped_bw, int B, int H, int W, uint8_t* mask, void* stream) {
  return brox_mask_launch(fw, warped_bw, B, H, W, mask, ST(stream));
}
int sininn_ssim(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int C, int H, int W, int md,
                float weight, float* acc, float* out, void* stream) {
  return ssim_fwd_launch(im1, im2, mask, mask_channels, B, C, H, W, md, weight, acc, out, ST(stream));
}
int sininn_ssim_bwd(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int C, int H, int W,
                    int md, float weight, const float* acc, const float* gscale, float* g1, float* g2, void* stream) {
  return ssim_bwd_launch(im1, im2, mask, mask_channels, B, C, H, W, md, weight, acc, gscale, g1, g2, ST(stream));
}
int sininn_bilateral_smooth(const float* img, const float* flow, int B, int C, int H, int W, int order, int gauss,
                            float edge_constant, float weight, float* acc, float* out, void* stream) {
  return smooth_fwd_launch(img, flow, B, C, H, W, order, gauss, edge_constant, weight, acc, out, ST(stream));
}
int sininn_bilateral_smooth_bwd(const float* img, const float* flow, int B, int C, int H, int W, int order, int gauss,
                                float edge_constant, float weight, const float* gscale, float* gflow, void* stream) {
  return smooth_bwd_launch(img, flow, B, C, H, W, order, gauss, edge_constant, weight, gscale, gflow, ST(stream));
}
int sininn_pack_work_items(const sininn_pack_desc* host_desc) { return host_desc ? pack_work_items(host_desc) : 0; }
int sininn_pack_batch(const sininn_pack_desc* descs, int n, int total_work, void* stream) {
  return pack_batch_launch(descs, n, total_work, ST(stream));
}
int sininn_pack_work_items_bf16(const sininn_pack_desc* host_desc) { return pack_work_items_bf16(host_desc); }
int sininn_pack_batch_bf16(const sininn_pack_desc* descs, int n, int total_work, void* stream) {
  return pack_batch_bf16_launch(descs, n, total_work, ST(stream));
}
int sininn_pack_winograd(const float* w_oihw, int N, int Cin, const int* colmap, int Np, float* u_fwd, int Cdp,
                         float* u_dgrad, void* stream) {
  return pack_winograd_launch(w_oihw, N, Cin, colmap, Np, u_fwd, Cdp, u_dgrad, ST(stream));
}

void sininn_coupling_colmap(int Co, int tile, int* colmap_host) {
  const int w = (tile == 32) ? 32 : 16, h = w / 2;
  for (int q = 0; q < 2 * Co; ++q) {
    const int t = q / w, j = q % w;
    colmap_host[q] = (j < h) ? (t * h + j) : (Co + t * h + j - h);
  }
}

int sininn_conv(const sininn_conv_args* args, void* stream) { return conv_launch(args, ST(stream)); }
int sininn_conv_pair_k1_supported(const sininn_conv_args* first, const sininn_conv_args* second) {
  return conv_pair_k1_supported(first, second);
}
int sininn_conv_pair_k1(const sininn_conv_args* first, const sininn_conv_args* second, void* stream) {
  return conv_pair_k1_launch(first, second, ST(stream));
}

int sininn_conv_sub1_fwd_supported(const sininn_conv_args* first, const sininn_conv_args* second) { return conv_sub1_fwd_supported(first, second); }
int sininn_conv_sub1_fwd(const sininn_conv_args* first, const sininn_conv_args* second, void* stream) { return conv_sub1_fwd_launch(first, second, ST(stream)); }
size_t sininn_conv_sub1_bwd_workspace_bytes(int cin, int co) { return conv_sub1_bwd_workspace_bytes(cin, co); }
int sininn_conv_sub1_bwd(const sininn_conv_args* recompute, const sininn_conv_args* d2, const sininn_conv_args* d1, int no_dx,
                         float* gw2, float* gb2, float* gw1, float* gb1, void* workspace, size_t workspace_bytes, void* stream) {
  int slabs = 0;
  if (int rc = conv_sub1_bwd_launch(recompute, d2, d1, no_dx, workspace, workspace_bytes, &slabs, ST(stream))) return rc;
  if (!gw2 && !gb2 && !gw1 && !gb1) return 0;
  return conv_sub1_bwd_reduce(recompute->Cin, d2->Cin / 2, workspace, slabs, gw2, gb2, gw1, gb1, ST(stream));
}
// the block executor's level-1 riders and gate-bit kernels, callable on their own (same internal functions, no other behaviour)
size_t sininn_conv_sub1_wide_bwd_workspace_bytes(int cin, int co) { return conv_sub1_bf16_wide_ws_bytes(1, 1, cin, co); }
int sininn_conv_sub1_wide_bwd(const sininn_conv_args* d2, const sininn_conv_args* d1, const float* x, int x_stride, float* gw1, float* gb1,
                              void* workspace, size_t workspace_bytes, void* stream) {
  SININN_CHECK(conv_sub1_bf16_wide_bwd_supported(d2, d1), "sininn_conv_sub1_wide_bwd: unsupported descriptor pair");
  if (!x) {
    SININN_CHECK(!gw1 && !gb1, "sininn_conv_sub1_wide_bwd: gw1 / gb1 need x");
    return conv_sub1_bf16_wide_bwd_launch(d2, d1, ST(stream));
  }
  int slabs = 0;
  if (int rc = conv_sub1_bf16_wide_bwd_wg1_launch(d2, d1, x, x_stride, workspace, workspace_bytes, &slabs, ST(stream))) return rc;
  if (!gw1 && !gb1) return 0;
  return conv_sub1_bf16_wide_reduce(workspace, slabs, gw1, gb1, ST(stream));
}
size_t sininn_conv_sub1_wide_wg2_workspace_bytes(int cin, int co) { return conv_sub1_bf16_wide_wg2_ws_bytes(1, 1, cin, co); }
int sininn_conv_sub1_wide_wg2(const float* dr, int dr_stride, const void* h, int h_stride, int B, int H, int W, float* gw2, float* gb2,
                              void* workspace, size_t workspace_bytes, void* stream) {
  SININN_CHECK(sininn_conv_sub1_wide_wg2_workspace_bytes(96, 96) > 0, "sininn_conv_sub1_wide_wg2: the wide kernels are switched off");
  return conv_sub1_bf16_wide_wg2_launch(dr, dr_stride, h, h_stride, B, H, W, workspace, workspace_bytes, gw2, gb2, ST(stream));
}
int sininn_conv3_smallk_bits_supported(const sininn_conv_args* args) { return conv3_smallk_bf16_supported(args); }
int sininn_conv3_smallk_bits(const sininn_conv_args* args, unsigned* bits, void* stream) {
  SININN_CHECK(bits != nullptr, "sininn_conv3_smallk_bits: bits is NULL");
  return conv3_smallk_bf16_launch_bits(args, bits, ST(stream));
}
// test hook: the block executor's fused 1x1 subnet backward on / off (A/B against the pair + grouped weight-gradient path)
void sininn_sub1_bwd_test_hook(int on) { conv_sub1_bwd_enable(on); conv3_smallk_enable(on); }   // every round-4 persistent kernel on / off

/* test hook (not part of the documented surface): force tile configuration / channel chunk */
void sininn_conv_test_hooks(int force_cfg, int force_ck) { conv_set_test_hooks(force_cfg, force_ck); }
void sininn_wgrad_test_hooks(int force16) { wgrad_set_force16(force16); }
// bit 0: fused 1x1 pairs on; bit 2: force the fused 3x3 subnet on, bit 1: force it off, neither: its default policy (SININN_SUB3)
void sininn_pair_k1_test_hook(int on) { conv_pair_k1_enable(on & 1); sub3_fusion_set((on & 4) ? 1 : ((on & 2) ? 0 : -1)); }
int sininn_conv_sub3_supported(const sininn_conv_args* first, const sininn_conv_args* second) {
  return conv_sub3_bf16_supported(first, second);
}
int sininn_conv_sub3(const sininn_conv_args* first, const sininn_conv_args* second, void* stream) {
  return conv_sub3_bf16_launch(first, second, ST(stream));
}

size_t sininn_wgrad_workspace_bytes(int N, int Cin, int ksize, int B, int H, int W) {
  return wgrad_workspace_bytes(N, Cin, ksize, B, H, W);
}
int sininn_wgrad(const float* in, int in_stride, int Cin, const float* dout, int dout_stride, int N, int B, int H, int W,
                 int ksize, float* gw_oihw, float* gbias, void* workspace, size_t workspace_bytes, void* stream) {
  return wgrad_launch(in, in_stride, Cin, dout, dout_stride, N, B, H, W, ksize, gw_oihw, gbias, workspace,
                      workspace_bytes, ST(stream));
}

int sininn_coupling_bwd(const float* dy, int dy_stride, const int* dy_map, const float* vy, int vy_stride,
                        const int* vy_map, const float* s, const float* gld, int B, int HW, int Co, float clamp,
                        int inverse, float* dr, float* dv, int dv_stride, void* stream) {
  return coupling_bwd_launch(dy, dy_stride, dy_map, vy, vy_stride, vy_map, s, gld, B, HW, Co, clamp, inverse, dr, dv,
                             dv_stride, ST(stream));
}

void sininn_profile_begin(int level_height, unsigned long long* stamps, int max_launches) {
  profile_begin(level_height, stamps, max_launches);
}
int sininn_wall_clock_khz(void) {
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return 0;
  return khz;
}
int sininn_profile_end(int* count, float* total_ms) { return profile_end(count, total_ms); }
size_t sininn_glow_saved_floats(int B, int H, int W, int C) { return glow_saved_floats(B, H, W, C, 0); }
size_t sininn_glow_saved_floats_dtype(int B, int H, int W, int C, int dtype) { return glow_saved_floats(B, H, W, C, dtype); }
size_t sininn_glow_scratch_bytes(int B, int H, int W, int C, int ksize) { return glow_scratch_bytes(B, H, W, C, ksize, 0); }
size_t sininn_glow_scratch_bytes_dtype(int B, int H, int W, int C, int ksize, int dtype) { return glow_scratch_bytes(B, H, W, C, ksize, dtype); }
int sininn_glow_forward(const sininn_glow_args* args, void* stream) { return glow_forward(args, ST(stream)); }
int sininn_glow_backward(const sininn_glow_args* args, void* stream, void* wgrad_stream) {
  return glow_backward(args, ST(stream), ST(wgrad_stream));
}

int sininn_haar(const float* in, const int64_t in_strides[4], float* out, const int64_t out_strides[4], int B, int C, int H,
                int W, int inverse, void* stream) {
  return haar_launch(in, in_strides, out, out_strides, B, C, H, W, inverse, ST(stream));
}
int sininn_lrelu_bwd(float* g, int g_stride, const float* f, int f_stride, int64_t M, int n, float slope, void* stream) {
  return lrelu_bwd_launch(g, g_stride, f, f_stride, M, n, slope, ST(stream));
}
int sininn_irn_coupling_bwd(const float* dy, int dy_stride, const float* vy, int vy_stride, const float* hval, int64_t M,
                            int Co, float clamp, int inverse, float* dG, float* dh, float* dv, int dv_stride,
                            void* stream) {
  return irn_coupling_bwd_launch(dy, dy_stride, vy, vy_stride, hval, M, Co, clamp, inverse, dG, Co, Co, dh, dv, dv_stride,
                                 ST(stream));
}

int sininn_irn_tail(const float* v, int v_stride, const float* h, const float* g, int64_t M, int Co, float clamp, int inverse,
                    float* out, int out_stride, void* stream) {
  return irn_tail_launch(v, v_stride, h, g, M, Co, clamp, inverse, out, out_stride, ST(stream));
}

int sininn_squeeze(const float* in, const int64_t in_strides[4], float* out, const int64_t out_strides[4], int B, int C,
                   int H, int W, int levels, int inverse, const int* chan_map, int map_on_out, void* stream) {
  return squeeze_launch(in, in_strides, out, out_strides, B, C, H, W, levels, inverse, chan_map, map_on_out, ST(stream));
}

int sininn_permute_channels(const float* in, int in_stride, float* out, int out_stride, int64_t M, int C,
                            const int* idx, void* stream) {
  return permute_launch(in, in_stride, out, out_stride, M, C, idx, ST(stream));
}

int sininn_sqdiff_sum(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4], int B, int C, int H,
                      int W, float* out, void* stream) {
  return sqdiff_sum_launch(x, xs, y, ys, B, C, H, W, out, ST(stream));
}
int sininn_sqdiff_bwd(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4], int B, int C, int H,
                      int W, const float* scale, float gscale, float* gx, const int64_t gxs[4], float* gy,
                      const int64_t gys[4], void* stream) {
  return sqdiff_bwd_launch(x, xs, y, ys, B, C, H, W, scale, gscale, gx, gxs, gy, gys, ST(stream));
}
int sininn_mmd_gram(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4], int B, int C, int H, int W,
                    float* g, void* stream) {
  return mmd_gram_launch(x, xs, y, ys, B, C, H, W, g, ST(stream));
}
int sininn_mmd_finish(const float* g, int B, int rev, float* out, float* coef, void* stream) {
  return mmd_finish_launch(g, B, rev, out, coef, ST(stream));
}
int sininn_mmd_bwd(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4], int B, int C, int H, int W,
                   const float* coef, const float* scale, float* gx, const int64_t gxs[4], float* gy,
                   const int64_t gys[4], void* stream) {
  return mmd_bwd_launch(x, xs, y, ys, B, C, H, W, coef, scale, gx, gxs, gy, gys, ST(stream));
}

int sininn_affine_warp(const float* img, const int64_t is[4], const float* theta, int B, int C, int H, int W, float* out,
                       const int64_t os[4], const float* ref, const int64_t rs[4], float* sse, void* stream) {
  return affine_warp_launch(img, is, theta, B, C, H, W, out, os, ref, rs, sse, ST(stream));
}
int sininn_affine_warp_bwd(const float* gout, const int64_t gs[4], const float* theta, int B, int C, int H, int W,
                           float* gimg, const int64_t gis[4], void* stream) {
  return affine_warp_bwd_launch(gout, gs, theta, B, C, H, W, gimg, gis, ST(stream));
}
int sininn_flow_warp_l1(const float* img, const float* flow, const float* target, int B, int C, int H, int W,
                        float* warped, float* metric, void* stream) {
  return flow_warp_l1_launch(img, flow, target, B, C, H, W, warped, metric, ST(stream));
}
int sininn_flow_warp_l1_bwd(const float* img, const float* flow, const float* target, const float* warped,
                            const float* gwarped, const float* gmetric, int B, int C, int H, int W, float* gimg,
                            float* gflow, void* stream) {
  return flow_warp_l1_bwd_launch(img, flow, target, warped, gwarped, gmetric, B, C, H, W, gimg, gflow, ST(stream));
}

int sininn_flow_warp_l1_bf16(const void* img, const float* flow, const void* target, int B, int C, int H, int W, void* warped,
                             float* metric, void* stream) {
  return flow_warp_l1_bf16_launch(img, flow, target, B, C, H, W, warped, metric, ST(stream));
}
int sininn_flow_warp_l1_bwd_bf16(const void* img, const float* flow, const void* target, const void* warped, const void* gwarped,
                                 const float* gmetric, int B, int C, int H, int W, float* gimg, float* gflow, void* stream) {
  return flow_warp_l1_bwd_bf16_launch(img, flow, target, warped, gwarped, gmetric, B, C, H, W, gimg, gflow, ST(stream));
}

int sininn_sample_windows(const uint8_t* hr_clip, const uint8_t* lr_clip, const int* idx, int n, int T, int H, int W,
                          int h, int w, int win, float* hr_out, const int64_t hs[4], float* lr_out, const int64_t ls[4],
                          void* stream) {
  return sample_windows_launch(hr_clip, lr_clip, idx, n, T, H, W, h, w, win, hr_out, hs, lr_out, ls, ST(stream));
}

int sininn_sample_pairs(const uint8_t* hr_clip, const int* idx, int n, int T, int H, int W, int gap, void* out0, void* out1,
                        int bf16, void* stream) {
  return sample_pairs_planar_launch(hr_clip, idx, n, T, H, W, gap, out0, out1, bf16, ST(stream));
}
int sininn_bayer_demosaic(const uint8_t* hr, uint8_t* rgb, int T, int H, int W, int scale, int reduce_sum, void* stream) {
  return bayer_demosaic_launch(hr, rgb, T, H, W, scale, reduce_sum, ST(stream));
}
int sininn_bayer_bin(const uint8_t* hr, uint8_t* lr, int T, int H, int W, int scale, int reduce_sum, void* stream) {
  return bayer_bin_launch(hr, lr, T, H, W, scale, reduce_sum, ST(stream));
}

size_t sininn_wgrad_group_workspace_bytes(const sininn_wgrad_item* items, int n, int B, int H, int W, int ksize) {
  return wgrad_group_workspace_bytes(items, n, B, H, W, ksize);
}
int sininn_wgrad_group(const sininn_wgrad_item* items, int n, int B, int H, int W, int ksize, void* workspace,
                       size_t workspace_bytes, void* stream) {
  return wgrad_group_launch(items, n, B, H, W, ksize, workspace, workspace_bytes, ST(stream));
}

int sininn_squeeze_rows(const float* in, float* out, int B, int C, int H, int W, int levels, int inverse,
                        const int* fine_map, void* stream) {
  return squeeze_rows_launch(in, out, B, C, H, W, levels, inverse, fine_map, ST(stream));
}

int sininn_pack_conv_weights_bf16(const float* w_oihw, const float* bias, int N, int Cin, int ksize, const int* colmap, int Np,
                                  void* wb_fwd, float* b_fwd, int Cdp, void* wb_dgrad, void* stream) {
  return pack_bf16_launch(w_oihw, bias, N, Cin, ksize, colmap, Np, wb_fwd, b_fwd, Cdp, wb_dgrad, ST(stream));
}

void sininn_profile_classes_begin(void) { profile_classes_begin(); }
int sininn_profile_classes_end(int n, double* ms, double* flops, int* launches) { return profile_classes_end(n, ms, flops, launches); }
int sininn_profile_classes_bytes(int n, double* bytes) { return profile_classes_bytes(n, bytes); }

int sininn_glow_group_major_fits(int B, int H, int W) { return group_major_fits((size_t)B * H * W, W) ? 1 : 0; }
int sininn_glow_hidden_gates(const sininn_glow_args* args, int which, uint8_t* gates, void* stream) {
  return glow_hidden_gates(args, which, gates, ST(stream));
}

size_t sininn_dense_workspace_bytes(int B, int H, int W, int cin, int cout) { return dense_workspace_bytes(B, H, W, cin, cout); }
int sininn_dense_forward(const sininn_dense_args* args, void* stream) { return dense_forward(args, ST(stream)); }
int sininn_dense_backward(const sininn_dense_args* args, void* stream, void* wgrad_stream) {
  return dense_backward(args, ST(stream), ST(wgrad_stream));
}
size_t sininn_dense_bf16_workspace_bytes(int B, int H, int W, int cin, int cout) {
  return dense_bf16_workspace_bytes(B, H, W, cin, cout);
}
int sininn_dense_forward_bf16(const sininn_dense_bf16_args* args, void* stream) { return dense_forward_bf16(args, ST(stream)); }
int sininn_dense_backward_bf16(const sininn_dense_bf16_args* args, void* stream, void* wgrad_stream) {
  return dense_backward_bf16(args, ST(stream), ST(wgrad_stream));
}

int sininn_frames_to_u8(const float* in, const int64_t in_strides[4], uint8_t* out, int B, int C, int H, int W, int wrap,
                        void* stream) {
  return frames_to_u8_launch(in, in_strides, out, B, C, H, W, wrap, ST(stream));
}

int sininn_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, float grad_scale, void* stream) {
  return adam_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, ST(stream));
}

int sininn_flownet_supported(const sininn_flownet_args* args) { return flownet_supported(args, "sininn_flownet_supported"); }
int sininn_flownet_supported_dim(const sininn_flownet_args* args, int domain_dim) {
  return flownet_supported_dim(args, domain_dim, "sininn_flownet_supported_dim");
}
size_t sininn_flownet_saved_bytes(int64_t n_points) { return flownet_saved_bytes(n_points); }
size_t sininn_flownet_workspace_bytes(int64_t n_points) { return flownet_workspace_bytes(n_points); }
size_t sininn_flownet_forward_workspace_bytes(const sininn_flownet_args* args) { return flownet_forward_workspace_bytes(args); }
int sininn_flownet_forward(const sininn_flownet_args* args, const sininn_flownet_call* call, void* stream) {
  return flownet_forward_launch(args, call, ST(stream));
}
int sininn_flownet_backward(const sininn_flownet_args* args, const sininn_flownet_call* call, void* stream) {
  return flownet_backward_launch(args, call, ST(stream));
}
int sininn_flownet_sample_mask(const sininn_flownet_args* args, const sininn_flownet_call* call, float* out, void* stream) {
  return flownet_sample_mask_launch(args, call, out, ST(stream));
}
size_t sininn_flownet_encgrad_workspace_bytes(const sininn_flownet_args* args) { return flownet_encgrad_workspace_bytes(args); }
size_t sininn_flownet_posegrad_workspace_bytes(const sininn_flownet_args* args, int with_enc_grad) {
  return flownet_posegrad_workspace_bytes(args, with_enc_grad);
}
size_t sininn_flownet_jacobian_saved_bytes(int64_t n_points, int n_dirs) { return flownet_jacobian_saved_bytes(n_points, n_dirs); }
size_t sininn_flownet_jacobian_workspace_bytes(const sininn_flownet_args* args, int64_t n_points, int n_dirs) {
  return flownet_jacobian_workspace_bytes(args, n_points, n_dirs);
}
int sininn_flownet_jacobian_forward(const sininn_flownet_args* args, const sininn_flownet_call* call, unsigned dirs, float* jac, float* tsaved,
                                    size_t tsaved_bytes, void* stream) {
  return flownet_jacobian_forward_launch(args, call, dirs, jac, tsaved, tsaved_bytes, ST(stream));
}
int sininn_flownet_jacobian_backward(const sininn_flownet_args* args, const sininn_flownet_call* call, unsigned dirs, const float* djac,
                                     const float* tsaved, size_t tsaved_bytes, void* jac_workspace, size_t jac_workspace_bytes, void* stream) {
  return flownet_jacobian_backward_launch(args, call, dirs, djac, tsaved, tsaved_bytes, jac_workspace, jac_workspace_bytes, ST(stream));
}
int sininn_siren_supported(const sininn_siren_args* args) { return siren_supported(args, "sininn_siren_supported"); }
size_t sininn_siren_saved_bytes(int64_t n_points) { return siren_saved_bytes(n_points); }
size_t sininn_siren_workspace_bytes(int64_t n_points) { return siren_workspace_bytes(n_points); }
int sininn_siren_forward(const sininn_siren_args* args, const sininn_flownet_call* call, void* stream) {
  return siren_forward_launch(args, call, ST(stream));
}
int sininn_siren_backward(const sininn_siren_args* args, const sininn_flownet_call* call, void* stream) {
  return siren_backward_launch(args, call, ST(stream));
}

size_t sininn_lamb_workspace_bytes(int64_t n_chunks, int n_tensors) { return lamb_workspace_bytes(n_chunks, n_tensors); }
int sininn_lamb_grad_norm(const sininn_lamb_args* args, void* stream) { return lamb_grad_norm_launch(args, ST(stream)); }
int sininn_lamb_step(const sininn_lamb_args* args, void* stream) { return lamb_step_launch(args, ST(stream)); }

int64_t sininn_flow_epe_partials(int n, int h, int w) { return flow_epe_partials(n, h, w); }
int sininn_flow_epe(const float* flow, int64_t flow_sample_stride, const float* gt, int n, int h, int w, double* partials,
                    int64_t n_partials, float* out, void* stream) {
  return flow_epe_launch(flow, flow_sample_stride, gt, n, h, w, partials, n_partials, out, ST(stream));
}
int sininn_splat_mask(const float* mask, int mask_channels, const float* splat, int n, int c, int h, int w, float* out, void* stream) {
  return splat_mask_launch(mask, mask_channels, splat, n, c, h, w, out, ST(stream));
}
int64_t sininn_flow_error_stash_workspace_floats(int B, int H, int W, int res) { return flow_error_stash_workspace_floats(B, H, W, res); }
int sininn_flow_error_stash(const float* softmax1, const float* frame1, const float* mask1, const float* softmax2, const float* frame2,
                            const float* mask2, int mask_channels, int B, int C, int H, int W, const float* times, const float* ys,
                            const float* xs, int res, float centre_t, float centre_y, float centre_x, float scale_t, float scale_y,
                            float scale_x, float* log_buffer, float* log_counter, float* E, float* workspace, int64_t workspace_floats,
                            void* stream) {
  const float centre[3] = {centre_t, centre_y, centre_x}, scale[3] = {scale_t, scale_y, scale_x};
  return flow_error_stash_launch(softmax1, frame1, mask1, softmax2, frame2, mask2, mask_channels, B, C, H, W, times, ys, xs, res, centre,
                                 scale, log_buffer, log_counter, E, workspace, workspace_floats, ST(stream));
}
int64_t sininn_flow2img_workspace_floats(int n, int h, int w) { return flow2img_workspace_floats(n, h, w); }
int sininn_flow2img(const float* flow, int n, int h, int w, float clip, const double* wheel, int wheel_rows, float* workspace,
                    int64_t workspace_floats, uint8_t* img, void* stream) {
  return flow2img_launch(flow, n, h, w, clip, wheel, wheel_rows, workspace, workspace_floats, img, ST(stream));
}

int64_t sininn_flow_synth_workspace(int B, int K, int C, int H, int W) { return flow_synth_workspace(B, K, C, H, W); }
int sininn_flow_synth(const float* i0, const float* i1, const float* f01, const float* f10, const float* tau, int B, int K, int C,
                      int H, int W, float* workspace, int64_t workspace_floats, float* out, unsigned char* out_u8, void* stream) {
  return flow_synth_launch(i0, i1, f01, f10, tau, B, K, C, H, W, workspace, workspace_floats, out, out_u8, ST(stream));
}

int64_t sininn_frame_quality_workspace_floats(int B, int C, int H, int W) { return frame_quality_workspace_floats(B, C, H, W); }
int sininn_frame_quality(const float* pred, const float* target, int B, int C, int H, int W, int quantize, const float* window,
                         float* workspace, int64_t workspace_floats, double* sqerr, float* out, float* ssim_map, void* stream) {
  return frame_quality_launch(pred, target, B, C, H, W, quantize, window, workspace, workspace_floats, sqerr, out, ssim_map,
                              ST(stream));
}

int sininn_flow_gather(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                       const float* tau, int B, int K, int C, int H, int W, int k_loop, float* out, unsigned char* out_u8,
                       void* stream) {
  return flow_gather_launch(i0, i1, flows, flow_sample_stride, slots, tau, B, K, C, H, W, k_loop, out, out_u8, ST(stream));
}

int sininn_flow_gather_visible(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                               const float* tau, const float* m0, const float* m1, int B, int K, int C, int H, int W, int k_loop,
                               float* out, unsigned char* out_u8, void* stream) {
  return flow_gather_visible_launch(i0, i1, flows, flow_sample_stride, slots, tau, m0, m1, B, K, C, H, W, k_loop, out, out_u8,
                                    ST(stream));
}

int64_t sininn_flow_gather_bwd_workspace(int B, int K, int H, int W) { return flow_gather_bwd_workspace(B, K, H, W); }
int sininn_flow_gather_bwd(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                           const float* tau, const float* grad_out, int B, int K, int C, int H, int W, int T, const int* reduce_list,
                           int64_t reduce_ints, float* workspace, int64_t workspace_floats, float* dflows, void* stream) {
  return flow_gather_bwd_launch(i0, i1, flows, flow_sample_stride, slots, tau, grad_out, B, K, C, H, W, T, reduce_list, reduce_ints,
                                workspace, workspace_floats, dflows, ST(stream));
}

int sininn_flow_gather_at(const float* i0, const float* i1, const float* flows, const float* pix, const int* pair, const float* tau,
                          const unsigned char* rev, const float* blend, int R, int S, int64_t N, int B, int C, int H, int W, float* out,
                          void* stream) {
  return flow_gather_at_launch(i0, i1, flows, pix, pair, tau, rev, blend, R, S, N, B, C, H, W, out, ST(stream));
}

int sininn_flow_gather_at_bwd(const float* i0, const float* i1, const float* flows, const float* pix, const int* pair,
                              const float* tau, const unsigned char* rev, const float* blend, const float* grad_out, int R, int S,
                              int64_t N, int B, int C, int H, int W, float* dflows, void* stream) {
  return flow_gather_at_bwd_launch(i0, i1, flows, pix, pair, tau, rev, blend, grad_out, R, S, N, B, C, H, W, dflows, ST(stream));
}

}  // extern "C"
