/*
 * sininn.h -- C ABI of libsininn.so: the MI355X (gfx950) kernels behind the sin-inn
 * single-video INN training path.
 *
 * Boundary rules:
 *   - extern "C", plain pointers and sizes only; no torch types.
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch allocates and frees);
 *     the library borrows it for the duration of the call and never allocates device memory.
 *     Scratch is a caller-provided workspace pointer + size in bytes.
 *   - every call is an asynchronous launch on the hipStream_t passed as `stream`
 *     (torch.cuda.current_stream().cuda_stream); no internal threads, no hidden syncs.
 *   - return value: 0 on success, non-zero on error (argument check or hipError_t);
 *     sininn_last_error() returns a thread-local message.  The Python side turns this into
 *     RuntimeError, mirroring the assert / NotImplementedError convention of the reference's only
 *     raw-pointer kernel call site (video-interpolation/my_utils/softsplat.py:239-331).
 *   - activations are fp32 NHWC ("pixel-major"): element (b,y,x,c) of a tensor with C channels
 *     and pixel stride `stride` floats lives at ((b*H+y)*W+x)*stride + c.  A channel sub-range is
 *     addressed by offsetting the base pointer (stride stays the full pixel stride).
 *
 * All file:line citations are into the reference repository (paramhanji/sin-inn).
 */
#ifndef SININN_H
#define SININN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* stays 4 although the flow-network entry points changed: the in-tree ctypes binding is the library's only consumer and checks every symbol
 * and every struct size when it loads it */
#define SININN_ABI_VERSION 4
#define SININN_HIDDEN 256 /* hidden width of subnet_conv / subnet_conv_1x1, archs.py:12,16 */

int sininn_version(void);
const char* sininn_last_error(void);
/* sizeof() of descriptor struct `which` as THIS library was compiled: 0 sininn_conv_args, 1 sininn_wgrad_item,
 * 2 sininn_dense_args, 3 sininn_glow_args, 4 sininn_subnet, 5 sininn_pack_desc, 6 sininn_dense_bf16_args, 7 sininn_flownet_args, 8 sininn_lamb_args, 9 sininn_siren_args; 0 for an unknown index.  A binding written in
 * another language (the ctypes mirrors in sin-inn_amd/_lib.py) checks its own layout against it at load time (ABI v4). */
size_t sininn_sizeof(int which);
/* A HIP stream at an explicit priority (lower number = higher priority; range from sininn_stream_priority_range: `least` is the
 * numerically largest, lowest priority).  torch.cuda.Stream only offers {high, normal}; the weight-gradient stream of the
 * training step can be created LOW with this (SININN_WGRAD_PRIO) and wrapped with torch.cuda.ExternalStream.  The stream lives
 * until the process exits.  ABI v4. */
int sininn_stream_priority_range(int* least, int* greatest);
int sininn_stream_create(int priority, void** stream);
/* Stream-capture diagnostics (hipGraph replay of the pass chains, lit_wrapper._graph_step): which of `n` helper streams belong to
 * the capture that `origin` started and still hold work that is NOT joined back into origin.  flags[i]: 0 not part of it,
 * 1 capturing and joined, 2 capturing and unjoined (hipStreamEndCapture on origin would fail).  Host-only graph walk. */
int sininn_capture_unjoined(void* origin, void** streams, int n, int* flags);

/* ------------------------------------------------------------------------------------------------
 * Weight packing.  Source: torch Conv2d weight, OIHW fp32 [N][Cin][k][k] (archs.py:12-13,16-17).
 *   w_fwd  [taps][Np ][Cin ]  row q holds output channel colmap[q] (or q when colmap==NULL; rows
 *                             whose source index is <0 or >=N are zero)  -- B operand of the conv.
 *   w_dgrad[taps][Cdp][N   ]  w_dgrad[t][c][n] = w[n][c][taps-1-t]       -- B operand of the
 *                             data-gradient conv (input channels N, output channels Cin padded to
 *                             Cdp, rows c>=Cin zero).
 *   b_fwd  [Np] packed bias (may be NULL together with bias).
 * Either destination may be NULL.
 * ---------------------------------------------------------------------------------------------- */
int sininn_pack_conv_weights(const float* w_oihw, const float* bias, int N, int Cin, int ksize,
                             const int* colmap, int Np, float* w_fwd, float* b_fwd,
                             int Cdp, float* w_dgrad, void* stream);

/* bf16 packs for the mixed-precision convs: wb_fwd [taps][Np][Kp] (Kp = Cin rounded up to 16, zero filled), b_fwd [Np]
 * fp32 (packed bias), wb_dgrad [taps][Cdp][Kd] (Kd = N rounded up to 16; flipped taps).  Either destination may be NULL. */
int sininn_pack_conv_weights_bf16(const float* w_oihw, const float* bias, int N, int Cin, int ksize,
                                  const int* colmap, int Np, void* wb_fwd, float* b_fwd,
                                  int Cdp, void* wb_dgrad, void* stream);

/* Winograd F(2x2,3x3) filter transform of a 3x3 conv weight (U = G g G^T), same row / column conventions as
 * sininn_pack_conv_weights with the tap axis replaced by the 16 transform positions:
 *   u_fwd [16][Cin/8][Np][8], u_dgrad [16][N/8][Cdp][8] (flipped taps): channel-chunk-major, so the 8-channel chunk a
 *   kernel iteration stages is contiguous per position.  Either destination may be NULL. */
int sininn_pack_winograd(const float* w_oihw, int N, int Cin, const int* colmap, int Np, float* u_fwd,
                         int Cdp, float* u_dgrad, void* stream);

/* All weight packs of a model in ONE launch (the optimiser step invalidates every pack at once; 48 small pack
 * launches per training step cost ~0.2 ms).  `descs` is a DEVICE array of n descriptors; destinations and
 * conventions are those of sininn_pack_conv_weights (wino_* == 0) / sininn_pack_winograd (wino_* != 0, ksize 3);
 * b_fwd (packed bias) is written whenever it is non-NULL.  work_begin = exclusive prefix sum of
 * sininn_pack_work_items over the array (host-computed), total_work = its grand total. */
typedef struct sininn_pack_desc {
  const float* w; const float* bias; int N, Cin, ksize; const int* colmap; int Np;
  float* w_fwd; float* b_fwd; int Cdp; float* w_dgrad; int wino_fwd, wino_dgrad;
  int work_begin;
  /* ABI v4, zero = as before.  N / Cin above are the PACKED dimensions; the source weight may be smaller: src_n outputs
   * (0 = N; packed outputs beyond it are zero) and Cin - gap_len input channels, the packed input channels [gap_begin,
   * gap_begin + gap_len) being zero padding it does not have (IRN DenseBlock: channel_in padded to a multiple of 8 inside
   * the feature buffer, archs.py:74-98).  Lets every pack of an IRN model join the one batched refresh launch. */
  int src_n, gap_begin, gap_len;
} sininn_pack_desc;
int sininn_pack_work_items(const sininn_pack_desc* host_desc);
int sininn_pack_batch(const sininn_pack_desc* descs, int n, int total_work, void* stream);
/* The same batched refresh for bf16 packs (sininn_pack_conv_weights_bf16 layouts: w_fwd [taps][Np][pad16(Cin)] and
 * w_dgrad [taps][Cdp][pad16(N)] hold bf16, b_fwd fp32), with src_n / gap_begin / gap_len as above; wino_* must be 0.
 * work_begin is the prefix sum of sininn_pack_work_items_bf16 (0 for a descriptor this layout cannot serve). */
int sininn_pack_work_items_bf16(const sininn_pack_desc* host_desc);
int sininn_pack_batch_bf16(const sininn_pack_desc* descs, int n, int total_work, void* stream);

/* Packed column order used by the coupling epilogue for a subnet with 2*Co outputs (s | t):
 * `tile`-column MFMA tile q = [ s[h*q .. h*q+h-1] | t[h*q .. h*q+h-1] ], h = tile/2, tile in {16, 32}
 * (tile 32 needs Co % 16 == 0).  Writes 2*Co ints (host memory).  The same `tile` must be passed as
 * sininn_conv_args.col_tile. */
void sininn_coupling_colmap(int Co, int tile, int* colmap_host);

/* ------------------------------------------------------------------------------------------------
 * Convolution engine (implicit GEMM on v_mfma_f32_16x16x4_f32, LDS-staged halo tiles).
 * One entry point, epilogue selected by `mode`.  Replaces nn.Conv2d + the elementwise tail of
 * FrEIA's GLOWCouplingBlock.forward (call site archs.py:61-64).
 * ---------------------------------------------------------------------------------------------- */
enum sininn_conv_mode {
  SININN_CONV_RELU = 0,       /* out = relu(conv + bias)                    (archs.py:12,16: Conv+ReLU)   */
  SININN_CONV_COUPLE_FWD = 1, /* y = exp(log_e(s)) * v + t ; logdet += sum log_e(s)                        */
  SININN_CONV_COUPLE_INV = 2, /* y = (v - t) / exp(log_e(s)) ; logdet -= sum log_e(s)                      */
  SININN_CONV_MASK = 3,       /* out = conv * (mask > 0)   (data gradient through the ReLU)                */
  SININN_CONV_ADD = 4,        /* out = conv (+ bias if given) + addend[addend_map]   (data gradient + skip grad;
                                 with bias: y1 = x1 + F(x2), archs.py:151)                                  */
  SININN_CONV_LINEAR = 5,     /* out = conv + bias                                                          */
  /* LINEAR and ADD with `mask` != NULL (ABI v4): a LeakyReLU-backward tail -- output columns c >= Co are multiplied by
   * (mask[pix * mask_stride + c] > 0 ? 1 : clamp).  The data gradient of DenseBlock conv k+1 finalises the gradient of
   * feature slot k in its last 32 columns; the LeakyReLU backward of that slot (archs.py:90-93) rides in its epilogue
   * instead of being a launch of its own (192 launches per IRN training step). */
  /* IRN architecture (archs.py:74-160): */
  SININN_CONV_LRELU = 6,      /* out = leaky_relu(conv + bias, slope = clamp)        (DenseBlock conv1-4, archs.py:90-93) */
  SININN_CONV_IRN_FWD = 7,    /* out = v * exp(clamp*(2*sigmoid(aux)-1)) + conv + bias  (InvBlockExp, archs.py:152-153;
                                 aux = H(y1) is passed in the mask / mask_stride fields)                     */
  SININN_CONV_IRN_INV = 8,    /* out = (v - (conv + bias)) / exp(clamp*(2*sigmoid(aux)-1))   (archs.py:155-156)        */
  /* data gradient of a subnet's first conv fused with the NEXT coupling tail's backward (saves a launch and the
   * round trip of the intermediate gradient): g = conv + addend[addend_map]; then exactly sininn_coupling_bwd on g:
   *   out  [M][2*Co] = (ds | dt), out_stride = 2*Co;  out2 = dv (stride out2_stride);  v = v (FWD) or y (INV);
   *   sbuf = s [M][Co] (read);  logdet = optional per-sample log-det gradient [B] (read);  N = Co. */
  SININN_CONV_ADD_CBWD_FWD = 9,
  SININN_CONV_ADD_CBWD_INV = 10
};

typedef struct sininn_conv_args {
  const float* in;   int in_stride;  int Cin;      /* Cin % 8 == 0                                         */
  const float* w;    const float* bias; int Np;    /* packed weights [taps][Np][Cin], Np % 16 == 0         */
  int winograd;                                    /* 1: w is the Winograd pack U[16][Np][Cin] (ksize 3, Np % 32 == 0) */
  int B, H, W, ksize;                              /* ksize 1 or 3, zero padding ksize/2                   */
  int mode;
  float* out;        int out_stride; int N;        /* generic modes: N valid output columns                */
  const int* out_map;                              /* coupling modes: y channel c -> out channel (or NULL) */
  const float* v;    int v_stride;                 /* coupling: transformed half                           */
  float* out2;       int out2_stride;              /* coupling: optional compact copy of y                 */
  float* sbuf;                                     /* coupling: optional [M][Co] copy of s (for backward)  */
  float* logdet;                                   /* coupling: optional [B], accumulated with atomics     */
  int Co;            float clamp;                  /* coupling: channels transformed, GLOW clamp           */
  int col_tile;                                    /* coupling: 16 or 32, the (s|t) interleave of the weights */
  const float* mask; int mask_stride;              /* MASK mode                                            */
  const float* addend; int addend_stride; const int* addend_map; /* ADD mode                               */
  unsigned long long* stamp;                       /* optional device words {start, end}: every block folds its entry /
                                                      exit time (wall-clock ticks, sininn_wall_clock_khz) in with atomic
                                                      min / max; initialise to {~0ull >> 1, 0}                       */
  /* ---- mixed-precision path (ABI version 2): bf16 operands on v_mfma_f32_32x32x16_bf16, fp32 accumulate + epilogue ---- */
  int w_bf16;                                      /* w is a bf16 pack [taps][Np][Kp] (sininn_pack_conv_weights_bf16): selects
                                                      the bf16 kernel; the fields below apply only then                   */
  int in_bf16;                                     /* `in` holds bf16 (stride in elements, Cin % 8 == 0); else fp32, converted
                                                      to bf16 (round to nearest even) while it is staged                  */
  int out_bf16;                                    /* `out` holds bf16 (RELU / LINEAR / MASK modes; an fp32-input conv must
                                                      set it); else fp32 through the mode's regular epilogue              */
  int mask_bf16;                                   /* MASK mode: `mask` holds bf16                                        */
  /* channel-group-major tensors [C/8][B*H*W][8] (Winograd kernels; the hidden tensors h / dh of a 3x3 GLOW block, which only
   * the block executor's kernels touch): every halo row of an 8-channel chunk is then one contiguous run.  A value > 0 is the
   * number of floats between channel groups (= B*H*W*8) and selects the layout for that operand: */
  int in_group_stride;                             /* `in` (then in_stride must be 8)                                     */
  int out_group_stride;                            /* `out` (RELU / MASK modes, N == Np, N % 64 == 0)                      */
  int mask_group_stride;                           /* `mask` (MASK mode)                                                  */
} sininn_conv_args;

/* Size limits (checked on the host, refused with sininn_last_error): B*H*W*stride of every operand < 2^31 elements; for
 * winograd = 1 and for sininn_conv_pair_k1 one IMAGE of the input (H*W*in_stride floats) < 2 GB -- the kernels stage through
 * raw buffer loads with 32-bit byte offsets inside the block's image (1280x720 at 1/4 scale with 256 channels is 59 MB). */
int sininn_conv(const sininn_conv_args* args, void* stream);

/* Two chained 1x1 convs of a GLOW subnet in one launch (subnet_conv_1x1, archs.py:15-17, called from FrEIA's
 * GLOWCouplingBlock, archs.py:56-64): `first` produces the 256-channel hidden tensor (mode RELU: h = relu(x W1 + b1), or
 * mode MASK: dh = (dr W2) . [h > 0]), `second` consumes it (any non-IRN mode: the coupling epilogues forward, the skip-add /
 * fused coupling-backward epilogues backward).  The hidden tile stays in LDS between the two GEMMs; it is still written to
 * first->out once (training needs it) unless first->out is NULL (no-grad passes: the hidden tensor never reaches HBM;
 * second->in is then ignored).  Same results as sininn_conv(first) followed by sininn_conv(second) up to fp32 summation
 * order.  Pixel-major operands only; fp32 pairs, or mixed-precision pairs (both convs w_bf16: first fp32 in -> bf16 hidden
 * tensor, second bf16 hidden tensor -> fp32 epilogue; the hidden values are rounded to bf16 exactly once, as in the two-launch
 * path).  sininn_conv_pair_k1_supported returns 1 when the pair's shapes / modes qualify (hidden width 256, first->Cin % 8 == 0
 * and <= 192, second->Np in {16, 32, 48, 64, 96, 192}). */
int sininn_conv_pair_k1_supported(const sininn_conv_args* first, const sininn_conv_args* second);
int sininn_conv_pair_k1(const sininn_conv_args* first, const sininn_conv_args* second, void* stream);

/* The fp32 1x1 subnet + affine coupling + log-det of a GLOW half-coupling as ONE persistent launch (round 4; subnet_conv_1x1,
 * archs.py:15-17, inside FrEIA's GLOWCouplingBlock, archs.py:56-64): the twin of sininn_conv_pair_k1 for the shapes
 * (Cin of conv1, 2 Co) in {(8, 16), (16, 32), (24, 48)} -- level 0 of the SRF network.  A block per CU keeps conv2's pack in LDS and
 * its conv1 fragments in registers over all of its 64-pixel tiles; the hidden tensor is never stored (first->out is ignored: the
 * matching backward, sininn_conv_sub1_bwd, recomputes it).  first: mode RELU; second: mode COUPLE_FWD / COUPLE_INV, described as
 * for sininn_conv_pair_k1.  Same values as the pair up to fp32 summation order (K = 256 is summed in two halves).
 * Mixed precision (both convs w_bf16, described as for the mixed-precision pair): the same entry points run the bf16 twins
 * (csrc/conv_sub1_bf16.hip: bf16 operands, fp32 accumulation / epilogue; h is rounded to bf16 once, bitwise as in the pair). */
int sininn_conv_sub1_fwd_supported(const sininn_conv_args* first, const sininn_conv_args* second);
int sininn_conv_sub1_fwd(const sininn_conv_args* first, const sininn_conv_args* second, void* stream);

/* The whole BACKWARD of a fp32 1x1 conv subnet of a GLOW half-coupling in one persistent launch + one slab reduce (round 4;
 * subnet_conv_1x1, archs.py:15-17, differentiated inside FrEIA's GLOWCouplingBlock, archs.py:56-64):
 *   h = relu(x W1^T + b1) is RECOMPUTED from the subnet's input (the forward pass need not store it: pass first->out == NULL to
 *   sininn_conv_pair_k1), dh = (dr W2) . [h > 0] never leaves the chip, dx = dh W1 goes through d1's epilogue (ADD / ADD_CBWD_*),
 *   and gw2 / gb2 / gw1 / gb1 (OIHW, +=; any of them may be NULL) are summed from per-block slabs in a fixed order.
 * recompute: {in = x, in_stride, Cin, w = forward pack of conv1 [256][Cin], bias, Np = 256, B, H, W, ksize = 1}; d2 / d1: the two
 * data-gradient convs exactly as for sininn_conv_pair_k1 (d2: in = dr [.. 2 Co], w = data-gradient pack of conv2; d1: Cin = 256,
 * w = data-gradient pack of conv1, Np = pad16(Cin of conv1), the epilogue fields); d2->mask / d2->out / d1->in are ignored.
 * Shapes served: (Cin of conv1, 2 Co) in {(8, 16), (16, 32), (24, 48)} -- sininn_conv_sub1_bwd_workspace_bytes returns 0 for any
 * other.  dx / the fused coupling backward are bitwise what sininn_conv_pair_k1(d2, d1) produces from the stored h; the weight
 * gradients agree with sininn_wgrad up to fp32 summation order.  no_dx != 0: the data gradient of conv1 is not needed.
 * Mixed precision: recompute / d2 / d1 with w_bf16 = 1 (bf16 packs; x, dr, dx and the gradients stay fp32) select the bf16 twin. */
size_t sininn_conv_sub1_bwd_workspace_bytes(int cin, int co);
int sininn_conv_sub1_bwd(const sininn_conv_args* recompute, const sininn_conv_args* d2, const sininn_conv_args* d1, int no_dx,
                         float* gw2, float* gb2, float* gw1, float* gb1, void* workspace, size_t workspace_bytes, void* stream);

/* The mixed-precision backward of the WIDE (level-1) 1x1 subnet, as the block executor runs it: one persistent launch for both data
 * gradients with the weight gradient of conv1 riding along, then one slab reduce (the same kernels sininn_glow_backward uses; ABI v4):
 *   dh = (dr W2) . [h > 0] (bf16, stored to d2->out unless it is NULL), dx = dh W1 through d1's epilogue (ADD / ADD_CBWD_*),
 *   gw1 [256][96] += dh^T x, gb1 [256] += sum dh (OIHW, fp32; x fp32 [pixel][x_stride], dh summed as the bf16 values above).
 * d2: in = dr fp32 [.. 192], w = bf16 data-gradient pack of conv2, Np = N = 256, mode MASK, mask = h (bf16, the forward's hidden
 * tensor), mask_bf16 = out_bf16 = 1; d1: in_bf16 = 1, Cin = 256, w = bf16 data-gradient pack of conv1, Np = N = 96, mode ADD or
 * ADD_CBWD_FWD / _INV with the epilogue fields of sininn_conv_pair_k1 (d1->in is ignored: dh stays on chip).  Shape served:
 * (Cin of conv1, 2 Co) = (96, 192); an unsupported descriptor pair is refused with an error.  x == NULL: no rider (gw1 / gb1
 * must then be NULL, the workspace is not used).  sininn_conv_sub1_wide_bwd_workspace_bytes returns 0 for any other shape. */
size_t sininn_conv_sub1_wide_bwd_workspace_bytes(int cin, int co);
int sininn_conv_sub1_wide_bwd(const sininn_conv_args* d2, const sininn_conv_args* d1, const float* x, int x_stride, float* gw1, float* gb1,
                              void* workspace, size_t workspace_bytes, void* stream);
/* ... and the weight gradient of its conv2, the executor's other rider (a persistent kernel + slab reduce on the weight-gradient
 * stream): gw2 [192][256] += dr^T h, gb2 [192] += sum dr (OIHW, fp32), dr fp32 [pixel][dr_stride] in conv2's OIHW channel order
 * (ds | dt), h bf16 [pixel][h_stride].  (cin, co) = (96, 96) only; the workspace size is 0 for any other shape. */
size_t sininn_conv_sub1_wide_wg2_workspace_bytes(int cin, int co);
int sininn_conv_sub1_wide_wg2(const float* dr, int dr_stride, const void* h, int h_stride, int B, int H, int W, float* gw2, float* gb2,
                              void* workspace, size_t workspace_bytes, void* stream);

/* The small-K 3x3 kernel of a level-0 subnet on the mixed-precision path WITH the ReLU-gate bit mask, as the block executor runs it
 * in training passes (ABI v4).  args: either conv1 (ksize 3, w_bf16, fp32 input with Cin in {8, 16, 24, 32}, bias, mode RELU, Np = N
 * = 256, out_bf16: h = relu(conv + bias) as bf16) -- it WRITES `bits`; or the masked data gradient of conv2 (fp32 dr with Cin in
 * {16, 32, 48}, mode MASK, Np = N = 256, out_bf16, mask_bf16 with a valid mask descriptor) -- it READS the gates from `bits`
 * instead of `mask`.  sininn_conv3_smallk_bits_supported returns 1 when the descriptor qualifies.
 * Bit layout: [pixel][8] 32-bit words over the image padded to 16 x 16 tiles, B * pad16(H) * pad16(W) * 8 words in all: the
 * tile (b, ty, tx) (tile = (b * ceil(H/16) + ty) * ceil(W/16) + tx) owns words [tile * 2048, tile * 2048 + 2048); word
 * (tile * 8 + m) * 256 + c holds, in bit p, the gate [h > 0] of hidden column c at pixel (16 ty + 2 m + p / 16, 16 tx + p % 16).
 * Bits of pixels outside the image (the padding of the last tile row / column) are unspecified and never read. */
int sininn_conv3_smallk_bits_supported(const sininn_conv_args* args);
int sininn_conv3_smallk_bits(const sininn_conv_args* args, unsigned* bits, void* stream);

/* The 3x3 twin for passes that keep nothing for a backward (ABI v4): the WHOLE 3x3 conv subnet (subnet_conv, archs.py:11-13) +
 * affine coupling + log-det of a GLOW half-coupling (archs.py:56-64) in one launch on the mixed-precision path.  `first`:
 * ksize 3, bf16 weights, fp32 input, mode RELU, 256 output channels, out == NULL (the hidden tile lives in LDS only);
 * `second`: ksize 3, bf16 weights, Cin 256, mode COUPLE_FWD / COUPLE_INV (same kernel for both directions), Np in {16, 32,
 * 48, 64, 96, 192}.  Same values as the two sininn_conv launches with a bf16 hidden tensor (one rounding of h to bf16) up to
 * fp32 summation order.  sininn_glow_forward dispatches it for dtype == 1, ksize == 3, no_save != 0 when SININN_SUB3=1 is set in the
 * environment (not the default: on MI355X it measures 1.8 - 2.7x slower than the two launches it replaces). */
int sininn_conv_sub3_supported(const sininn_conv_args* first, const sininn_conv_args* second);
int sininn_conv_sub3(const sininn_conv_args* first, const sininn_conv_args* second, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Weight gradient: dW[n][c][tap] += sum_pixels dout[pix][n] * in[pix+tap][c], db[n] += sum dout.
 * Split over pixel ranges into slabs in `workspace`, then reduced into OIHW gradients (+=).
 * sininn_wgrad_workspace_bytes gives the slab size for a shape.
 * ---------------------------------------------------------------------------------------------- */
size_t sininn_wgrad_workspace_bytes(int N, int Cin, int ksize, int B, int H, int W);
int sininn_wgrad(const float* in, int in_stride, int Cin, const float* dout, int dout_stride, int N,
                 int B, int H, int W, int ksize, float* gw_oihw, float* gbias,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Grouped form: the weight gradients of up to 8 convs that see the same pixels (B,H,W) and kernel size -- the four
 * convs of one GLOW block -- in two launches (gradient kernel + ordered slab reduce).  The convs share the launch
 * grid, so each needs far fewer split-K slabs than on its own (3-6x less slab traffic); results are bitwise
 * reproducible like sininn_wgrad's.  3x3: Winograd F(3x3,2x2) kernel, 64 x 32 output tiles; 1x1: 32 x 32 tiles. */
typedef struct sininn_wgrad_item {
  size_t struct_bytes;                             /* ABI v4: must be sizeof(sininn_wgrad_item).  The descriptor has grown
                                                      optional fields twice; a caller built against another revision, or one
                                                      that fills a stack item field by field and misses a new field, is
                                                      refused instead of launching with garbage ("the round-2 abort") */
  const float* in;   int in_stride;   int Cin;     /* conv input  [M][in_stride], Cin % 4 == 0                      */
  const float* dout; int dout_stride; int N;       /* output gradient [M][dout_stride], N % 4 == 0                  */
  float* gw; float* gb;                            /* OIHW weight gradient (+=), bias gradient (+=, may be NULL)    */
  int in_bf16, dout_bf16;                          /* mixed-precision path: the operand is stored as bf16 (pointer cast,
                                                      stride in elements); the gradient accumulates in fp32          */
  int in_group_stride, dout_group_stride;          /* > 0: the operand is channel-group-major [C/8][B*H*W][8] (fp32, 3x3
                                                      Winograd kernels); value = floats between channel groups         */
  int gap_begin, gap_len;                          /* gap_len > 0: input channels [gap_begin, gap_begin + gap_len) are padding
                                                      that the weight does not have (gw rows hold Cin - gap_len channels)  */
} sininn_wgrad_item;
size_t sininn_wgrad_group_workspace_bytes(const sininn_wgrad_item* items, int n, int B, int H, int W, int ksize);
int sininn_wgrad_group(const sininn_wgrad_item* items, int n, int B, int H, int W, int ksize,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the coupling tail (the elementwise part of GLOWCouplingBlock).
 *   inverse==0: y = e(s) v + t      dv = dy e ; dt = dy  ; ds = (dy v e + gld) L'(s)
 *   inverse==1: y = (v - t)/e(s)    dv = dy/e ; dt = -dy/e ; ds = -(dy y + gld) L'(s)
 * dy[m][c] is read from dy[m*dy_stride + (dy_map ? dy_map[c] : c)] ; `vy` is v (inverse==0) or y
 * (inverse==1) read through vy_map likewise.  dr is [M][2*Co] = (ds | dt).  gld is the optional
 * per-sample gradient of the block's log-det ([B], may be NULL).
 * ---------------------------------------------------------------------------------------------- */
int sininn_coupling_bwd(const float* dy, int dy_stride, const int* dy_map,
                        const float* vy, int vy_stride, const int* vy_map,
                        const float* s, const float* gld, int B, int HW, int Co, float clamp,
                        int inverse, float* dr, float* dv, int dv_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * IRN elementwise pieces (archs.py:135-199).
 * haar: HaarDownsampling.forward / rev (archs.py:183-199): 2x2 Haar analysis (/4) with the band-major channel
 *   regrouping out[:, k*C + c] = band k of channel c, or the synthesis (conv_transpose2d, no /4).  Element strides.
 * lrelu_bwd: g[m][j] *= (f[m][j] > 0 ? 1 : slope)   (gradient through LeakyReLU, in place on a channel slot).
 * irn_coupling_bwd: backward of y = v*exp(s)+G (inverse==0) or y = (v-G)/exp(s) (inverse==1), s = clamp*(2*sigmoid(h)-1):
 *   dG, dh [M][Co] compact, dv [M][Co] at dv_stride.  vy = v (inverse==0) or y (inverse==1).
 * ---------------------------------------------------------------------------------------------- */
int sininn_haar(const float* in, const int64_t in_strides[4], float* out, const int64_t out_strides[4],
                int B, int C, int H, int W, int inverse, void* stream);
int sininn_lrelu_bwd(float* g, int g_stride, const float* f, int f_stride, int64_t M, int n, float slope, void* stream);
/* irn_tail: the InvBlockExp tail on its own (archs.py:152-156): out = v * exp(s) + g (inverse == 0) or (v - g) / exp(s)
 *   (inverse == 1), s = clamp * (2 sigmoid(h) - 1); h, g [M][Co] compact, v / out at their pixel strides.  Its backward is
 *   sininn_irn_coupling_bwd.  Lets the H and G DenseBlocks of a block run on two streams (ABI v4). */
int sininn_irn_tail(const float* v, int v_stride, const float* h, const float* g, int64_t M, int Co, float clamp, int inverse,
                    float* out, int out_stride, void* stream);
int sininn_irn_coupling_bwd(const float* dy, int dy_stride, const float* vy, int vy_stride, const float* hval,
                            int64_t M, int Co, float clamp, int inverse, float* dG, float* dh, float* dv,
                            int dv_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One DenseBlock of the IRN architecture per call (archs.py:74-133, with the InvBlockExp tail of archs.py:135-160 as the
 * epilogue of its fifth conv): host-side launch sequence, like sininn_glow_forward / _backward for the SRF path.  The five
 * dense-connected 3x3 convs write their 32-channel outputs into slots of ONE feature buffer buf [M][cinp + 128]
 * (cinp = cin rounded up to 8; the torch.cat chain costs nothing); weights are packed for that padded channel order.
 *   mode 0: out = conv5(...)                       1: out = aux1 + conv5(...)          (y1 = x1 + F(x2))
 *   mode 2: out = aux1 * exp(s) + conv5(...)       3: out = (aux1 - conv5(...)) / exp(s),   s = clamp * (2 sigmoid(aux2) - 1)
 * backward: dF [M][cinp + 128] (on return its first cin channels are d loss / d x), dv / dh (modes 2, 3: gradients w.r.t.
 * aux1 and aux2; mode 1: the gradient w.r.t. aux1 is dout itself), OIHW weight / bias gradients (+=) of the UNPADDED convs.
 * The five weight gradients run as one grouped launch pair on wgrad_stream.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sininn_dense_args {
  size_t struct_bytes;                             /* ABI v4: must be sizeof(sininn_dense_args)                            */
  int B, H, W, cin, cout, mode, winograd;
  float clamp;
  const float* x; int x_stride;
  const float* aux1; int aux1_stride;
  const float* aux2;                               /* [M][cout] */
  float* buf; float* out;                          /* [M][cinp + 128], [M][cout] */
  const float* w_fwd[5]; const float* b_fwd[5]; const float* w_dgrad[5];
  /* backward only */
  const float* dout;                               /* [M][cout] */
  float* dF;                                       /* [M][cinp + 128] */
  float* dD;                                       /* [M][cout rounded up to 8] scratch (modes 2, 3 and cout % 8 != 0)   */
  float* dh; float* dv;                            /* modes 2, 3: [M][cout] each                                          */
  float* gw[5]; float* gb[5];
  void* workspace; size_t workspace_bytes;         /* sininn_dense_workspace_bytes                                        */
  /* ABI v4: extents (in floats) of every buffer the executor writes or reads at a size it derives itself; a call whose
   * buffers are smaller than the launch sequence needs is refused (sininn_last_error) before anything is launched.
   * M = B*H*W, bw = pad8(cin) + 128.  Required: buf >= M*bw, out >= M*cout; backward: dout >= M*cout, dF >= M*bw,
   * dD >= M*pad8(cout) when used, dh / dv >= M*cout (modes 2, 3), aux2 >= M*cout (modes 2, 3).                         */
  size_t buf_floats, out_floats, aux2_floats, dout_floats, dF_floats, dD_floats, dh_floats, dv_floats;
} sininn_dense_args;
size_t sininn_dense_workspace_bytes(int B, int H, int W, int cin, int cout);
int sininn_dense_forward(const sininn_dense_args* args, void* stream);
int sininn_dense_backward(const sininn_dense_args* args, void* stream, void* wgrad_stream);

/* Mixed-precision DenseBlock (the IRN path's --precision bf16): the same launch sequence on the bf16 matrix pipe.
 * Precision contract: the conv subnets compute in bf16 with fp32 accumulation, the invertible flow stays fp32.
 *   - stored as bf16 (round to nearest even, once): the feature buffer buf [M][cinp + 128] -- the block input x (pad channels
 *     [cin, cinp) zero) and conv1-4's outputs after bias + LeakyReLU(0.2) in fp32 -- and the five weight packs;
 *   - fp32: biases, accumulators, every epilogue, conv5's output with its InvBlockExp tail, dF / dD / dh / dv and the
 *     parameter gradients.  dD and each finished 32-channel slot of dF are rounded to bf16 while a data-gradient or
 *     weight-gradient kernel stages them; dF accumulates in fp32.  The LeakyReLU-backward gate is the stored bf16 feature.
 * Packs (sininn_pack_batch_bf16 / sininn_pack_conv_weights_bf16 layouts) for conv i = 0..4 in the padded channel order:
 *   w_fwd[i]   [9][Np_i][Kp_i] bf16, Np_i = 32 (i < 4) or pad16(pad8(cout)), Kp_i = pad16(cinp + 32 i)
 *   b_fwd[i]   [Np_i] fp32
 *   w_dgrad[i] [9][pad16(cinp + 32 i)][Kd_i] bf16, Kd_i = 32 (i < 4) or pad16(pad8(cout))
 * Every extent is checked (struct_bytes, element counts, dtype flags) before anything is launched. */
typedef struct sininn_dense_bf16_args {
  size_t struct_bytes;                             /* must be sizeof(sininn_dense_bf16_args)                               */
  int buf_bf16, w_bf16;                            /* dtype flags: must both be 1 (buf and the packs hold bf16)            */
  int B, H, W, cin, cout, mode;                    /* modes 0-3 as in sininn_dense_args                                     */
  float clamp;
  const float* x; int x_stride;
  const float* aux1; int aux1_stride;
  const float* aux2;                               /* [M][cout] */
  void* buf; float* out;                           /* bf16 [M][cinp + 128], fp32 [M][cout] */
  const void* w_fwd[5]; const float* b_fwd[5]; const void* w_dgrad[5];
  /* backward only */
  const float* dout; float* dF; float* dD; float* dh; float* dv;   /* fp32, shapes as sininn_dense_args                 */
  float* gw[5]; float* gb[5];
  void* workspace; size_t workspace_bytes;         /* sininn_dense_bf16_workspace_bytes                                   */
  /* extents in ELEMENTS of each buffer's own type */
  size_t buf_elems, out_floats, aux2_floats, dout_floats, dF_floats, dD_floats, dh_floats, dv_floats;
  size_t w_fwd_elems[5], b_fwd_floats[5], w_dgrad_elems[5];
} sininn_dense_bf16_args;
size_t sininn_dense_bf16_workspace_bytes(int B, int H, int W, int cin, int cout);
int sininn_dense_forward_bf16(const sininn_dense_bf16_args* args, void* stream);
int sininn_dense_backward_bf16(const sininn_dense_bf16_args* args, void* stream, void* wgrad_stream);

/* ------------------------------------------------------------------------------------------------
 * One GLOW coupling block per call (FrEIA GLOWCouplingBlock.forward / its autograd, SURVEY Appendix A;
 * wired at archs.py:61-64): host-side launch sequence of the kernels above.
 *   forward : (rev==0)  r2=s2(x2); y1=e(s2)*x1+t2; r1=s1(y1); y2=e(s1)*x2+t1      logdet += sum log_e
 *             (rev==1)  r1=s1(x1); y2=(x2-t1)/e(s1); r2=s2(y2); y1=(x1-t2)/e(s2)  logdet -= sum log_e
 *             out channel c is stored at dst_map[c] (folds the following / preceding PermuteRandom).
 *   backward: dx, and (+=) the OIHW weight / bias gradients of the four convs; weight-gradient kernels are
 *             queued on wgrad_stream (ordered after their inputs with events), everything else on stream.
 * `saved` (sininn_glow_saved_floats floats) is written by forward and read by backward: hidden activations of
 * both subnets, both s tensors, the first half's compact output.  `scratch` is backward-only.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sininn_subnet {
  const float* w1; const float* b1;      /* conv1 packed [taps][256][Cin] + bias[256]                          */
  const float* w2; const float* b2;      /* conv2 packed [taps][2*Co][256] (s|t interleaved), bias packed alike */
  const float* w1_dgrad;                 /* [taps][pad16(Cin)][256]  (backward only)                           */
  const float* w2_dgrad;                 /* [taps][256][2*Co]        (backward only)                           */
  float* gw1; float* gb1; float* gw2; float* gb2;   /* OIHW gradient accumulators (NULL: skip)                 */
  int winograd;                          /* bit 0: w1, bit 1: w2, bit 2: w1_dgrad (rows padded to 32), bit 3: w2_dgrad
                                            hold Winograd packs (sininn_pack_winograd) instead of tap-major packs   */
} sininn_subnet;

typedef struct sininn_glow_args {
  int B, H, W, C, ksize, rev; float clamp;
  const float* x; float* out; const int* dst_map; float* logdet;
  sininn_subnet s1, s2;
  float* saved;
  void* scratch; size_t scratch_bytes;
  const float* dout; const float* gld; float* dx;
  int skip_dx;                           /* backward: the caller does not need dx (first block of a pass): the last data-
                                            gradient conv is skipped; dx must still be a valid buffer (partly written) */
  int dtype;                             /* 0: fp32 subnets (f32 MFMA, Winograd for 3x3).  1: mixed precision -- the conv
                                            subnets run on bf16 MFMA with fp32 accumulation (packs from
                                            sininn_pack_conv_weights_bf16, hidden tensors stored as bf16), the flow tensors,
                                            the coupling arithmetic, log-det and all gradients w.r.t. parameters stay fp32 */
  int no_save;                           /* forward: nothing will be differentiated (torch.no_grad passes: validation /
                                            inference, lit_wrapper.py:79-128) -- the saved s and, where the subnet runs as one
                                            launch (1x1: sininn_conv_pair_k1; 3x3 with dtype 1: sininn_conv_sub3), the hidden
                                            tensor are not written to HBM                                                  */
} sininn_glow_args;

/* Live timing for bench.py: between begin and end, every forward 3x3 coupling conv (conv2 + affine epilogue) of the
 * level whose image height is `level_height` is (a) bracketed by HIP events on its launch stream and (b), when `stamps`
 * (device, 2 words per launch, initialised to {~0ull >> 1, 0}) is given, stamped from inside the kernel (see
 * sininn_conv_args.stamp; launch i uses words 2i, 2i+1, launches beyond max_launches are not stamped).  With several
 * streams in flight the event bracket also contains the time the launch waits for the GPU behind other streams'
 * kernels; the stamps are the kernel's own execution window (what a kernel trace reports).  end() synchronises on the
 * events and returns the number of launches timed and their summed event duration. */
void sininn_profile_begin(int level_height, unsigned long long* stamps, int max_launches);
int sininn_profile_end(int* count, float* total_ms);
int sininn_wall_clock_khz(void);   /* tick rate of the stamps */

/* Per-class timing of the block executor for bench.py's roofline.classes: between begin and end every launch of
 * sininn_glow_forward / _backward is bracketed by HIP events on its stream.  Classes (index = class + 6 * (ksize == 1)):
 * 0 conv1 forward (+ReLU), 1 conv2 forward + coupling + log-det, 2 data gradient of conv2 (+ReLU mask), 3 data gradient of
 * conv1 (+ skip gradient, + fused coupling backward), 4 weight gradients (+ slab reduce), 5 coupling backward tail.
 * end() synchronises and fills, per class, the summed event time (ms), the summed ALGORITHMIC FLOPs (2 M k^2 Cin N) and
 * the launch count (n = 12 entries).  The bracket is the kernel's own duration only when everything runs on one stream. */
#define SININN_PROFILE_CLASSES 12
void sininn_profile_classes_begin(void);
int sininn_profile_classes_end(int n, double* ms, double* flops, int* launches);
/* algorithmic HBM bytes per class, summed over the launches of the last sininn_profile_classes_end (the fused 1x1 launches report
 * them: x / dr / side inputs / outputs / slabs; 0 for a class whose launches do not) */
int sininn_profile_classes_bytes(int n, double* bytes);

size_t sininn_glow_saved_floats(int B, int H, int W, int C);
size_t sininn_glow_saved_floats_dtype(int B, int H, int W, int C, int dtype);   /* dtype 1: bf16 hidden tensors (half the floats) */
size_t sininn_glow_scratch_bytes(int B, int H, int W, int C, int ksize);                       /* dtype 0 */
size_t sininn_glow_scratch_bytes_dtype(int B, int H, int W, int C, int ksize, int dtype);   /* dtype 1 needs no slabs for the fused 1x1 backward */
int sininn_glow_forward(const sininn_glow_args* args, void* stream);
int sininn_glow_backward(const sininn_glow_args* args, void* stream, void* wgrad_stream);
/* Parity tooling (ABI v4): the ReLU gates the forward pass of a block took, gates[m][j] = (hidden[m][j] > 0) as bytes
 * [B*H*W][256], for the subnet executed first (which = 0: s2 when rev == 0, s1 when rev == 1) or second (which = 1), decoded
 * from `saved` in whatever layout / dtype the executor stored it.  args: the descriptor of the forward call (B, H, W, C, ksize,
 * rev, dtype, s1 / s2 .winograd, saved).  With these gates forced, a float64 evaluation of the network is a smooth function
 * and can be compared with the HIP path without the discrete noise of units that sit within rounding distance of 0. */
int sininn_glow_hidden_gates(const sininn_glow_args* args, int which, uint8_t* gates, void* stream);
/* 1 when the block executor may keep the 256-channel hidden tensors of a fp32 3x3 subnet channel-group-major ([256/8][M][8]) at
 * this shape, 0 when it takes the row-major layout because the 32-bit staging offsets of the kernels reading the tensor could not
 * address it (the same bound sininn_conv / sininn_wgrad_group check and refuse).  Host-only; no launch. */
int sininn_glow_group_major_fits(int B, int H, int W);

/* ------------------------------------------------------------------------------------------------
 * Index maps: FrEIA IRevNetDownsampling (archs.py:28-31,35-38) and PermuteRandom (archs.py:65-68),
 * plus NCHW<->NHWC import/export, as ONE strided gather:
 *   levels==0 : out[b,y,x,cm(c)] = in[b,c,y,x]
 *   squeeze (inverse==0), per level: out[b,(hb*2+wb)*C+c,i,j] = in[b,c,2i+hb,2j+wb]
 *   unsqueeze (inverse==1) is the exact inverse.
 * `levels` squeezes are composed in one pass.  Tensors are described by element strides
 * (sb, sc, sh, sw) so either side may be NCHW or NHWC.  chan_map (device, may be NULL) is applied on
 * the C-channel side that is being WRITTEN when map_on_out!=0, else on the side being READ.
 * B,C,H,W describe the un-squeezed (fine) tensor.
 * ---------------------------------------------------------------------------------------------- */
int sininn_squeeze(const float* in, const int64_t in_strides[4], float* out, const int64_t out_strides[4],
                   int B, int C, int H, int W, int levels, int inverse,
                   const int* chan_map, int map_on_out, void* stream);

/* The same index maps between two DENSE pixel-major tensors (fine [B][H][W][C], coarse [B][H/2^l][W/2^l][C*4^l]), in
 * gather form: four consecutive output floats per thread, 16-byte stores.  fine_map (device, may be NULL) acts on the
 * fine tensor's channel index:  forward  coarse[.., q*C + c] = fine[.., fine_map[c]];
 *                               inverse  fine[.., c] = coarse[.., q*C + fine_map[c]].
 * levels == 0: out[.., c] = in[.., fine_map[c]].  Needs B*C*H*W % 4 == 0 and (C*4^levels) % 4 == 0. */
int sininn_squeeze_rows(const float* in, float* out, int B, int C, int H, int W, int levels, int inverse,
                        const int* fine_map, void* stream);

/* out[m][j] = in[m][idx[j]] on pixel-major tensors (PermuteRandom.forward: x[:, perm]). */
int sininn_permute_channels(const float* in, int in_stride, float* out, int out_stride,
                            int64_t M, int C, const int* idx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Losses (loss.py).  Strided 4-D views (element strides sb,sc,sh,sw); sums are written to fp32
 * device scalars, the caller divides (torch.mean) -- keeps the kernels stream-async.
 * ---------------------------------------------------------------------------------------------- */
/* sum (x-y)^2 -> out[0]  (loss.py:3-5).  y may be NULL => sum x^2 (loss.py:38-39).  out must be zeroed. */
int sininn_sqdiff_sum(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4],
                      int B, int C, int H, int W, float* out, void* stream);
/* gx = scale[0]*gscale * (x-y) (and gy = -gx when gy!=NULL); `scale` is a device scalar (upstream grad). */
int sininn_sqdiff_bwd(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4],
                      int B, int C, int H, int W, const float* scale, float gscale,
                      float* gx, const int64_t gxs[4], float* gy, const int64_t gys[4], void* stream);
/* Gram matrices for loss.mmd (loss.py:15-18): g[0]=x x^T, g[1]=y y^T, g[2]=x y^T, each [B][B].  g holds
 * (1 + SININN_MMD_SLOTS) * 3*B*B floats ZEROED by the caller: the result followed by the partial-sum slots. */
#define SININN_MMD_SLOTS 16
int sininn_mmd_gram(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4],
                    int B, int C, int H, int W, float* g, void* stream);
/* loss.py:20-36 on the three Grams (the result block of g) -> out[0] (mean) and, when coef is not NULL, coef[4][B][B]:
 * the matrices AX, BX, AY, BY (in this order, each [B][B] row-major) with dLoss/dx = AX x + BX y, dLoss/dy = AY x + BY y
 * (rows = samples; the chain rule through the distances and the clamp is folded in). */
int sininn_mmd_finish(const float* g, int B, int rev, float* out, float* coef, void* stream);
/* coef = the 4*B*B floats sininn_mmd_finish wrote:  gx[i,:] = scale[0] * sum_j ( AX[i][j] x[j,:] + BX[i][j] y[j,:] ),
 * gy[i,:] = scale[0] * sum_j ( AY[i][j] x[j,:] + BY[i][j] y[j,:] ).  gx or gy may be NULL (not both). */
int sininn_mmd_bwd(const float* x, const int64_t xs[4], const float* y, const int64_t ys[4],
                   int B, int C, int H, int W, const float* coef, const float* scale,
                   float* gx, const int64_t gxs[4], float* gy, const int64_t gys[4], void* stream);

/* ------------------------------------------------------------------------------------------------
 * Warps.
 * affine_warp: F.affine_grid(theta, align_corners=False) + F.grid_sample(bilinear, zeros,
 *   align_corners=False) fused -- what kornia.warp_affine evaluates for tcr.py:43 once theta (the
 *   inverted, normalised 2x3 matrix, [B][2][3]) is known.  Optional fused MSE against `ref`
 *   (sum (warp-ref)^2 -> sse[0]).  bwd is the image gradient (atomic scatter).
 * flow_warp_l1: Resample2d.forward + the photometric metric
 *   (video-interpolation/my_utils/resample2d.py:57-72, video-interpolation/trainer.py:61-62):
 *   warped = grid_sample(img, (coords+flow)/(W-1,H-1)*2-1) ; metric = mean_c |target - warped|.
 * ---------------------------------------------------------------------------------------------- */
int sininn_affine_warp(const float* img, const int64_t is[4], const float* theta, int B, int C, int H, int W,
                       float* out, const int64_t os[4], const float* ref, const int64_t rs[4], float* sse,
                       void* stream);
int sininn_affine_warp_bwd(const float* gout, const int64_t gs[4], const float* theta, int B, int C, int H, int W,
                           float* gimg, const int64_t gis[4], void* stream);
int sininn_flow_warp_l1(const float* img, const float* flow, const float* target, int B, int C, int H, int W,
                        float* warped, float* metric, void* stream);
int sininn_flow_warp_l1_bwd(const float* img, const float* flow, const float* target, const float* warped,
                            const float* gwarped, const float* gmetric, int B, int C, int H, int W,
                            float* gimg, float* gflow, void* stream);
/* The same two kernels in the arithmetic BASELINE configs[3] names ("pair_flow warp + INN at 512x512, bf16"): img, target,
 * warped and gwarped are bf16 in HBM (half the bytes of this HBM-bound pair); the bilinear weights, the interpolation, the
 * metric (taken on the ROUNDED warped value, i.e. on what the consumer reads back) and every gradient accumulator
 * (gimg, gflow) are fp32, flow and metric are fp32 tensors (ABI v4). */
int sininn_flow_warp_l1_bf16(const void* img, const float* flow, const void* target, int B, int C, int H, int W,
                             void* warped, float* metric, void* stream);
int sininn_flow_warp_l1_bwd_bf16(const void* img, const float* flow, const void* target, const void* warped,
                                 const void* gwarped, const float* gmetric, int B, int C, int H, int W,
                                 float* gimg, float* gflow, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Frame-window sampler (data.py:31-45 + 112-115 on an HBM-resident uint8 clip):
 *   hr[n] = hr_clip[idx[n]] / 255 as (3,H,W) planar or pixel-major, lr[n] = concat of the 2*win+1 LR
 *   frames idx[n]-win..idx[n]+win on the channel axis / 255.
 * hr_clip (T,H,W,3) u8, lr_clip (T,h,w,4) u8, idx device int32 [n].
 * ---------------------------------------------------------------------------------------------- */
int sininn_sample_windows(const uint8_t* hr_clip, const uint8_t* lr_clip, const int* idx, int n,
                          int T, int H, int W, int h, int w, int win,
                          float* hr_out, const int64_t hs[4], float* lr_out, const int64_t ls[4], void* stream);

/* Frame-pair sampler of the flow path (video-interpolation/trainer.py:49-62 consumes (frame1, frame2) of one clip as planar
 * (B,3,H,W) tensors): out0[s] = clip[idx[s]] / 255, out1[s] = clip[idx[s] + gap] / 255 (frame index clamped to the clip), planar,
 * fp32 (bf16 == 0) or bf16 (the arithmetic of BASELINE configs[3]).  clip (T,H,W,3) u8, H*W % 4 == 0.  ABI v4. */
int sininn_sample_pairs(const uint8_t* hr_clip, const int* idx, int n, int T, int H, int W, int gap,
                        void* out0, void* out1, int bf16, void* stream);

/* ------------------------------------------------------------------------------------------------
 * On-device LR synthesis (datasets/prepare.py:35-82,147-165): RGGB sampling + scale x scale binning per Bayer plane
 * with the reference's float64 arithmetic and uint8 truncation.  hr (T,H,W,3) u8 -> lr (T,H/(2s),W/(2s),4) u8.
 * ---------------------------------------------------------------------------------------------- */
int sininn_bayer_bin(const uint8_t* hr, uint8_t* lr, int T, int H, int W, int scale, int reduce_sum, void* stream);
/* Demosaiced LR preview (datasets/prepare.py:103-119,158,163-165): the unquantised binned planes re-packed as an RGGB
 * mosaic and bilinearly demosaiced (colour_demosaicing 0.1.6, scipy 'reflect' boundary), clipped, quantised:
 * rgb [T][H/scale][W/scale][3] uint8. */
int sininn_bayer_demosaic(const uint8_t* hr, uint8_t* rgb, int T, int H, int W, int scale, int reduce_sum, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Output pixels of the inference path (SingleVideoINN.infer, lit_wrapper.py:91-128): float frames `in` (logical
 * (B,C,H,W), element strides) -> uint8 images out[B][H][W][C] on the device, so only bytes cross PCIe.
 *   wrap == 0: clamp(x,0,1)*255 truncated;  wrap != 0: (uint8)(int)(x*255) = torchvision ToPILImage's
 *   pic.mul(255).byte() with its wrap-around on out-of-range values (what the reference does, lit_wrapper.py:94,120).
 * ---------------------------------------------------------------------------------------------- */
int sininn_frames_to_u8(const float* in, const int64_t in_strides[4], uint8_t* out, int B, int C, int H, int W, int wrap,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * Adam exactly as torch.optim.Adam (lit_wrapper.py:131-138: L2 weight decay, not AdamW):
 *   g = grad*grad_scale + wd*p ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ;
 *   p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * ---------------------------------------------------------------------------------------------- */
int sininn_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Photometric-loss operators of the flow trainer.  NCHW contiguous fp32.
 *   softsplat      video-interpolation/my_utils/softsplat.py:8-177: out (ZEROED by the caller) += forward splat of `in`
 *                  along `flow`; _bwd returns d/d in and / or d/d flow (either may be NULL) for an upstream gout.
 *   occlusion_wang video-interpolation/my_utils/occlusions.py:29-104: corr (ZEROED, [B][H][W]) = range map of flow21,
 *                  mask (optional, [B][1][H][W]) = 1 - (corr <= thresh).
 *   census         video-interpolation/my_utils/loss.py:30-72 (CensusLoss.forward(im1, im2, mask)), 3-channel images,
 *                  mask [B][mask_channels][H][W] with 1 (pair_flow.py) or 3 (trainer.py:64) channels, max_distance 1..4.  acc (ZEROED, SININN_CENSUS_ACC_FLOATS floats: two sums + 64
 *                  partial slots) receives {sum of distances, sum(mask)} in its first two words
 *                  and is the saved state for _bwd; out[0] = the loss.  _bwd: g1 / g2 = gscale[0] * d loss / d im1 / im2
 *                  (no gradient w.r.t. the mask, which the trainer builds from comparisons).
 * ---------------------------------------------------------------------------------------------- */
int sininn_softsplat(const float* in, const float* flow, int B, int C, int H, int W, float* out, void* stream);
int sininn_softsplat_bwd(const float* in, const float* flow, const float* gout, int B, int C, int H, int W,
                         float* gin, float* gflow, void* stream);
int sininn_occlusion_wang(const float* flow21, int B, int H, int W, float thresh, float* corr, float* mask, void* stream);
#define SININN_CENSUS_ACC_FLOATS 130
/* occlusion_brox (occlusions.py:111-118): mask [B][1][H][W] bytes (1 = inconsistent) from the forward flow and the backward
 * flow already warped by it (sininn_flow_warp_l1(bw, fw)). */
int sininn_occlusion_brox(const float* fw, const float* warped_bw, int B, int H, int W, uint8_t* mask, void* stream);
int sininn_census(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int H, int W,
                  int max_distance, float weight, float* acc, float* out, void* stream);
int sininn_census_bwd(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int H, int W,
                      int max_distance, float weight, const float* acc, const float* gscale, float* g1, float* g2,
                      void* stream);
/* L1Loss (loss.py:17-27): l1_loss(im1*mask, im2*mask) / sum(mask) * numel(mask) * weight; mask channels 1 or C; acc as for
 * the census loss (ZEROED, SININN_CENSUS_ACC_FLOATS).  _bwd: g1 = -g2 = gscale[0] * d loss / d im1. */
int sininn_masked_l1(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int C, int H, int W,
                     float weight, float* acc, float* out, void* stream);
int sininn_masked_l1_bwd(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int C, int H,
                         int W, float weight, const float* acc, const float* gscale, float* g1, float* g2, void* stream);
/* SSIMLoss (loss.py:75-103): (2 md + 1)^2 unpadded average pooling, md 1..2; acc / gradients as for sininn_masked_l1. */
int sininn_ssim(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int C, int H, int W, int md,
                float weight, float* acc, float* out, void* stream);
int sininn_ssim_bwd(const float* im1, const float* im2, const float* mask, int mask_channels, int B, int C, int H, int W,
                    int md, float weight, const float* acc, const float* gscale, float* g1, float* g2, void* stream);
/* BilateralSmooth (loss.py:106-132): edge-aware smoothness of flow [B][2][H][W] guided by img [B][C][H][W];
 * order 1 | 2, gauss != 0: squared ('gauss') else absolute ('exp') image differences scaled by edge_constant.
 * acc (ZEROED, SININN_CENSUS_ACC_FLOATS) is scratch.  _bwd: gflow = gscale[0] * d loss / d flow (img gets none). */
int sininn_bilateral_smooth(const float* img, const float* flow, int B, int C, int H, int W, int order, int gauss,
                            float edge_constant, float weight, float* acc, float* out, void* stream);
int sininn_bilateral_smooth_bwd(const float* img, const float* flow, int B, int C, int H, int W, int order, int gauss,
                                float edge_constant, float weight, const float* gscale, float* gflow, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The flow-field network of the flow trainer: coordinate MLP, forward and backward (csrc/flownet.hip).
 *   video-interpolation/model.py:490-505 RbfModel (RadialBasisEncoding, model.py:343-366: exp(-sigma_k^2 |x - c_k|^2)),
 *   model.py:418-433 FFModel / model.py:454-469 UFFModel (FourierFeatures.forward, model.py:230-238: x * 2 pi, x @ frequencies,
 *   sin / cos interleaved), MLP model.py:31-43, all with the ModelParams defaults (model.py:18-28): 3 -> 512 -> 256 -> 256 -> 256 -> 4.
 *   forward = FlowTrainer.forward (video-interpolation/trainer.py:37-45): poses = meshgrid(times, linspace(-1,1,H),
 *   linspace(-1,1,W)); flows[t][c][y][x] = net(poses)[p][c] * scale, flow12 = flows[:, :2], flow21 = flows[:, 2:].
 * The axis vectors are DEVICE arrays computed by the caller (torch.linspace: bit-identical coordinates); neither the poses nor
 * the N x 512 encoding are ever stored.  Weights are nn.Linear's own [out][in] layout: there is no packing step.
 *   forward : writes flows; if saved != NULL (training) also the three post-ReLU hidden layers, [3][Npad][256], Npad = N rounded
 *             up to 64 (sininn_flownet_saved_bytes(N)); every row is written on every call.
 *   backward: dflows [T][4][H][W] -> gw[0..3] / gb[0..3] (OVERWRITTEN, nn.Linear layout, scale folded in).  Needs the saved
 *             buffer of the forward call on the same weights and a workspace of sininn_flownet_workspace_bytes(N) bytes (the three
 *             hidden gradients, two transposed weights, per-block partial sums); sums over points are added in a fixed order
 *             (no floating-point atomics): two calls on the same inputs are bitwise equal.  The ReLU gates the forward took are
 *             saved > 0.
 * Progressive networks (model.py:526-625 PRBFModel / PFFModel / PUFFModel under the per-feature mask of a controller,
 *   progressive_controller.py:14-158): progressive = 1, enc_dim = 515, w[0] is [256][515]; the input of layer 1 is
 *   cat((t, y, x), enc) * mask with mask a DEVICE vector of 515 floats (feature order t, y, x, e0 .. e511).  k_active, from the host, is a
 *   number of leading features after which every mask entry is zero (515 is always valid): layer 1 and its weight gradient skip the
 *   features beyond it, which is exact, so any valid k_active gives bitwise the same flows and gradients.  gw[0] is [256][515],
 *   column k = mask[k] * sum_p dh1[p][j] feature_k[p], an exact 0 where mask[k] is 0.  The forward call folds the mask into a packed
 *   copy of w[0] and needs a workspace of sininn_flownet_forward_workspace_bytes(args) bytes for it (0 if not progressive); the
 *   backward call needs no more than sininn_flownet_workspace_bytes(N), and `saved` has the same size.
 * Learnable frequencies (model.py:263-307 RotatedFourierFeatures, RFFModel model.py:436-451, PRFFModel model.py:586-590): the caller passes
 *   F_eff = normalize(frequencies, dim 0) * magnitudes as enc_a (768 values, computed with its own ops) and the forward call is the
 *   Fourier one.  The ENCGRAD mode of sininn_flownet_backward does everything the call without it does (the eight gradients are bitwise the same)
 *   and also writes g_enc_a [3][256] (OVERWRITTEN), the gradient with respect to the matrix passed as enc_a:
 *     dE[p][k] = sum_j dh1[p][j] w[0][j][k] (progressive: w[0][j][3 + k] * mask[3 + k]), never stored;
 *     dphi[p][f] = dE[p][2 f] cos(phi[p][f]) - dE[p][2 f + 1] sin(phi[p][f]), sin / cos as the forward pass computed them;
 *     g_enc_a[d][f] = 2 pi sum_p coordinate_d[p] dphi[p][f], per-block partial sums added in index order (no floating-point atomics: two
 *     calls are bitwise equal); progressive: an exact +0 for a frequency whose sin and cos features are both closed, and any valid
 *     k_active gives bitwise the same g_enc_a.
 *   It needs a second workspace of sininn_flownet_encgrad_workspace_bytes(args) bytes (a transposed copy of w[0] and the partial sums; 0
 *   if the encoding is not Fourier), 16-byte aligned, and refuses encoding != SININN_FLOWNET_FOURIER, a null g_enc_a and a short
 *   enc_workspace before any launch.
 * Radial-basis grid (model.py:369-415 UniformRadialBasisGridEncoding, RbfgModel model.py:508-523, PRBFGModel model.py:614-618): encoding
 *   SININN_FLOWNET_RBFG, 256 frequencies j with buffers offsets [256][3] (enc_a) and sigma [256] (enc_b), all fp32, p = 2 / sigma_j:
 *     xa_d = x_d + offsets[j][d], xb_d = xa_d + 1 / sigma_j;  u_d = (v_d mod p) * 2 - p  (v = xa or xb, the remainder in [0, p));
 *     e(v) = 2 exp(-(sum_d u_d^2) sigma_j^2) - 1;  feature 2 j = e(xa), feature 2 j + 1 = e(xb).
 *   The buffers are constants: the backward call is sininn_flownet_backward, progressive networks work as above.
 * Positional encoding (model.py:321-340 PositionalEncoding, PEModel model.py:472-487, PPEModel model.py:607-611): encoding
 *   SININN_FLOWNET_PE, enc_a = freqs [4] (2^i pi in fp32), enc_b unused, enc_dim = 24 (progressive: 27), w[0] is [256][24] ([256][27]):
 *     feature 6 f + d = cos(freqs[f] * x_d), feature 6 f + 3 + d = sin(freqs[f] * x_d), f = 0 .. 3, d = 0 .. 2 (t, y, x); the argument is
 *     one fp32 product, sine and cosine the accurate full-range fp32 functions.
 *   The reference's forward reshapes through view(-1, 21) and raises unless N is a multiple of 7; where it runs it is this formula, which
 *   the library evaluates for every N.  Plain PE reads w[0] in place (96-byte rows) and sininn_flownet_forward_workspace_bytes is 0 for it;
 *   the progressive forward packs mask * w[0] into [256][32] + [256][4] (36864 bytes).  mask has 27 entries, k_active is 0 .. 27; gw[0]
 *   is [256][24] / [256][27], progressive: an exact +0 where mask[k] is 0 and in an encoded column k >= 3 with k >= k_active; the three
 *   coordinate columns k < 3 are governed by the mask alone, whatever k_active is (as in the 515-wide networks).  The order of every sum is
 *   independent of k_active; the backward call is sininn_flownet_backward, workspace and `saved` have the sizes above.
 * Piecewise-linear encoding (model.py:628-678 PieceWiseEncoding, MPFFModel model.py:600-604): encoding SININN_FLOWNET_PIECEWISE, enc_a =
 *   frequencies [3][256] (the layout of the Fourier kind), enc_b unused, progressive = 1 and enc_dim = 515 only: the reference has no plain
 *   network of this encoding, (5, 512, progressive 0) is refused.  For frequency f and a point x:
 *     u = (x_t + 1) F[0][f] + (x_y + 1) F[1][f] + (x_x + 1) F[2][f] (each x_d + 1 one fp32 sum, then fused multiply-adds from t to x);
 *     tri(w) = 2 r + 1 if r < 0 else 1 - 2 r,  r = fmod(w, 2) - 1, fmod TRUNCATING as C's and torch.fmod (the sign of w);
 *     feature 2 f = tri(u), feature 2 f + 1 = tri(u + 1).
 *   For w >= 0 that is a triangle wave of period 2 in [-1, 1]; for w < 0 the reference's values lie in (-5, -1] and jump at the negative
 *   integers, and the kernels give those values.  The frequencies are constants: the backward call is sininn_flownet_backward, the
 *   encgrad calls refuse this kind; masks, k_active, the spatial and the points calls are those of the other 515-wide networks.  The
 *   coordinate gradient is piecewise constant, d feature / d x_d = -+2 F[d][f] with the sign of the branch the forward pass took.
 * Borrowed pointers, 16-byte aligned (axis vectors, biases and the mask: 4), the caller's stream, non-zero return + sininn_last_error.
 * sininn_flownet_supported: 1 if the sizes are the ones the kernels are built for, else 0 (callers raise, there is no second path).
 * ---------------------------------------------------------------------------------------------- */
#define SININN_FLOWNET_RBF 0     /* enc_a = centres [512][3], enc_b = sigma [512]                                  */
#define SININN_FLOWNET_FOURIER 1 /* enc_a = frequencies [3][256], enc_b unused (FFN and UFF differ in the buffer only) */
#define SININN_FLOWNET_RBFG 3    /* enc_a = offsets [256][3], enc_b = sigma [256] (2 is not an encoding of this library) */
#define SININN_FLOWNET_PE 4      /* enc_a = freqs [4], enc_b unused; enc_dim 24 (progressive: 27)                   */
#define SININN_FLOWNET_PIECEWISE 5 /* enc_a = frequencies [3][256], enc_b unused; progressive only, enc_dim 515  */
typedef struct sininn_flownet_args {
  size_t struct_bytes;                    /* must be sizeof(sininn_flownet_args)                                          */
  int encoding;                           /* SININN_FLOWNET_*                                                             */
  int enc_dim, hidden, layers, out_dim;   /* 512 (progressive: 515; PE: 24 / 27), 256, 3, 4                               */
  int T, H, W;                            /* N = T H W points, at most 2^22                                               */
  float scale;
  const float *times, *ys, *xs;           /* [T], [H], [W]                                                                */
  const float *enc_a, *enc_b;
  const float* w[4];                      /* [256][512] (progressive: [256][515]), [256][256], [256][256], [4][256]       */
  const float* b[4];
  float* flows;                           /* forward: out [T][4][H][W]                                                    */
  float* saved; size_t saved_bytes;       /* forward: out or NULL; backward: in                                           */
  const float* dflows;                    /* backward: in [T][4][H][W]                                                    */
  float* gw[4]; float* gb[4];             /* backward: out                                                                */
  void* workspace; size_t workspace_bytes;/* backward; progressive forward                                                */
  int progressive;                        /* 0, or 1: layer 1 reads cat((t, y, x), enc) * mask                            */
  int k_active;                           /* progressive: 0 .. enc_dim, every mask entry from this index on is zero       */
  const float* mask;                      /* progressive: device [enc_dim]                                                */
} sininn_flownet_args;
int sininn_flownet_supported(const sininn_flownet_args* args);
size_t sininn_flownet_saved_bytes(int64_t n_points);
size_t sininn_flownet_workspace_bytes(int64_t n_points);
size_t sininn_flownet_forward_workspace_bytes(const sininn_flownet_args* args);
size_t sininn_flownet_encgrad_workspace_bytes(const sininn_flownet_args* args);
size_t sininn_flownet_posegrad_workspace_bytes(const sininn_flownet_args* args, int with_enc_grad);
int sininn_flownet_supported_dim(const sininn_flownet_args* args, int domain_dim);

/* The call descriptor: everything a call takes BESIDE the network descriptor, which it leaves unchanged (its size and its tag too).  One
 * struct serves the flow networks and SIREN.  `mode` states what the call is, bit by bit; nothing is inferred from a null pointer, and a
 * field whose bit is clear is not read.  A NULL call descriptor is the plain call: the descriptor's grid of points, three coordinates, no
 * extra output.  A new mode is one bit here, one branch in the validator (check_call, csrc/flownet_tile.h) and one clause in the Python
 * builder (flownet.py, _call).
 *
 *   bit          fields read                          shapes                                   workspace                          refused
 *   AT_POINTS    poses, n                             poses DEVICE [n][domain_dim] fp32;       saved / workspace sized for n      null poses, n < 1, n > 2^22
 *                                                     flows / dflows planar [4][n]
 *   SPATIAL      grid, res, centre_scale              grid DEVICE [res^3][515] fp32,           none (no forward pack)             null grid / centre_scale, res < 3, res^3 * 515 > 2^31 - 1,
 *                                                     centre_scale HOST [6]                                                       not progressive, PPE; SIREN; domain_dim 2
 *   ENCGRAD      g_enc_a, enc_workspace[_bytes]       g_enc_a DEVICE [3][256], OVERWRITTEN     sininn_flownet_encgrad_workspace_  forward / sample_mask; encoding != FOURIER, null g_enc_a,
 *   (backward)                                                                                 bytes(args), 16-byte aligned       null / short enc_workspace; SIREN; domain_dim 2
 *   POSEGRAD     g_poses, extra_workspace[_bytes]     g_poses DEVICE [n][3], OVERWRITTEN       sininn_flownet_posegrad_workspace_ forward / sample_mask; without AT_POINTS; null g_poses,
 *   (backward)                                                                                 bytes(args, ENCGRAD set) in        null / short extra_workspace; domain_dim 2
 *                                                                                              extra_workspace, which then holds
 *                                                                                              the ENCGRAD workspace too
 *                                                                                              (enc_workspace is not read);
 *                                                                                              SIREN: none
 *   domain_dim   3: points (t, y, x).  2: points (y, x), one frame pair (flow networks only, see below).  Anything else is refused.
 *   also refused: a wrong struct_bytes, an unknown bit, sininn_flownet_sample_mask without SPATIAL.
 * Every refusal comes before any launch and is one sentence under the call's name, flownet_<forward | backward | backward_encgrad |
 * backward_posegrad>[_spatial][_points] or flownet_sample_mask[_points] (siren_...), as the mode spells it.
 *
 * AT_POINTS (net(poses), trainer.py:43-44, pair_flow.py:58-59, progressive_controller.py:45-53): row p of poses = (t, y, x) of point p, a
 *   contiguous torch (n, 3) tensor, 4-byte alignment, read in place where the grid call reads the axis vectors:
 *     flows[c][p] = net(poses[p])[c] * scale              flows / dflows are [4][n] (the grid layout with T = H = 1, W = n)
 *   T, H, W, times, ys, xs of the descriptor are ignored and may be 0 / NULL; every other field keeps its meaning.  Tiles, partial sums and
 *   the order of every sum depend on n alone: a pose list that spells out meshgrid(times, ys, xs) gives bitwise the flows and gradients (and,
 *   SPATIAL, the sampled mask) of the grid call, two calls are bitwise equal and any valid k_active gives the same bits.
 * SPATIAL (progressive_controller.py:461-710 StashedSpatialController, what --spatially-adaptive builds; at a pose list: controller(poses),
 *   progressive_controller.py:655-680): every point has its own 515 mask values, interpolated trilinearly from the grid G (row-major,
 *   features contiguous: the controller's blurred mask).  The descriptor has progressive = 1; its `mask` is ignored and may be NULL.
 *   centre_scale is read during the call: centre (t, y, x), then scale (t, y, x), the reference's center_scale; identity is 0, 0, 0, 1, 1, 1.
 *   For the point with coordinates x_d, d = 0 .. 2 = (t, y, x), as interpolate_ does (progressive_controller.py:655-664), every operation a
 *   rounded fp32 one, nothing contracted:
 *     u_d = ((x_d - centre_d) * scale_d + 1) / 2 * max(res - 2, 1) + 0.5;   i0 = floor(u_d), i1 = ceil(u_d + 1e-6);
 *     a0 = i1 - u_d, a1 = u_d - i0 (their sum is 2 where u_d lies within 1e-6 below an integer, as in the reference);
 *     corner c = 0 .. 7 takes i / a number (c >> 2) & 1 of t, (c >> 1) & 1 of y, c & 1 of x: row = i_t + i_y res + i_x res^2 (t has
 *     stride 1), weight = (a_t a_y) a_x;   m_k(p) = sum over c in that order of weight_c * G[row_c][k].
 *   Corner indices are clamped to [0, res - 1] before the load: where the reference would raise an index error the edge cell is read.
 *   Nothing is validated on the device and nothing is read back.  Layer 1 reads cat((t, y, x), enc)_k * m_k(p): the mask multiplies the
 *   generated operand in registers, w[0] [256][515] is read in place.  gw[0][j][k] = sum_p dh1[p][j] feature_k[p] m_k(p), and for the Fourier
 *   encoding dE[p][k] = m_{3 + k}(p) sum_j dh1[p][j] w[0][j][3 + k] feeds g_enc_a.  k_active keeps its meaning: every entry of G in a column
 *   from k_active on must be zero (515 is always valid); any valid value gives bitwise the same flows and gradients (finite weights), every
 *   sum over points keeps its fixed order, and a column of gw[0] whose grid column is all zero is an exact +0.
 *   sininn_flownet_sample_mask writes m_k(p) for the points of the call, out [N][515] (device): what the kernels multiply by.
 * ENCGRAD: the frequency gradient of "Learnable frequencies" above, beside the eight gradients, which are bitwise those of the call without
 *   the bit.
 * POSEGRAD: everything the backward call at the pose list does (the eight gradients and, with ENCGRAD, g_enc_a are bitwise the same), and
 *   g_poses, which needs no initialisation: the gradient of sum(dflows * flows) with respect to poses, `scale` included:
 *     dE[p][k]    = sum_j dh1[p][j] w[0][j][k]           (progressive: w[0][j][3 + k] * mask[3 + k], an exact zero for a closed feature)
 *     g_poses[p][d] = sum_k dE[p][k] * d feature_k / d x_d (p)   (progressive: + mask[d] * sum_j dh1[p][j] w[0][j][d])
 *   with the derivative of each encoding evaluated from the forward pass's own inputs, x = poses[p], d = 0 .. 2 = (t, y, x):
 *     RBF      feature k = e_k = exp(-sigma_k^2 |x - c_k|^2):                  -2 sigma_k^2 (x_d - c_kd) e_k
 *     Fourier  features 2 f / 2 f + 1 = sin / cos(phi), phi = 2 pi x . F[:, f]:  2 pi F[d][f] (dE_sin cos(phi) - dE_cos sin(phi)) for the pair
 *              (fixed and learnable enc_a alike: enc_a is the matrix the call was given)
 *     RBFG     feature e = 2 exp(-sigma^2 |u|^2) - 1, u_d the wrapped, doubled offset of the forward pass:  -4 sigma^2 u_d (e + 1); the
 *              remainder's derivative with respect to its dividend is 1, so the gradient jumps where a coordinate wraps although e is continuous
 *     PE       feature 6 f + d = cos(w_f x_d): -w_f sin(w_f x_d);  feature 6 f + 3 + d = sin(w_f x_d): w_f cos(w_f x_d);  its own coordinate only
 *     ReLU gates are those the forward pass took (saved > 0).
 *   The order of every sum is fixed and depends on nothing but the encoding: the four features of a lane in index order, the 16 lanes of a
 *   feature group by an xor butterfly, the groups of 64 features in index order, then the coordinate column.  No atomics, nothing crosses a
 *   tile: two calls are bitwise equal, a point's gradient does not depend on n or on its place in the list, and any valid k_active gives
 *   the same bits.  There is no second derivative.  extra_workspace holds a packed, mask-folded copy of w[0] (SPATIAL: unmasked).
 *   With SPATIAL: g_poses[p][d] = sum_k (m_{3 + k}(p) dE[p][k]) * d feature_k / d x_d (p) + m_d(p) * sum_j dh1[p][j] w[0][j][d], dE[p][k] =
 *     sum_j dh1[p][j] w[0][j][3 + k], each product with the mask a rounded fp32 one, the order of every sum as above.  The mask is a CONSTANT
 *     of the point: the reference interpolates it under no_grad, so there is no d mask / d pose term, although m_k(p) is piecewise trilinear
 *     in the pose.
 * domain_dim = 2 (one frame pair: video-interpolation/pair_flow.py, ModelParams(domain_dim=2), poses (y, x)):
 *   networks  SININN_FLOWNET_RBF (enc_a = centres [512][2]), SININN_FLOWNET_FOURIER (enc_a = frequencies [2][256], rows y, x) and
 *             SININN_FLOWNET_RBFG (enc_a = offsets [256][2]); enc_b as above.  enc_dim 512, w[0] [256][512]; progressive: enc_dim 514, w[0]
 *             [256][514] = the columns of cat((y, x), enc), mask [514], k_active 0 .. 514, gw[0] [256][514] with an exact +0 where the mask is
 *             zero or an encoded column lies past k_active.  Every encoder evaluates the reference's two-term expressions; no t term exists.
 *   points    the descriptor's grid is (ys, xs): T must be 1, `times` is not read (NULL is fine), flows / dflows are [1][4][H][W]; AT_POINTS
 *             takes poses [n][2], columns (y, x).  The size queries are those of three coordinates.
 *   refused   SININN_FLOWNET_PE and SININN_FLOWNET_PIECEWISE (sininn_flownet_supported_dim is 0, the error names the dimension), T != 1, and
 *             SPATIAL, ENCGRAD, POSEGRAD: they exist for three coordinates only. */
#define SININN_FLOWNET_AT_POINTS 1u /* the points are `poses` [n][domain_dim], not the descriptor's grid                        */
#define SININN_FLOWNET_SPATIAL 2u   /* per-point mask from `grid`; the descriptor's mask is ignored                             */
#define SININN_FLOWNET_ENCGRAD 4u   /* backward: also g_enc_a, with enc_workspace                                               */
#define SININN_FLOWNET_POSEGRAD 8u  /* backward: also g_poses, with extra_workspace                                             */
typedef struct sininn_flownet_call {
  size_t struct_bytes;                    /* must be sizeof(sininn_flownet_call)                                          */
  unsigned mode;                          /* SININN_FLOWNET_* bits                                                        */
  int domain_dim;                         /* 3 or 2                                                                       */
  const float* poses; int64_t n;          /* AT_POINTS                                                                    */
  const float* grid; int res; const float* centre_scale;                       /* SPATIAL                                 */
  float* g_enc_a; void* enc_workspace; size_t enc_workspace_bytes;             /* ENCGRAD                                 */
  float* g_poses; void* extra_workspace; size_t extra_workspace_bytes;         /* POSEGRAD                                */
} sininn_flownet_call;
int sininn_flownet_forward(const sininn_flownet_args* args, const sininn_flownet_call* call, void* stream);
int sininn_flownet_backward(const sininn_flownet_args* args, const sininn_flownet_call* call, void* stream);
int sininn_flownet_sample_mask(const sininn_flownet_args* args, const sininn_flownet_call* call, float* out, void* stream);

/* The Jacobian of the network as an output with a gradient to the parameters (csrc/flownet_jacobian.h).  Plain arguments beside
 * the two descriptors, which keep their size, every meaning and every refusal; no mode bit is added.  dirs: the direction set D, bit 0 t,
 * bit 1 y, bit 2 x; slots of jac / djac / tsaved follow the set bits in that order.  With g_l = [h_l > 0], the gates of the value pass:
 *     t_1 = g_1 . (W1' dE_d(p) [+ wc[:, d]])   t_2 = g_2 . (W2 t_1)   t_3 = g_3 . (W3 t_2)   jac[slot][c][p] = scale * (W4 t_3)[c]
 *   W1' is the layer-1 matrix the forward pass multiplies (progressive: the mask-folded pack, wc its coordinate columns), dE_d the POSEGRAD
 *   derivative of the encoding above (RBF, Fourier); no bias enters a tangent.  jac is DEVICE planar [|D|][4][n], flow units per unit of
 *   the normalised coordinate.
 * sininn_flownet_jacobian_forward: does everything sininn_flownet_forward does with the same (args, call) in its training mode (flows and
 *   `saved` are bitwise that call's; args->saved must not be NULL; progressive: args->workspace as there), then writes jac and the gated
 *   tangents tsaved [|D|][3][Npad][256] (sininn_flownet_jacobian_saved_bytes(n, |D|) bytes, 16-byte aligned).
 * sininn_flownet_jacobian_backward: does everything sininn_flownet_backward does with the same (args, call) for args->dflows (gw / gb are
 *   bitwise that call's when djac is all zero), then adds to gw[0..3], for every d in D in the order t, y, x, the gradient of
 *   sum(djac_d * jac_d):  dt_3 = g_3 . (W4^T scale djac_d), dt_2 = g_2 . (W3^T dt_3), dt_1 = g_1 . (W2^T dt_2);
 *   gw[3] += (scale djac_d)^T t_3, gw[2] += dt_3^T t_2, gw[1] += dt_2^T t_1, gw[0][:, enc k] += mask_k sum_p dt_1[p] dE_d,k(p),
 *   gw[0][:, coord d] += mask_d sum_p dt_1[p].  The gates carry no gradient, the biases get none from a tangent, the poses and the
 *   encoding's buffers get none.  djac DEVICE [|D|][4][n]; tsaved: the forward call's; jac_workspace:
 *   sininn_flownet_jacobian_workspace_bytes(args, n, |D|) bytes, 16-byte aligned.  Every sum has a fixed order (partial sums in the
 *   workspace, reduced in index order, then value + t + y + x), no atomics: two calls are bitwise equal, any valid k_active gives the same bits.
 * Refused, each before any launch, in one sentence under flownet_jacobian_forward / flownet_jacobian_backward: dirs of 0 or above 7; a NULL
 *   call descriptor or one without AT_POINTS; SPATIAL, ENCGRAD, POSEGRAD; domain_dim != 3; an encoding other than SININN_FLOWNET_RBF /
 *   SININN_FLOWNET_FOURIER; NULL jac / djac / tsaved / jac_workspace / saved; short or misaligned buffers; and whatever the plain call refuses. */
size_t sininn_flownet_jacobian_saved_bytes(int64_t n_points, int n_dirs);
size_t sininn_flownet_jacobian_workspace_bytes(const sininn_flownet_args* args, int64_t n_points, int n_dirs);
int sininn_flownet_jacobian_forward(const sininn_flownet_args* args, const sininn_flownet_call* call, unsigned dirs, float* jac, float* tsaved,
                                    size_t tsaved_bytes, void* stream);
int sininn_flownet_jacobian_backward(const sininn_flownet_args* args, const sininn_flownet_call* call, unsigned dirs, const float* djac,
                                     const float* tsaved, size_t tsaved_bytes, void* jac_workspace, size_t jac_workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The SIREN flow network of the flow trainer: sine MLP on the raw coordinates, forward and backward (csrc/siren.hip).
 *   video-interpolation/model.py:123-146 SineLayer (sin(omega_0 * linear(x)), omega_0 = 30), model.py:149-171 SirenModel with the
 *   ModelParams defaults (model.py:18-28): 3 -> 256 -> 256 -> 256 -> 256 -> 4, four sine layers and a plain last nn.Linear; evaluated on the
 *   grid of FlowTrainer.forward (trainer.py:37-45) like the networks above: h_0 = (t, y, x) of meshgrid(times, ys, xs), N = T H W points,
 *     u_l = omega (W_l h_{l-1} + b_l),  h_l = sin(u_l)    l = 1 .. 4     w[0] [256][3], w[1..3] [256][256]
 *     out = W_5 h_4 + b_5                                                 w[4] [4][256]
 *     flows[t][c][y][x] = out[p][c] * scale
 *   The sine is the accurate full-range fp32 function (phases are tens of radians).  omega is read on every call.
 *   forward : writes flows; if saved != NULL (training) also what the backward call needs, sininn_siren_saved_bytes(N) bytes whose content is
 *             this library's business (today the phases u_1 .. u_4, [4][Npad][256], Npad = N rounded up to 64); every byte is written on
 *             every call.  Training and inference flows are bitwise equal.  No N x 3 pose list and (inference) no N x 256 activation is
 *             ever stored.
 *   backward: dflows [T][4][H][W] -> gw[0..4] / gb[0..4] (OVERWRITTEN, nn.Linear layout, scale folded in), dout = dflows * scale:
 *               gW5 = dout^T h_4        gb5 = sum_p dout
 *               dh_4 = dout W_5         dz_l = omega dh_l cos(u_l)
 *               gW_l = dz_l^T h_{l-1}   gb_l = sum_p dz_l     dh_{l-1} = dz_l W_l
 *             Needs the saved buffer of the forward call on the same weights and omega, and a workspace of
 *             sininn_siren_workspace_bytes(N) bytes; sums over points are added in a fixed order (no floating-point atomics): two calls on
 *             the same inputs are bitwise equal.
 * Borrowed pointers, 16-byte aligned (axis vectors and biases: 4), the caller's stream, non-zero return + sininn_last_error, N <= 2^22.
 * Refused before any launch: a wrong struct_bytes; sizes other than in_dim 3, hidden 256, layers 3, out_dim 4 and an omega that is not
 * finite and positive (the message lists what is supported); null or short buffers.  sininn_siren_supported: 1 if the sizes and omega are
 * supported, else 0 (callers raise, there is no second path).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sininn_siren_args {
  size_t struct_bytes;                    /* must be sizeof(sininn_siren_args)                                            */
  int in_dim, hidden, layers, out_dim;    /* 3, 256, 3 (hidden sine layers after the first), 4                            */
  float omega;                            /* omega_0 of every sine layer, finite and > 0 (the reference: 30)              */
  int T, H, W;                            /* N = T H W points, at most 2^22                                               */
  float scale;
  const float *times, *ys, *xs;           /* [T], [H], [W]                                                                */
  const float* w[5];                      /* [256][3], [256][256] x 3, [4][256]                                           */
  const float* b[5];
  float* flows;                           /* forward: out [T][4][H][W]                                                    */
  float* saved; size_t saved_bytes;       /* forward: out or NULL; backward: in                                           */
  const float* dflows;                    /* backward: in [T][4][H][W]                                                    */
  float* gw[5]; float* gb[5];             /* backward: out                                                                */
  void* workspace; size_t workspace_bytes;/* backward                                                                     */
} sininn_siren_args;
int sininn_siren_supported(const sininn_siren_args* args);
size_t sininn_siren_saved_bytes(int64_t n_points);
size_t sininn_siren_workspace_bytes(int64_t n_points);
/* The call descriptor is sininn_flownet_call, above (NULL: the plain call).  AT_POINTS: h_0 = poses[p], DEVICE [n][3] fp32 row-major (4-byte
 * alignment), read in place; flows / dflows are [4][n], flows[c][p] = out[p][c] * scale; T, H, W, times, ys, xs of the descriptor are ignored
 * (0 / NULL); saved and workspace have the sizes of sininn_siren_saved_bytes(n) / sininn_siren_workspace_bytes(n).  The same kernels: a pose
 * list that spells out the grid gives bitwise the grid call's flows and gradients.  POSEGRAD (backward, with AT_POINTS): also g_poses [n][3]
 * (DEVICE, OVERWRITTEN, the layout of poses): g_poses[p][d] = sum_j dz_1[p][j] w[0][j][d], dz_1 = omega dh_1 cos(u_1), `scale` included; 256
 * terms in a fixed order, no atomics, no extra workspace; the ten gradients are bitwise those of the call without the bit.  Refused before
 * any launch: null poses, n < 1, n > 2^22, a null g_poses, SPATIAL, ENCGRAD, a domain_dim other than 3, and everything the grid calls refuse. */
int sininn_siren_forward(const sininn_siren_args* args, const sininn_flownet_call* call, void* stream);
int sininn_siren_backward(const sininn_siren_args* args, const sininn_flownet_call* call, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LAMB, the optimiser of the flow trainer (video-interpolation/trainer.py:134-135: apex.optimizers.FusedLAMB(params, lr=lr)),
 * restated from apex/optimizers/fused_lamb.py and its multi_tensor_lamb stages 1 and 2 (csrc/lamb.hip).  fp32.
 * One step, t = step (from 1), gs = grad_scale:
 *   G      = sqrt( sum over ALL tensors of ALL param groups of (gs*g)^2 )        -- one global norm
 *   clip   = G / max_grad_norm  if G > max_grad_norm  else 1                      -- max_grad_norm <= 0: clip = 1
 *   bc1,bc2 = 1 - beta1^t, 1 - beta2^t   (both 1 if not bias_correction; computed on the host in double, as 1 - beta1 and 1 - beta2 are)
 *   beta3  = 1 - beta1 if grad_averaging else 1
 *   per element:  sg = gs*g / clip
 *                 m  = beta1*m + beta3*sg ;   v = beta2*v + (1-beta2)*sg*sg
 *                 adam_w_mode:      u = (m/bc1) / (sqrt(v/bc2) + eps) + wd*p
 *                 not adam_w_mode:  sg += wd*p before m, v ;  u = (m/bc1) / (sqrt(v/bc2) + eps)
 *   per tensor:   pn = ||p||_2 (before the step),  un = ||u||_2
 *                 ratio = lr * pn/un   if (use_nvlamb or wd != 0) and pn != 0 and un != 0   else lr
 *                 p -= ratio * u
 * g is read only (apex overwrites it with u; here u has a buffer of its own).
 * Layout: one param group = flat buffers p, g, m, v, u of n floats (n % 4 == 0); tensor k occupies [tensor_offsets[k],
 *   tensor_offsets[k] + numel_k), every offset a multiple of 4, tensor_offsets[n_tensors] = n; the padding between tensors belongs to
 *   no tensor, is never read or written and enters no norm.  `chunks` is a DEVICE table [n_chunks][3] of int64 (tensor, begin, len),
 *   sorted, begin % 4 == 0, a chunk never crosses a tensor; `tensor_offsets` a DEVICE table of n_tensors + 1 int64.  A chunk that does
 *   not lie inside its tensor and inside n is skipped by the kernels.
 * Sums are per-chunk partials in the workspace, added in chunk-index order: no floating-point atomics, results independent of the
 *   grid size, two calls from the same state bitwise equal.  Nothing is read back: G, clip and the ratios stay on the device.
 * Several param groups share `norm_slots` (DEVICE, n_groups floats): sininn_lamb_grad_norm writes slot `group` with this group's
 *   sum of (gs*g)^2 (two launches); sininn_lamb_step reads all n_groups slots, so call grad_norm for EVERY group before step for any.
 *   sininn_lamb_step is three launches: stage 1 (m, v, u, partials of p^2 and u^2), one block per tensor for the ratio, stage 2.
 * Workspace: sininn_lamb_workspace_bytes(n_chunks, n_tensors) bytes, 16-byte aligned; its first n_tensors floats are the trust
 *   ratios of the last step (diagnostic).  Every extent is checked before anything is launched.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sininn_lamb_args {
  size_t struct_bytes;                       /* must be sizeof(sininn_lamb_args)                                              */
  float* p; const float* g; float* m; float* v; float* u;   /* n floats each, 16-byte aligned                                */
  int64_t n;
  const int64_t* chunks; int64_t n_chunks;
  const int64_t* tensor_offsets; int n_tensors;
  double lr, beta1, beta2, eps, weight_decay, max_grad_norm, grad_scale;   /* the kernels compute with their fp32 images; 1 - beta1,
                                                1 - beta2, the bias corrections and lr * pn/un are formed in double first   */
  int step;                                  /* >= 1                                                                          */
  int bias_correction, adam_w_mode, grad_averaging, use_nvlamb;
  float* norm_slots; int group, n_groups;
  void* workspace; size_t workspace_bytes;
} sininn_lamb_args;
size_t sininn_lamb_workspace_bytes(int64_t n_chunks, int n_tensors);
int sininn_lamb_grad_norm(const sininn_lamb_args* args, void* stream);
int sininn_lamb_step(const sininn_lamb_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The flow trainer's step beyond the losses (video-interpolation/trainer.py:47-132; csrc/flowtrain.hip).  fp32 tensors, NCHW.
 * Every reduction is a per-block partial in a caller-provided buffer, combined by one wave in a fixed order: no floating-point
 * atomics, two calls bitwise equal, the buffers need no initialisation.  Every extent is checked before anything is launched.
 *
 * End-point error (trainer.py:58, 97, 110):  out[0] = mean over (n, y, x) of sqrt((flow[n,0] - gt[n,0])^2 + (flow[n,1] - gt[n,1])^2).
 *   `flow` is read in place from a larger tensor: sample n starts at flow + n * flow_sample_stride (floats, >= 2 h w), its two channel
 *   planes are contiguous -- channels 0..1 or 2..3 of the (t, 4, h, w) tensor of the flow network, stride 4 h w.  `gt` is a contiguous
 *   (n, 2, h, w).  Per pixel fp32, each operation rounded once; the sum is carried in double; the mean is rounded to fp32 once and
 *   stays on the device.  `partials`: DEVICE doubles, at least the count returned for (n, h, w) by the _partials call.
 * ---------------------------------------------------------------------------------------------- */
int64_t sininn_flow_epe_partials(int n, int h, int w);
int sininn_flow_epe(const float* flow, int64_t flow_sample_stride, const float* gt, int n, int h, int w, double* partials,
                    int64_t n_partials, float* out, void* stream);
/* out[n,c,y,x] = mask[n, c % mask_channels, y, x] * (splat[n,c,y,x] != 0)   (trainer.py:64, 68): c = 3, mask_channels 1 or 3; -0.0
 * counts as zero; the product is formed, so it is bitwise what torch's `mask * (splat != 0)` gives.  Not differentiable, as in the
 * reference. */
int sininn_splat_mask(const float* mask, int mask_channels, const float* splat, int n, int c, int h, int w, float* out, void* stream);
/* flow2img (my_utils/flow_viz.py:6-77) for a batch: flow (n, 2, h, w) fp32 -> img (n, 3, h, w) bytes.  Per frame:
 *   u, v = clip(flow, -clip, clip), both 0 where |u| or |v| > 1e7 (those pixels come out black)
 *   maxrad = max(-1, max sqrt(u^2 + v^2))        fp32, as numpy evaluates it on the fp32 array; a NaN anywhere in the frame gives -1
 *                                                (Python's max(-1, nan))
 *   u, v = u / maxrad (fp32) + 2.220446049250313e-16 (float64 from here on); NaN pixels -> u = v = 0 and a black pixel
 *          (this is the whole frame when maxrad == 0)
 *   rad = sqrt(u^2 + v^2);  fk = (atan2(-v, -u) / pi + 1) / 2 * 54 + 1;  k0 = floor(fk);  k1 = k0 + 1, 56 -> 1;  f = fk - k0
 *   col = (1 - f) wheel[k0 - 1] / 255 + f wheel[k1 - 1] / 255;  rad <= 1: col = 1 - rad (1 - col), else col *= 0.75
 *   img = floor(255 col)
 * `wheel`: DEVICE [55][3] doubles, the Middlebury colour wheel (make_color_wheel), built by the caller.  `workspace`: DEVICE floats,
 * at least the count returned for (n, h, w) by the _workspace_floats call; n <= 65535. */
int64_t sininn_flow2img_workspace_floats(int n, int h, int w);
int sininn_flow2img(const float* flow, int n, int h, int w, float clip, const double* wheel, int wheel_rows, float* workspace,
                    int64_t workspace_floats, uint8_t* img, void* stream);
/* The per-pixel photometric error of a step and its stash into the loss log of a spatially adaptive controller (DESIGN 16.2;
 * progressive_controller.py:596-618 with the per-point loss the reference leaves undefined).  softmax*, frame*: (B, C, H, W), C = 1 or 3;
 * mask*: (B, mask_channels, H, W), mask_channels 1 or C, the masks after sininn_splat_mask.
 *   E[b][y][x]         = 0.5 (mean_c |m1 S1 - m1 I1| + mean_c |m2 S2 - m2 I2|)      the integrand of the two L1 terms; every product,
 *                                                                                  difference and sum rounded once, no FMA
 *   log_buffer[cell]  += sum of alpha(p, k) E[p] over the points p = (times[b], ys[y], xs[x]) and their 8 corners k with cell(p, k) == cell
 *   log_counter[cell] += the same sum of alpha(p, k)
 * Per axis, u = ((v - centre) scale + 1) / 2 * max(res - 2, 1) + 0.5 in fp32, the cells floor(u) and ceil(u + 1e-6) clamped to the grid,
 * their weights ceil(u + 1e-6) - u and u - floor(u): alpha is the product over the axes, cell = i_t + res (i_y + res i_x) -- the cells and
 * weights the flow-network kernels interpolate the per-point mask with.  times: B floats, ys: H, xs: W, all DEVICE; centre and scale by value.
 * log_buffer, log_counter: DEVICE [res^3], read, added to and written.  Three launches, no atomics, every sum in a fixed order: two
 * calls on equal inputs give bitwise equal buffers.  E (may be NULL): DEVICE (B, H, W), written when given.  `workspace`: DEVICE
 * floats, at least the count the _workspace_floats call returns (0 for sizes the call refuses); needs no initialisation.
 * 3 <= res <= 1024, H <= 65535, B <= 65534.  The call reads no device memory on the host.  Not differentiable. */
int64_t sininn_flow_error_stash_workspace_floats(int B, int H, int W, int res);
int sininn_flow_error_stash(const float* softmax1, const float* frame1, const float* mask1, const float* softmax2, const float* frame2,
                            const float* mask2, int mask_channels, int B, int C, int H, int W, const float* times, const float* ys,
                            const float* xs, int res, float centre_t, float centre_y, float centre_x, float scale_t, float scale_y,
                            float scale_x, float* log_buffer, float* log_counter, float* E, float* workspace, int64_t workspace_floats,
                            void* stream);

/* ----------------------------------------------------------------------------------------------
 * Frame synthesis from a pair of flows (csrc/flowsynth.hip).  i0, i1: frames (B, C, H, W), C = 1 or 3; f01, f10: flows
 * (B, 2, H, W) in pixels, channel 0 = x; tau: K DEVICE floats in [0, 1] (not validated here: the call reads no device memory on the
 * host), K <= 64.  out (B, K, C, H, W):
 *   Z0 = -20 mean_c |i0 - warp(i1, f01)|, Z1 = -20 mean_c |i1 - warp(i0, f10)|    warp = sininn_flow_warp_l1's rule; on an axis of
 *                                                                                 length 1 its sample lies outside the frame (0)
 *   S0 = softmax-splat(i0, tau_k f01, Z0), S1 = softmax-splat(i1, (1 - tau_k) f10, Z1);  N0, N1 = the splatted exp(Z) channels
 *   a0 = (1 - tau_k) (N0 != 0), a1 = tau_k (N1 != 0);  out = (a0 S0 + a1 S1) / (a0 + a1), and (1 - tau_k) i0 + tau_k i1 where
 *   a0 + a1 == 0; -0.0 counts as zero.
 * out_u8 (may be NULL): the same layout in bytes, clamp(round-half-even(255 out), 0, 255).  `workspace`: DEVICE floats, at least
 * the count the _workspace call returns (B K 2 (C + 1) H W; 0 for a non-positive size); it is zeroed inside the call, on `stream`,
 * so it needs no initialisation.  Two kernel launches whatever K is.  Not differentiable. */
int64_t sininn_flow_synth_workspace(int B, int K, int C, int H, int W);
int sininn_flow_synth(const float* i0, const float* i1, const float* f01, const float* f10, const float* tau, int B, int K, int C,
                      int H, int W, float* workspace, int64_t workspace_floats, float* out, unsigned char* out_u8, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Frame quality (csrc/framequality.hip): PSNR and mean SSIM of predicted frames against real ones.  pred, target: DEVICE
 * (B, C, H, W) fp32, contiguous, C = 1 or 3, H, W >= 11.  Per frame b:
 *   sqerr[b]      = sum_{c,y,x} (p - t)^2       difference and square rounded once each in fp32; the sum in double, in a fixed order
 *   out[0][b] mse = sqerr / (C H W)             formed in double, rounded to fp32 once
 *   out[1][b] psnr = 10 log10(1 / mse)          data range 1; +inf where mse == 0; formed on the device
 *   out[2][b] ssim = the mean over channels and over the (H - 10)(W - 10) windows per channel ("valid": no padding) of
 *       ((2 mu_p mu_t + C1)(2 s_pt + C2)) / ((mu_p^2 + mu_t^2 + C1)(s_p + s_t + C2)),   C1 = 0.01^2, C2 = 0.03^2   (Wang et al. 2004)
 *     mu_p, mu_t, E[pp], E[tt], E[pt]: the moments under the 11 x 11 window w[i] w[j], filtered along x, then y, in fp32;
 *     s_p = E[pp] - mu_p^2, s_t = E[tt] - mu_t^2, s_pt = E[pt] - mu_p mu_t.  Every operation of the formula is rounded once and none
 *     is contracted, so a frame against itself gives exactly 1 in every window.  The mean is carried in double, in a fixed order.
 * `window`: 11 HOST floats, w[i] = exp(-(i - 5)^2 / 4.5) / sum for the standard sigma = 1.5; passed to the kernel by value.
 * ssim_map (may be NULL): DEVICE (B, C, H - 10, W - 10), the per-window values.  sqerr: DEVICE B doubles.  out: DEVICE 3 B floats.
 * quantize != 0: both inputs first become bytes by sininn_flow_synth's out_u8 rule, byte = clamp(round-half-even(255 v), 0, 255)
 * with the product 255 v rounded to fp32 and NaN giving 0; sqerr is then the integer sum of squared byte differences (exact in the
 * double), mse = sqerr / (255^2 C H W), and SSIM is taken on byte / 255 rounded to fp32.
 * `workspace`: DEVICE, 8-byte aligned, at least the count of floats the _workspace_floats call returns (0 for a shape the call
 * refuses); one partial per block, so it needs no initialisation.  Two launches, no atomics: two calls on equal inputs give equal
 * bits, and a frame's results do not depend on B or on its place in the batch.  B C H W <= 2^31 - 1.  The call reads no device
 * memory on the host.  Not differentiable. */
int64_t sininn_frame_quality_workspace_floats(int B, int C, int H, int W);
int sininn_frame_quality(const float* pred, const float* target, int B, int C, int H, int W, int quantize, const float* window,
                         float* workspace, int64_t workspace_floats, double* sqerr, float* out, float* ssim_map, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Frame synthesis by gathering (csrc/flowgather.hip): the flows are taken at the in-between time, on the grid of the frame
 * being synthesized, and both source frames are read through a backward warp.  i0, i1: DEVICE (B, C, H, W) fp32, contiguous, C = 1 or 3.
 * flows: DEVICE (T', 4, H, W) fp32 read in place: time slice t starts at flows + t * flow_sample_stride (floats, >= 4 H W) and its four
 * channel planes are contiguous; channels 0..1 the forward flow (x, y), 2..3 the backward one, in pixels.  slots: DEVICE (B, K, 6)
 * int32, per output frame idx0, idx1 (the time slices of G0, G1), ch0, ch1 (0 or 2, their first channel) and the bit patterns of the
 * floats c0, c1.  tau: DEVICE K floats in [0, 1].  out: DEVICE (B, K, C, H, W); out_u8 (may be NULL): the same layout in bytes,
 * clamp(round-half-even(255 out), 0, 255).  Per output pixel p = (x, y), every operation rounded once and none contracted:
 *   q0 = p + c0 G0(p), q1 = p + c1 G1(p)                 the product is rounded, then the sum
 *   (W0, n0) = sample(i0, q0), (W1, n1) = sample(i1, q1) bilinear with pixel centres at integers; a tap outside the frame adds 0 to W
 *                                                        and to n, the sum of the weights inside; a coordinate that is not finite or
 *                                                        is 1e9 or more in size has no tap inside
 *   a0 = 1 - tau, a1 = tau, L = a0 i0(p) + a1 i1(p)
 *   out = (a0 W0 + a1 W1 + e L) / (a0 n0 + a1 n1 + e),   e = 2^-10
 * The slot table is NOT validated on the device: the caller guarantees 0 <= idx < T' and ch in {0, 2}.  k_loop != 0: a lane walks the
 * K times of its pixel and loads i0(p), i1(p) once; 0: one lane per (b, k, y, x).  Both give the same bits.  One launch whatever K is,
 * no workspace, no atomics: equal inputs give equal bits, and a frame's result does not depend on B or on its place in the batch.
 * H W <= 2^31 - 1 and B K ceil(H W / 256) <= 2^31 - 1.  Its gradient with respect to `flows`: sininn_flow_gather_bwd. */
int sininn_flow_gather(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                       const float* tau, int B, int K, int C, int H, int W, int k_loop, float* out, unsigned char* out_u8,
                       void* stream);

/* The occlusion-aware form of sininn_flow_gather.  Every argument of that call, with its meaning and its checks, and two
 * visibility planes per pair: m0, m1 DEVICE (B, 1, H, W) fp32, contiguous, 4-byte aligned, not inside out or out_u8.  m0[b] is 1 where
 * a pixel of i0[b] is visible in i1[b], m1[b] the same for i1[b] in i0[b]; they are read as numbers of any value and nothing is
 * indexed with them.  With S(X, q) the four taps and weights of W (a tap outside the frame adds 0),
 *   o0 = S(1 - m0, q0),  o1 = S(1 - m1, q1);   v0 = 1 - o1,  v1 = 1 - o0;   b0 = a0 v0,  b1 = a1 v1
 *   out = (b0 W0 + b1 W1 + e L) / (b0 n0 + b1 n1 + e)
 * each operation rounded once: a sample is trusted unless the surface the OTHER sample found is hidden in its frame.  With m0 = m1 = 1
 * the result has the bits of sininn_flow_gather; where both v are 0 it is L.  One launch, no workspace, no atomics: equal inputs give
 * equal bits.  It has no gradient. */
int sininn_flow_gather_visible(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                               const float* tau, const float* m0, const float* m1, int B, int K, int C, int H, int W, int k_loop,
                               float* out, unsigned char* out_u8, void* stream);

/* The gradient of sininn_flow_gather with respect to `flows`.  i0 .. tau, B .. W as in sininn_flow_gather; grad_out:
 * DEVICE (B, K, C, H, W), contiguous, d loss / d out.  dflows: DEVICE (T, 4, H, W), contiguous, every element written.  At pixel p
 * of row (b, k), with D = a0 n0 + a1 n1 + e and out_c recomputed as the forward pass rounds it,
 *   dG0 = c0 a0 / D  sum_c g_c (grad_q W0_c - out_c grad_q n0),   dG1 = c1 a1 / D  sum_c g_c (grad_q W1_c - out_c grad_q n1)
 * grad_q: the derivative of the bilinear interpolant of the zero-padded plane in the cell floor(q) (on a cell border: the right-hand
 * derivative); a sample whose coordinate is not finite, or 1e9 or more in size, has gradient 0.  dG0 is added to channels ch0, ch0 + 1
 * of slice idx0, dG1 to channels ch1, ch1 + 1 of slice idx1; elements no row names are 0.  No gradient to the frames, tau or the
 * coefficients.  No atomics: the rows that share a target are summed in ascending b K + k, dG0 before dG1.
 * reduce_list: DEVICE ints, NOT validated on the device -- for each of the 2 T targets (2 slice + ch / 2) the begin of its entries,
 * 2 T + 1 ints (the last: the number of entries), then the entries 2 (b K + k) + which (0: dG0, 1: dG1), ascending within a target;
 * reduce_ints: its length.  Two launches: the per-row gradients go to `workspace` (DEVICE floats, at least what the _workspace call
 * returns, B K 4 H W; 0 for a non-positive size; no initialisation), a second kernel sums them.  reduce_list == NULL: the caller
 * guarantees that no two (row, sample) name the same target; dflows is zeroed and the one kernel writes in place, `workspace` is
 * not used and may be NULL.  Both paths give the same bits on such a table.  T 4 ceil(H W / 256) <= 2^31 - 1.  Once differentiable. */
int64_t sininn_flow_gather_bwd_workspace(int B, int K, int H, int W);
int sininn_flow_gather_bwd(const float* i0, const float* i1, const float* flows, int64_t flow_sample_stride, const int* slots,
                           const float* tau, const float* grad_out, int B, int K, int C, int H, int W, int T, const int* reduce_list,
                           int64_t reduce_ints, float* workspace, int64_t workspace_floats, float* dflows, void* stream);

/* The same rule at a list of N points.  i0, i1: DEVICE (B, C, H, W) fp32, contiguous, C = 1 or 3.  pix: DEVICE (N, 2)
 * fp32, (y, x) in pixels, any value, 8-byte aligned; pair: DEVICE N int32, the pair of the batch a point reads; tau: DEVICE N floats;
 * rev: DEVICE N bytes, or NULL for none set.  flows: DEVICE (S, 4, N) fp32, contiguous, S = 1 or 2, rows (x, y) forward, (x, y)
 * backward.  G1 = flows[0, 0:2, n], c1 = 1 - tau[n];  G0 = flows[1, 2:4, n], c0 = tau[n] where S == 2 and rev[n] == 0, else G0 = G1,
 * c0 = -tau[n].  blend: HOST R floats, R in 1..4, or NULL (R must be 1): a1 = tau[n] per point.  out: DEVICE (R, N, C),
 *   out[r, n, c] = (a0 W0 + a1 W1 + e (a0 H0 + a1 H1)) / (a0 n0 + a1 n1 + e),   a1 = blend[r], a0 = 1 - a1, e = 2^-10
 * with (W0, n0) = sample(i0[b], p + c0 G0), (W1, n1) = sample(i1[b], p + c1 G1), H0 = sample(i0[b], p).W, H1 = sample(i1[b], p).W and
 * `sample` that of sininn_flow_gather.  Nothing on the device is trusted: a pair outside [0, B) gives a row of zeros (and a zero
 * gradient), a coordinate that is not finite or is 1e9 or more in size has no tap, and no value makes the kernel read outside its
 * inputs.  One launch, one lane per point, no workspace, no atomics.  N <= 2^31 - 1, H W <= 2^31 - 1.
 * _bwd: grad_out DEVICE (R, N, C); dflows DEVICE (S, 4, N), every element written by the lane of its column: dG1 in [0, 0:2], dG0 in
 * [1, 2:4] -- or, where G0 = G1, added as dG0 + dG1 -- and zeros elsewhere; the R blends are summed in ascending r.  The formulas
 * are those of sininn_flow_gather_bwd.  One launch; equal inputs give equal bits.  Once differentiable. */
int sininn_flow_gather_at(const float* i0, const float* i1, const float* flows, const float* pix, const int* pair, const float* tau,
                          const unsigned char* rev, const float* blend, int R, int S, int64_t N, int B, int C, int H, int W, float* out,
                          void* stream);
int sininn_flow_gather_at_bwd(const float* i0, const float* i1, const float* flows, const float* pix, const int* pair,
                              const float* tau, const unsigned char* rev, const float* blend, const float* grad_out, int R, int S,
                              int64_t N, int B, int C, int H, int W, float* dflows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SININN_H */
