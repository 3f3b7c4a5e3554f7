// The flow-field network of the flow trainer (reference: video-interpolation/model.py, RbfModel / FFModel / UFFModel with the
// ModelParams defaults, evaluated by FlowTrainer.forward, video-interpolation/trainer.py:37-45):
//     poses = meshgrid(times, linspace(-1, 1, h), linspace(-1, 1, w))            N = t h w points of 3 coordinates
//     enc   = exp(-sigma_k^2 |x - c_k|^2)                       (RBF,  512 centres,      model.py:349-356)
//           | sin / cos (2 pi x . f_k), interleaved             (FFN / UFF, 256 frequencies, model.py:230-238)
//           | 2 exp(-sigma_k^2 |((x + o_k [+ 1 / sigma_k]) mod p_k) 2 - p_k|^2) - 1, p_k = 2 / sigma_k, the pair interleaved
//                                                               (RBFG, 256 frequencies, model.py:375-387)
//           | cos / sin (freqs_f x_d), feature 6 f + d the cosine, 6 f + 3 + d the sine   (PE, 4 frequencies x 3 coordinates: 24
//                                                               features, model.py:321-340)
//           | tri(u), tri(u + 1), u = (x + 1) . f_k, interleaved; tri(w) = 2 r + 1 if r < 0 else 1 - 2 r, r = fmod(w, 2) - 1 with
//             torch.fmod's truncation          (MPFF, 256 frequencies, model.py:634-646; progressive only)
//     h1 = relu(enc W1^T + b1)   h2 = relu(h1 W2^T + b2)   h3 = relu(h2 W3^T + b3)   out = h3 W4^T + b4        (model.py:36-43)
//     flows[t][c][y][x] = out[p][c] * scale                                                                    (trainer.py:44)
// fp32 on v_mfma_f32_16x16x4_f32.  Neither the N x 3 poses nor the N x 512 encoding exist in memory in either pass: a lane
// computes the four encoded features its A fragment needs from the point's three coordinates (flownet_fwd_kernel) or writes
// them straight into the LDS operand tile (flownet_wgrad_kernel<.., true>); both call encode4, so the weight gradient of layer 1
// sees bitwise the encoding the forward pass multiplied.
//
// structure: Enc<KIND> is the one description of an encoding (live features, padded K width, whether enc_b is read, whether enc_a has a
//           gradient); the row strides of W1, the pack size, the K steps, the weight-gradient tile and its partial sums are derived from
//           it there and nowhere else.  for_kind turns the run-time `encoding` into that compile-time kind for every launch, for
//           flownet_supported and for the text of its refusal.  A new encoding is one Enc<> row, one case in for_kind and one branch
//           of encode4.  The mode of a call is described once as well: for_mode turns (encoding, progressive, spatial) into the three
//           template arguments for the forward and the backward dispatch, forward_kind_launch<KIND, PROG, SPATIAL> is the one forward
//           launch, tile_lds / wgrad_lds are the LDS size of every launch of a kernel mode, check_head is the head of every entry point
//           (the struct, the support table and, spatial, the refusals of that mode, made once under the entry point's own name).
//           Shared with siren.hip through flownet_tile.h: the tile, gemm_lds, mfma_k4 (the coordinate K group), store_acc and its
//           epilogues, copy_tile_out, stage_coord, and on the host the point-grid part of a descriptor
//           (check_points), check_layers, check_saved and the buffer checks of a forward and a backward call.  siren.hip also calls
//           hidden_wgrad_launch below.  The output layer, dout, the tile load, the column sums and the transpose kernel are spelled out
//           here and there: as helpers they changed the instructions, or the placement, of the kernels that use them.
//
// forward   flownet_fwd_kernel: block = 256 threads (4 waves, two blocks per CU), grid-stride over 64-point tiles.  Wave w owns
//           hidden columns [64 w, 64 w + 64) of all 64 rows: 16 accumulator tiles.  Layer 1's A operand comes from encode4, layers
//           2 / 3 read the previous hidden tile from LDS ([64][260] floats, ONE buffer: the accumulators hold the next tile until
//           every wave has finished reading), the weights stream from L2 as 16-byte loads of nn.Linear's own [out][in] layout (no
//           packing).  Layer 4 (256 -> 4) is 256 dot products on the vector ALU.  Training mode copies each post-ReLU tile to
//           `saved` ([3][Npad][256]); inference writes the flows only.
// backward  flownet_bwd_chain_kernel: per tile  dout = dflows * scale;  gW4 / gb4 partials in registers over the block's tiles (gb4 in double);
//           dh3 = (dout W4) . [h3 > 0] on the vector ALU in place over the h3 tile;  dh2 = (dh3 W3) . [h2 > 0],
//           dh1 = (dh2 W2) . [h1 > 0] with the forward's GEMM loop on transposed weights;  dh1..3 -> workspace.
//           flownet_wgrad_kernel: gW_l[j][k] = sum_p dh_l[p][j] in_l[p][k] (in_1 = the regenerated encoding), gb_l = sum_p dh_l: a block
//           owns a 128 x 128 output tile and a fixed set of point tiles (split over points), partial sums go to the workspace and
//           flownet_reduce_kernel adds them in a fixed order: no floating-point atomics, two runs are bitwise equal.
// Rows of the last tile beyond N are computed on a clamped point in the forward pass and carry dout = 0 in the backward pass, so
// saved / workspace rows are always written before they are read and contribute exact zeros to every sum.
//
// progressive (PRBF / PFF / PUFF of model.py:526-625 under a controller's mask, progressive_controller.py:14-158): the input of layer 1
//           is cat((t, y, x), enc) * mask, 515 features, W1 [256][515].  flownet_pack_kernel folds the mask into the weights once per
//           call ((e m) w = e (m w)): W1p = W1[:, 3:] * mask[3:] as an aligned [256][512] matrix and the three coordinate columns as
//           [256][4] (padded with a zero), so the K loop and encode4 are the ones above; the coordinates are one more K group of four
//           on the MFMA (16 of 2064 layer-1 MFMAs per wave and tile).  The K loop stops after the last open feature (k_active, from
//           the host), rounded up to 16: the skipped terms are e * 0, so skipping is exact.  The chain kernel does not see layer 1's
//           input and is shared.  flownet_wgrad_kernel<.., true, true> adds the three coordinate-weighted column sums of the dh1 tile
//           next to gb1 and is launched on the open 128-column tiles only; flownet_reduce_l1_kernel scatters the sums into
//           nn.Linear's [256][515] layout, times the mask, exact zeros where the mask is zero.
//
// points    (SININN_FLOWNET_AT_POINTS) the coordinates of point p are row p of a caller's pose list [N][3] instead of an entry of each axis
//           vector: point_coord (flownet_tile.h) branches on q.poses, a kernel argument, and the host sets T = H = 1, W = N, which makes
//           the [T][4][H][W] indexing of flows / dflows the planar [4][N].  No kernel is instantiated for it and nothing else differs:
//           tiles, `saved`, workspaces and the order of every sum depend on N alone, so a pose list that spells out a grid gives the grid
//           call's bits.  Combined with the spatial mode (AT_POINTS | SPATIAL) it is PoseList plus Spatial in one FlowNetDev:
//           the SPATIAL instantiations below take a point's coordinates through point_coord as well, so they serve a pose list as they are.
//
// two coordinates (domain_dim = 2 in the call descriptor: one frame pair, poses (y, x)) the number of coordinates is a template
//           parameter DIM of flownet_fwd_kernel, flownet_wgrad_kernel, flownet_pack_kernel and flownet_reduce_l1_kernel, 3 by default: the
//           three-coordinate instantiations are the code they were.  DIM = 2 exists for the Enc<> rows that say PAIR (RBF, Fourier, RBFG):
//           point_coord_dim<2> reads two values per point, encode4<KIND, 2> reads centres [512][2] / frequencies [2][256] / offsets [256][2]
//           and evaluates two-term expressions (no zero is fed for t: in RBFG it would not drop out), the progressive W1 is [256][514] and
//           its two coordinate columns fill the [256][4] K group with two zero columns, the coordinate sums of gW1 are two.  The chain
//           kernel, the hidden layers' weight gradient and every workspace size do not see the dimension.  No per-point mask, frequency
//           gradient or pose gradient at DIM = 2: check_call refuses them.
//
// pose gradient (SININN_FLOWNET_POSEGRAD) after the whole backward of a points call: flownet_posegrad_kernel contracts
//           dE = dh1 W1 (the GEMM of the frequency gradient, for every encoding) with the analytic derivative of the encoding over the
//           FEATURES of each point: g_poses [N][3].  A tile owns its points: no partial sums in memory, no atomics, a fixed order.  DESIGN 14.8
//           SPATIAL (POSEGRAD | SPATIAL): a per-point mask cannot be folded into the packed W1, so the pack is
//           unmasked and the kernel multiplies dE[p][k] by m_k(p) after the GEMM, and the coordinate column's sum by m_d(p), from the corner
//           tile staged once per tile.  The mask is a CONSTANT of the point: the reference interpolates it under no_grad
//           (progressive_controller.py:655-680), so there is no d mask / d pose term.  DESIGN 14.9
//
// positional encoding (PE / PPE, PEModel model.py:472-487, PPEModel model.py:607-611): layer 1 has LIVE (LIVE + 3) inputs, fewer than
//           its padded K width KW; features LIVE .. KW - 1 are exact zeros from encode4.  Plain PE reads W1 [256][LIVE] in place (96-byte
//           rows, the 16-byte loads of columns LIVE .. KW - 1 are replaced by zeros), two K steps; PPE packs mask * W1 into [256][KW] +
//           [256][4] like the other progressive networks and runs ceil(open / 16) K steps.  The layer-1 weight gradient is the NARROW
//           instantiation of flownet_wgrad_kernel: a block owns 128 hidden columns x the KW padded features (a wave 32 x 32), always all of
//           them, so nothing in it depends on k_active; flownet_reduce_l1_kernel writes nn.Linear's [256][LIVE] / [256][LIVE + 3] layout,
//           for PPE an exact +0 where the mask is zero or the column lies beyond k_active.
//
// spatially adaptive (StashedSpatialController, progressive_controller.py:461-710): the mask is a per-point one, m_k(p) = the trilinear
//           interpolation of a device grid G [res^3][515] at the point's coordinates (Spatial, corners_of, sample_cols).  It cannot be
//           folded into W1, so the SPATIAL instantiations multiply the generated operand instead: encode4 * m in the forward pass and in
//           the layer-1 weight gradient (the same function on the same inputs: the same bits), dE * m in the frequency gradient.  W1
//           [256][515] is read in place with dword-aligned 16-byte loads (rows of 2060 bytes), and so are the eight grid rows of a
//           point: a 64-point tile of one image row spans a few grid cells, a few dozen distinct rows of 2060 bytes that L2 serves
//           again and again; they are NOT staged in LDS, which two blocks per CU leave no room for.  What is staged
//           per tile is the 64 x (8 corner weights, 8 row offsets), 4 KiB, computed once per point by the first 64 threads.  k_active
//           cuts the K loop and the weight-gradient tiles as above: the grid is zero from there on, the operand e * 0.
#include "flownet_tile.h"
#include "spatial_cells.h"   // FN_DOM, FN_GW, Spatial, Corners, corners_of

namespace sininn {

namespace {

constexpr int FN_WT = 128;          // weight-gradient output tile (FN_WT x FN_WT per block)
constexpr int FN_WS = FN_WT + 16;   // floats per point row of a weight-gradient operand tile (4 rows x 16 lanes -> 64 banks)
constexpr int FN_CHUNK_ELEMS = 1 << 15;   // split over points: (number of chunks) x (output tiles) is about 512 blocks
constexpr size_t FN_WG_LDS = (size_t)(2 * FN_P * FN_WS) * sizeof(float);
constexpr int FN_FWD_MAX_BLOCKS = 2048;   // the forward launch: at most this many blocks, grid-stride over the 64-point tiles
constexpr int FN_CN = 16;           // spatial: floats per point of the corner tile in LDS: 8 weights, 8 row offsets
constexpr size_t FN_CN_LDS = (size_t)(FN_P * FN_CN) * sizeof(float);
// the dynamic LDS of each kernel mode, for every launch of it: the forward, chain and frequency-gradient kernels hold the hidden tile and
// a [64][4] tile, the weight gradient its two operand tiles and (PROG) the coordinate tile; SPATIAL adds the corner tile
constexpr size_t tile_lds(bool spatial) { return FN_LDS + (spatial ? FN_CN_LDS : 0); }
constexpr size_t wgrad_lds(bool prog, bool spatial) {
  return FN_WG_LDS + (prog ? (size_t)(FN_P * FN_CS) * sizeof(float) : 0) + (spatial ? FN_CN_LDS : 0);
}

// ---- the input of a layer as the kernels see it: LIVE features in a K range of KW.  Everything that depends on the encoding is here ----
template <int LIVE_, int KW_, bool ENC_B_ = false, bool FREQ_GRAD_ = false>
struct LayerInput {
  static constexpr int LIVE = LIVE_;                   // features that exist
  static constexpr int KW = KW_;                       // ... padded to whole 16-feature K steps: encode4 gives exact zeros from LIVE on
  static constexpr bool ENC_B = ENC_B_;                // the encoding reads enc_b
  static constexpr bool FREQ_GRAD = FREQ_GRAD_;        // the gradient with respect to enc_a exists
  static constexpr bool PLAIN = true;                  // the network without the coordinates and the mask exists (a row may say no)
  static constexpr bool PAIR = false;                  // the kernels exist for two coordinates per point as well (a row may say yes)
  static constexpr int KSTEPS = KW / 16;
  static constexpr int width(bool prog, int dim = FN_DOM) { return LIVE + (prog ? dim : 0); }   // enc_dim: a row of nn.Linear's W1
  static constexpr int w1_stride(bool prog) { return prog ? KW : LIVE; }         // a row of the W1 the forward reads: packed / in place
  static constexpr size_t PACK_FLOATS = (size_t)FN_HID * (KW + FN_CS);           // progressive: W1p [256][KW] and wc [256][4]
  // the weight gradient: a block owns 128 x KT outputs, a wave AT x AT accumulator tiles (wide: 64 x 64, narrow: 32 x 32)
  static constexpr bool NARROW = KW < FN_WT;
  static constexpr int KT = NARROW ? KW : FN_WT;
  static constexpr int AT = NARROW ? 2 : 4;
  static constexpr int CHUNK_KF = FN_WT * (KW / KT);   // wgrad_chunks' width: (chunks) x (2 KW / KT output tiles) is about 512 blocks
  static constexpr int part_stride(bool prog) { return FN_HID * KW + FN_HID + (prog ? FN_HID * FN_CS : 0); }   // one chunk's partial sums
};

template <int KIND> struct Enc;
template <> struct Enc<SININN_FLOWNET_RBF> : LayerInput<512, 512, true> {
  static constexpr const char* NAME = "RBF";
  static constexpr bool PAIR = true;
};
template <> struct Enc<SININN_FLOWNET_FOURIER> : LayerInput<512, 512, false, true> {
  static constexpr const char* NAME = "Fourier";
  static constexpr bool PAIR = true;
};
template <> struct Enc<SININN_FLOWNET_RBFG> : LayerInput<512, 512, true> {
  static constexpr const char* NAME = "RBFG";
  static constexpr bool PAIR = true;
};
// 4 frequencies x 3 coordinates x (cos, sin), padded to two K steps
template <> struct Enc<SININN_FLOWNET_PE> : LayerInput<24, 32> { static constexpr const char* NAME = "PE"; };
// the triangle wave of MPFF: the shape of the Fourier kind, no frequency gradient; the reference has the progressive network only, so the
// plain 512-wide form is refused and its kernels are not instantiated
template <> struct Enc<SININN_FLOWNET_PIECEWISE> : LayerInput<512, 512> {
  static constexpr const char* NAME = "PieceWise";
  static constexpr bool PLAIN = false;
};
using Hidden = LayerInput<FN_HID, FN_HID>;             // layers 2 and 3, for their weight gradient
constexpr int FN_KINDS[] = {SININN_FLOWNET_RBF, SININN_FLOWNET_FOURIER, SININN_FLOWNET_RBFG, SININN_FLOWNET_PE, SININN_FLOWNET_PIECEWISE};

// f(std::integral_constant<int, KIND>) for the run-time `encoding`; `otherwise` for a value that is no encoding of this library
template <class R, class F>
R for_kind(int encoding, R otherwise, F&& f) {
  switch (encoding) {
    case SININN_FLOWNET_RBF: return f(std::integral_constant<int, SININN_FLOWNET_RBF>{});
    case SININN_FLOWNET_FOURIER: return f(std::integral_constant<int, SININN_FLOWNET_FOURIER>{});
    case SININN_FLOWNET_RBFG: return f(std::integral_constant<int, SININN_FLOWNET_RBFG>{});
    case SININN_FLOWNET_PE: return f(std::integral_constant<int, SININN_FLOWNET_PE>{});
    case SININN_FLOWNET_PIECEWISE: return f(std::integral_constant<int, SININN_FLOWNET_PIECEWISE>{});
    default: return otherwise;
  }
}

struct FlowNetDev {
  int T, H, W, N, ntiles;
  float scale;
  const float *times, *ys, *xs;
  const float* poses;      // points mode: [N][3], the coordinates of point p; nullptr: the grid above
  const float *enc_a, *enc_b;
  const float* w[4];
  const float* b[4];
  float* flows;
  float* saved;            // [3][ntiles * 64][256] or nullptr (inference)
  const float* dflows;
  float* dh;               // [3][ntiles * 64][256]
  const float* wt;         // W2^T, W3^T
  float* part;             // partial sums
  const float* wc;         // progressive: coordinate columns of W1 times their mask, [256][4]
  int ksteps;              // progressive: 16-feature steps of the layer-1 K loop
  Spatial sp;
};

// ---- spatial: the per-point mask ----
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes at a dword-aligned address: rows of FN_GW floats
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void store_corners(float* cn, const Corners& o) {
  *reinterpret_cast<f32x4*>(cn) = (f32x4){o.w[0], o.w[1], o.w[2], o.w[3]};
  *reinterpret_cast<f32x4*>(cn + 4) = (f32x4){o.w[4], o.w[5], o.w[6], o.w[7]};
  *reinterpret_cast<i32x4*>(cn + 8) = (i32x4){o.row[0], o.row[1], o.row[2], o.row[3]};
  *reinterpret_cast<i32x4*>(cn + 12) = (i32x4){o.row[4], o.row[5], o.row[6], o.row[7]};
}

__device__ __forceinline__ Corners load_corners(const float* cn) {
  const f32x4 w0 = *reinterpret_cast<const f32x4*>(cn), w1 = *reinterpret_cast<const f32x4*>(cn + 4);
  const i32x4 r0 = *reinterpret_cast<const i32x4*>(cn + 8), r1 = *reinterpret_cast<const i32x4*>(cn + 12);
  return Corners{{w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]}, {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3]}};
}

// m[j] = sum_c w_c G[row_c][col + j], corners in index order, a rounded product and a rounded sum each: the one place the mask is
// computed, so the forward pass, both gradients and sample_mask see the same bits
template <int NC>
__device__ __forceinline__ void sample_cols(const float* grid, const Corners& cn, int col, float (&m)[NC]) {
#pragma clang fp contract(off)
  static_assert(NC == 1 || NC == 2 || NC == 4, "one, two or four columns");
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float* g = grid + cn.row[c] + col;
    float v[NC];
    if constexpr (NC == 4) {
      const f32x4u t = *reinterpret_cast<const f32x4u*>(g);
      v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else if constexpr (NC == 2) {
      const f32x2u t = *reinterpret_cast<const f32x2u*>(g);
      v[0] = t[0]; v[1] = t[1];
    } else {
      v[0] = g[0];
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const float t = cn.w[c] * v[j];
      m[j] = c ? m[j] + t : t;
    }
  }
}

__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// the first 64 threads: the corners of the tile's points -> LDS
__device__ __forceinline__ void stage_corners(const FlowNetDev& q, int tile, int tid, float* cns) {
  if (tid < FN_P) store_corners(cns + tid * FN_CN, corners_of(q.sp, point_coord(q, tile * FN_P + tid)));
}

// the three masked coordinates of a point, as layer 1 reads them
__device__ __forceinline__ f32x4 masked_coord(const FlowNetDev& q, const Coord c, const Corners& cn) {
  float m0[1], m1[1], m2[1];
  sample_cols<1>(q.sp.grid, cn, 0, m0);
  sample_cols<1>(q.sp.grid, cn, 1, m1);
  sample_cols<1>(q.sp.grid, cn, 2, m2);
  return (f32x4){mul_rn(c.t, m0[0]), mul_rn(c.y, m1[0]), mul_rn(c.x, m2[0]), 0.f};
}



// sin / cos of 2 pi (c . f) for one frequency f = (fa, fb, fc).  The phase is kept in REVOLUTIONS: each product is split into its
// rounded value and its exact rounding error, the rounded value is reduced to [-1/2, 1/2] exactly, so the phase of a 75-cycle
// frequency is as good as that of a slow one; sincospi does the rest
__device__ __forceinline__ void fourier_sincos(const Coord c, float fa, float fb, float fc, float& s, float& co) {
  const float p0 = c.t * fa, p1 = c.y * fb, p2 = c.x * fc;
  const float e = fmaf(c.t, fa, -p0) + fmaf(c.y, fb, -p1) + fmaf(c.x, fc, -p2);
  const float r = ((p0 - rintf(p0)) + (p1 - rintf(p1)) + (p2 - rintf(p2))) + e;
  sincospif(2.f * r, &s, &co);
}

// two coordinates (domain_dim = 2): the same phase from the two products the reference's (y, x) @ frequencies [2][256] has
__device__ __forceinline__ void fourier_sincos2(const Coord c, float fb, float fc, float& s, float& co) {
  const float p1 = c.y * fb, p2 = c.x * fc;
  const float e = fmaf(c.y, fb, -p1) + fmaf(c.x, fc, -p2);
  const float r = ((p1 - rintf(p1)) + (p2 - rintf(p2))) + e;
  sincospif(2.f * r, &s, &co);
}

// the piecewise-linear kind (model.py:638-644).  piecewise_arg: u = (c + 1) . f for one frequency f = (fa, fb, fc), each c_d + 1 rounded
// as the reference rounds it before its matmul; explicit fmaf, for the reason recorded at the RBF branch below.  piecewise_rem:
// r = fmod(w, 2) - 1 with torch.fmod's truncation (the sign follows the dividend, NOT the floor-mod of the RBFG branch):
// w - 2 trunc(w / 2) is exact in fp32, the quotient's integer part is exact and the difference lies on w's own grid.  The feature is
// 2 r + 1 where r < 0, else 1 - 2 r; for w < 0 that is the reference's value in (-5, -1], jumps at the negative integers included.
// encode4 and FeatureGrad4 call these and take the same branch on the same r
__device__ __forceinline__ float piecewise_arg(const Coord c, float fa, float fb, float fc) {
  const float xt = c.t + 1.f, xy = c.y + 1.f, xx = c.x + 1.f;
  return fmaf(xx, fc, fmaf(xy, fb, xt * fa));
}

__device__ __forceinline__ float piecewise_rem(float w) { return fmaf(-2.f, truncf(0.5f * w), w) - 1.f; }

__device__ __forceinline__ float piecewise_tri(float w) {
  const float r = piecewise_rem(w);
  return r < 0.f ? fmaf(2.f, r, 1.f) : fmaf(-2.f, r, 1.f);
}

// features f0 .. f0 + 3 (f0 % 4 == 0) of one point
// DIM = 2 (RBF, Fourier, RBFG): the parameters have the reference's two-coordinate layouts, centres [512][2], frequencies [2][256], offsets
// [256][2], and every expression its two terms (y, x); c.t is not read.  The t term is ABSENT, not fed as zero: in RBFG a zero t would not
// drop out, (0 mod p) 2 - p = -p
template <int KIND, int DIM = 3>
__device__ __forceinline__ f32x4 encode4(const FlowNetDev& q, const Coord c, int f0) {
  static_assert(DIM == 3 || (DIM == 2 && Enc<KIND>::PAIR), "two coordinates: RBF, Fourier and RBFG");
  f32x4 o;
  if constexpr (DIM == 2 && KIND == SININN_FLOWNET_RBF) {
    const f32x4* cp = reinterpret_cast<const f32x4*>(q.enc_a + 2 * f0);   // centres [512][2]
    const f32x4 c0 = cp[0], c1 = cp[1];
    const f32x4 sg = *reinterpret_cast<const f32x4*>(q.enc_b + f0);
    const float cc[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dy = c.y - cc[2 * j], dx = c.x - cc[2 * j + 1];
      const float d = fmaf(dx, dx, dy * dy);                               // explicit fmaf, for the reason recorded below
      o[j] = expf(-(d * (sg[j] * sg[j])));
    }
  } else if constexpr (DIM == 2 && KIND == SININN_FLOWNET_RBFG) {
    const int f = f0 >> 1;                                                 // offsets [256][2], sigma [256]
    const f32x4 ov = *reinterpret_cast<const f32x4*>(q.enc_a + 2 * f);
    const f32x2 sg = *reinterpret_cast<const f32x2*>(q.enc_b + f);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float is = 1.f / sg[u], p = 2.f * is, hp = 0.5f * sg[u], s2 = sg[u] * sg[u];
      const float xa[2] = {c.y + ov[2 * u], c.x + ov[2 * u + 1]};
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        float w[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const float x = v ? xa[d] + is : xa[d];
          const float r = fmaf(-floorf(x * hp), p, x);                     // Python's remainder, as below
          w[d] = fmaf(r, 2.f, -p);
        }
        const float d = fmaf(w[1], w[1], w[0] * w[0]);
        o[2 * u + v] = fmaf(expf(-(d * s2)), 2.f, -1.f);
      }
    }
  } else if constexpr (DIM == 2) {
    const int f = f0 >> 1;                                                 // frequencies [2][256]
    const f32x2 fb = *reinterpret_cast<const f32x2*>(q.enc_a + f);
    const f32x2 fc = *reinterpret_cast<const f32x2*>(q.enc_a + 256 + f);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float s, co;
      fourier_sincos2(c, fb[u], fc[u], s, co);
      o[2 * u] = s;
      o[2 * u + 1] = co;
    }
  } else if constexpr (KIND == SININN_FLOWNET_RBF) {
    const f32x4* cp = reinterpret_cast<const f32x4*>(q.enc_a + 3 * f0);   // centres [512][3]
    const f32x4 c0 = cp[0], c1 = cp[1], c2 = cp[2];
    const f32x4 sg = *reinterpret_cast<const f32x4*>(q.enc_b + f0);
    const float cc[12] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3], c2[0], c2[1], c2[2], c2[3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dt = c.t - cc[3 * j], dy = c.y - cc[3 * j + 1], dx = c.x - cc[3 * j + 2];
      // explicit fmaf: left to the compiler, the contraction of this sum differed between the unrolled copies of one call site
      // (mul, mul, mul, add, add for one point of the forward's four, mul, fma, add for the others), so the same point gave
      // different bits in different rows of a tile and the weight gradient did not see the forward's encoding
      const float d = fmaf(dx, dx, fmaf(dy, dy, dt * dt));
      o[j] = expf(-(d * (sg[j] * sg[j])));
    }
  } else if constexpr (KIND == SININN_FLOWNET_RBFG) {
    const int f = f0 >> 1;                                                 // offsets [256][3], sigma [256]
    const f32x2* op = reinterpret_cast<const f32x2*>(q.enc_a + 3 * f);
    const f32x2 o0 = op[0], o1 = op[1], o2 = op[2];
    const f32x2 sg = *reinterpret_cast<const f32x2*>(q.enc_b + f);
    const float off[6] = {o0[0], o0[1], o1[0], o1[1], o2[0], o2[1]};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      // one division per frequency: 2 * (1 / sigma) is 2 / sigma to the bit, sigma / 2 is exact
      const float is = 1.f / sg[u], p = 2.f * is, hp = 0.5f * sg[u], s2 = sg[u] * sg[u];
      const float xa[3] = {c.t + off[3 * u], c.y + off[3 * u + 1], c.x + off[3 * u + 2]};
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        float w[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float x = v ? xa[d] + is : xa[d];
          // Python's remainder, x - floor(x / p) p: the fma rounds once, like fmod's exact result plus p for a negative x.  A
          // quotient that rounds across an integer leaves r one period off, next to 0 or p, where (2 r - p)^2 is continuous
          const float r = fmaf(-floorf(x * hp), p, x);
          w[d] = fmaf(r, 2.f, -p);
        }
        // explicit fmaf, as above: the forward and the weight gradient must see the same bits
        const float d = fmaf(w[2], w[2], fmaf(w[1], w[1], w[0] * w[0]));
        o[2 * u + v] = fmaf(expf(-(d * s2)), 2.f, -1.f);
      }
    }
  } else if constexpr (KIND == SININN_FLOWNET_PE) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = f0 + j;                                                // freqs [4]; 6 f + d: cos, 6 f + 3 + d: sin
      float v = 0.f;
      if (k < Enc<KIND>::LIVE) {
        const int f = k / 6, r = k - 6 * f, d = r < 3 ? r : r - 3;
        const float xd = d == 0 ? c.t : d == 1 ? c.y : c.x;
        // one rounded product, as torch's einsum makes it, never contracted; the accurate full-range sine and cosine
        float sn, co;
        sincosf(__fmul_rn(q.enc_a[f], xd), &sn, &co);
        v = r < 3 ? co : sn;
      }
      o[j] = v;
    }
  } else if constexpr (KIND == SININN_FLOWNET_PIECEWISE) {
    const int f = f0 >> 1;                                                 // frequencies [3][256]
    const f32x2 fa = *reinterpret_cast<const f32x2*>(q.enc_a + f);
    const f32x2 fb = *reinterpret_cast<const f32x2*>(q.enc_a + 256 + f);
    const f32x2 fc = *reinterpret_cast<const f32x2*>(q.enc_a + 512 + f);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float w = piecewise_arg(c, fa[u], fb[u], fc[u]);
      o[2 * u] = piecewise_tri(w);
      o[2 * u + 1] = piecewise_tri(w + 1.f);
    }
  } else {
    const int f = f0 >> 1;                                                 // frequencies [3][256]
    const f32x2 fa = *reinterpret_cast<const f32x2*>(q.enc_a + f);
    const f32x2 fb = *reinterpret_cast<const f32x2*>(q.enc_a + 256 + f);
    const f32x2 fc = *reinterpret_cast<const f32x2*>(q.enc_a + 512 + f);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float s, co;
      fourier_sincos(c, fa[u], fb[u], fc[u], s, co);
      o[2 * u] = s;
      o[2 * u + 1] = co;
    }
  }
  return o;
}



// the chain kernel's plain store: acc + 0.f, which turns a -0 into +0.  flownet_tile.h's Plain stores the accumulator as it is; this kernel
// keeps the sum it has always made, its instructions and its bits
struct PlainAddZero {
  __device__ __forceinline__ float col(int) const { return 0.f; }
  __device__ __forceinline__ float operator()(float v, float bq) const { return v + bq; }
};

// PROG: q.w[0] is the packed W1p [256][KW], q.wc the coordinate columns, q.ksteps the length of the K loop
// SPATIAL (with PROG): q.w[0] is nn.Linear's own W1 [256][FN_GW], the operand is multiplied by the point's mask, q.ksteps as above
// DIM = 2: two coordinates per point (point_coord_dim, encode4<KIND, 2>); PROG: the coordinate K group is y, x, 0, 0 and q.wc holds the
// two coordinate columns of W1 [256][514] and two zero columns
template <int KIND, bool PROG = false, bool SPATIAL = false, int DIM = 3>
__global__ __launch_bounds__(FN_NTHR, 2) void flownet_fwd_kernel(FlowNetDev q) {
  static_assert(PROG || !SPATIAL, "a spatial mask is a progressive network's");
  static_assert(DIM == 3 || !SPATIAL, "per-point masks are a grid over (t, y, x)");
  using E = Enc<KIND>;
  constexpr int EW = SPATIAL ? FN_GW : E::w1_stride(PROG);   // floats per row of q.w[0]
  extern __shared__ __attribute__((aligned(16))) float fn_smem[];
  float* const hs = fn_smem;
  float* const cns = fn_smem + FN_P * FN_HS + FN_P * FN_OUT;   // SPATIAL: [64][FN_CN]
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kq = lane >> 4;
  const int cw = wave * 64;
  const size_t lstride = (size_t)q.ntiles * FN_P * FN_HID;
  const int hw = q.H * q.W;

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    Coord pc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) pc[m] = point_coord_dim<DIM>(q, tile * FN_P + 16 * m + li);

    f32x4 acc[4][4];
    zero_acc(acc);
    if constexpr (SPATIAL) {
      stage_corners(q, tile, tid, cns);                // the last reads of the previous tile's lie before its barriers
      __syncthreads();
    }
    if constexpr (PROG) {
      // ---- the coordinates: one K group, k = kq: t, y, x, 0 ----
      float a[4], b[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if constexpr (DIM == 3) a[m] = kq == 0 ? pc[m].t : kq == 1 ? pc[m].y : kq == 2 ? pc[m].x : 0.f;
        else a[m] = kq == 0 ? pc[m].y : kq == 1 ? pc[m].x : 0.f;
      }
      if constexpr (SPATIAL) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          float mk[1];
          sample_cols<1>(q.sp.grid, load_corners(cns + (16 * m + li) * FN_CN), kq < FN_DOM ? kq : 0, mk);
          a[m] = kq < FN_DOM ? mul_rn(a[m], mk[0]) : 0.f;
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) b[n] = kq < FN_DOM ? q.w[0][(size_t)(cw + 16 * n + li) * FN_GW + kq] : 0.f;
      } else {
#pragma unroll
        for (int n = 0; n < 4; ++n) b[n] = q.wc[(cw + 16 * n + li) * FN_CS + kq];
      }
      mfma_k4(a, b, acc);
    }
    // ---- layer 1: the A fragment is generated, never stored ----
    const int ksteps = PROG ? q.ksteps : E::KSTEPS;
#pragma unroll 1
    for (int s = 0; s < ksteps; ++s) {
      f32x4 bf[4], af[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        if (!PROG && E::LIVE < E::KW && 16 * s + 4 * kq >= E::LIVE) bf[n] = (f32x4){0.f, 0.f, 0.f, 0.f};   // W1 [256][LIVE] has no such columns
        else if constexpr (SPATIAL) bf[n] = *reinterpret_cast<const f32x4u*>(q.w[0] + (size_t)(cw + 16 * n + li) * EW + FN_DOM + 16 * s + 4 * kq);
        else bf[n] = *reinterpret_cast<const f32x4*>(q.w[0] + (size_t)(cw + 16 * n + li) * EW + 16 * s + 4 * kq);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        af[m] = encode4<KIND, DIM>(q, pc[m], 16 * s + 4 * kq);
        if constexpr (SPATIAL) {
          float mk[4];
          sample_cols<4>(q.sp.grid, load_corners(cns + (16 * m + li) * FN_CN), FN_DOM + 16 * s + 4 * kq, mk);
#pragma unroll
          for (int j = 0; j < 4; ++j) af[m][j] = mul_rn(af[m][j], mk[j]);
          __builtin_amdgcn_sched_barrier(0);           // one point's eight grid rows in flight at a time: 32 registers, not 128
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m][j], bf[n][j], acc[m][n], 0, 0, 0);
    }
    __syncthreads();                       // the previous tile's layer 4 has read hs
    store_acc(hs, cw, li, kq, acc, BiasRelu{q.b[0]});
    __syncthreads();
    if (q.saved) copy_tile_out(hs, q.saved, tile, tid);
    // ---- layers 2 and 3 ----
#pragma unroll 1
    for (int l = 1; l < 3; ++l) {
      zero_acc(acc);
      gemm_lds(hs, q.w[l], cw, li, kq, acc);
      __syncthreads();                     // every wave has read the whole tile (and copied it out)
      store_acc(hs, cw, li, kq, acc, BiasRelu{q.b[l]});
      __syncthreads();
      if (q.saved) copy_tile_out(hs, q.saved + l * lstride, tile, tid);
    }
    // ---- layer 4 on the vector ALU: thread = (channel tid / 64, point tid % 64) ----
    {
      const int c = tid >> 6, pl = tid & 63;
      const float* w4 = q.w[3] + c * FN_HID;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
      for (int k = 0; k < FN_HID; k += 4) {
        const f32x4 h = *reinterpret_cast<const f32x4*>(hs + pl * FN_HS + k);
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w4 + k);
        a0 = fmaf(h[0], wv[0], a0);
        a1 = fmaf(h[1], wv[1], a1);
        a2 = fmaf(h[2], wv[2], a2);
        a3 = fmaf(h[3], wv[3], a3);
      }
      const int p = tile * FN_P + pl;
      if (p < q.N) {
        const int t = p / hw, rem = p - t * hw;
        q.flows[((size_t)t * FN_OUT + c) * hw + rem] = (((a0 + a1) + (a2 + a3)) + q.b[3][c]) * q.scale;
      }
    }
  }
}

// out[k][j] = in[j][k] for W2 and W3 (blockIdx.y): the data-gradient GEMMs then read 16-byte rows like the forward pass does
__global__ __launch_bounds__(FN_NTHR) void flownet_transpose_kernel(const float* w2, const float* w3, float* wt) {
  const float* in = blockIdx.y ? w3 : w2;
  float* out = wt + (size_t)blockIdx.y * FN_HID * FN_HID;
  const int j = blockIdx.x, k = threadIdx.x;
  out[k * FN_HID + j] = in[j * FN_HID + k];
}

// progressive: w1p[j][k] = w1[j][3 + k] mask[3 + k] (k < 512), wc[j][c] = w1[j][c] mask[c] (c < 3), wc[j][3] = 0; block = row j.
// A closed feature gets an exact zero whatever the weight holds.  EW > LIVE (PE: w1 is [256][3 + LIVE], w1p [256][KW]): zeros from LIVE on.
// Instantiated as <E::KW, E::LIVE>: encodings of one shape share one kernel.  DOM = 2: w1 is [256][2 + LIVE], mask [2 + LIVE]; wc[j] =
// (w1[j][0] mask[0], w1[j][1] mask[1], 0, 0)
template <int EW, int LIVE, int DOM = FN_DOM>
__global__ __launch_bounds__(FN_NTHR) void flownet_pack_kernel(const float* w1, const float* mask, float* w1p, float* wc) {
  const int j = blockIdx.x, tid = threadIdx.x;
  const float* row = w1 + (size_t)j * (DOM + LIVE);
#pragma unroll
  for (int k = tid; k < EW; k += FN_NTHR) {
    float v = 0.f;
    if (k < LIVE) {
      const float m = mask[DOM + k];
      v = m == 0.f ? 0.f : row[DOM + k] * m;
    }
    w1p[(size_t)j * EW + k] = v;
  }
  if (tid < FN_CS) {
    float v = 0.f;
    if (tid < DOM) {
      const float m = mask[tid];
      v = m == 0.f ? 0.f : row[tid] * m;
    }
    wc[j * FN_CS + tid] = v;
  }
}

__global__ __launch_bounds__(FN_NTHR, 2) void flownet_bwd_chain_kernel(FlowNetDev q) {
  extern __shared__ __attribute__((aligned(16))) float fn_smem[];
  float* const hs = fn_smem;
  float* const dos = fn_smem + FN_P * FN_HS;           // [64][4]: dout of the tile
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kq = lane >> 4;
  const int cw = wave * 64;
  const size_t lstride = (size_t)q.ntiles * FN_P * FN_HID;
  const int hw = q.H * q.W;

  float w4k[4], gw4[4] = {0.f, 0.f, 0.f, 0.f};
  double gb4 = 0.0;                                    // four lanes, 64 terms per tile: a long sum of signed terms, kept in double
#pragma unroll
  for (int c = 0; c < 4; ++c) w4k[c] = q.w[3][c * FN_HID + tid];

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    __syncthreads();                                   // the previous tile is done with hs / dos
#pragma unroll 4
    for (int u = 0; u < FN_P * FN_HID / 4 / FN_NTHR; ++u) {
      const int f = tid + FN_NTHR * u;
      const int row = f >> 6, c4 = (f & 63) * 4;
      *reinterpret_cast<f32x4*>(hs + row * FN_HS + c4) =
          *reinterpret_cast<const f32x4*>(q.saved + 2 * lstride + ((size_t)tile * FN_P + row) * FN_HID + c4);
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
    __syncthreads();
    // gW4 += dout^T h3;  dh3 = (dout W4) . [h3 > 0] in place: thread = hidden column tid
#pragma unroll 4
    for (int p = 0; p < FN_P; ++p) {
      const f32x4 d = *reinterpret_cast<const f32x4*>(dos + p * FN_OUT);
      const float h = hs[p * FN_HS + tid];
      float v = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        gw4[c] = fmaf(d[c], h, gw4[c]);
        v = fmaf(d[c], w4k[c], v);
      }
      hs[p * FN_HS + tid] = h > 0.f ? v : 0.f;
    }
    if (tid < FN_OUT) {
      double s = 0.0;
      for (int p = 0; p < FN_P; ++p) s += (double)dos[p * FN_OUT + tid];
      gb4 += s;
    }
    __syncthreads();
    copy_tile_out(hs, q.dh + 2 * lstride, tile, tid);
    // dh2 = (dh3 W3) . [h2 > 0], dh1 = (dh2 W2) . [h1 > 0]
#pragma unroll 1
    for (int l = 1; l >= 0; --l) {
      f32x4 acc[4][4];
      zero_acc(acc);
      gemm_lds(hs, q.wt + (size_t)l * FN_HID * FN_HID, cw, li, kq, acc);
      __syncthreads();
      store_acc(hs, cw, li, kq, acc, PlainAddZero{});
      __syncthreads();
#pragma unroll 4
      for (int u = 0; u < FN_P * FN_HID / 4 / FN_NTHR; ++u) {
        const int f = tid + FN_NTHR * u;
        const int row = f >> 6, c4 = (f & 63) * 4;
        const size_t g = ((size_t)tile * FN_P + row) * FN_HID + c4;
        const f32x4 h = *reinterpret_cast<const f32x4*>(q.saved + l * lstride + g);
        f32x4 v = *reinterpret_cast<const f32x4*>(hs + row * FN_HS + c4);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = h[j] > 0.f ? v[j] : 0.f;
        *reinterpret_cast<f32x4*>(q.dh + l * lstride + g) = v;
        if (l) *reinterpret_cast<f32x4*>(hs + row * FN_HS + c4) = v;
      }
      __syncthreads();
    }
  }
  float* const out = q.part + (size_t)blockIdx.x * (FN_OUT * FN_HID + FN_OUT);
#pragma unroll
  for (int c = 0; c < 4; ++c) out[c * FN_HID + tid] = gw4[c];
  if (tid < FN_OUT) out[FN_OUT * FN_HID + tid] = (float)gb4;
}

// part[chunk][j][k] = sum over the chunk's point tiles of dh[p][j] in[p][k]  (+ [chunk][256 * KF + j] = sum_p dh[p][j]);
// grid = (2 * KF / KT output tiles, chunks); ENC: in = the encoding (KF = Enc<KIND>::KW), else a saved hidden layer (KF = 256, KIND unused).
// PROG (with ENC): + [chunk][256 * KF + 256 + 4 j + c] = sum_p dh[p][j] coordinate_c[p]; the grid may cover the leading k tiles only.
// NARROW (an encoding of fewer than 128 padded features): grid = (2, chunks), a block owns 128 x KF and a wave 32 x 32 of it
// SPATIAL (with PROG): the input is times the point's mask, as the forward pass made it, the coordinates included
// DIM = 2 (with ENC): two coordinates per point; PROG: the coordinate sums are two, [chunk][256 * KF + 256 + 4 j + c], c = 0: y, 1: x
template <int KIND, bool ENC, bool PROG = false, bool SPATIAL = false, int DIM = 3>
__global__ __launch_bounds__(FN_NTHR, 2) void flownet_wgrad_kernel(FlowNetDev q, const float* dh, const float* in) {
  static_assert(ENC || !PROG, "the progressive weight gradient is layer 1's");
  static_assert(DIM == 3 || (ENC && !SPATIAL), "two coordinates: layer 1 under a global mask or none");
  static_assert(PROG || !SPATIAL, "a spatial mask is a progressive network's");
  using L = std::conditional_t<ENC, Enc<KIND>, Hidden>;
  constexpr bool NARROW = L::NARROW;
  constexpr int KF = L::KW;
  constexpr int KT = L::KT;                            // input columns of a block
  constexpr int MT = L::AT, NT = L::AT;                // 16 x 16 accumulator tiles of a wave
  constexpr int PSTRIDE = L::part_stride(PROG);
  constexpr int NU = FN_P * FN_WT / 4 / FN_NTHR;       // 16-byte units per thread and operand tile
  constexpr int NUB = FN_P * KT / 4 / FN_NTHR;         // ... of the input tile
  extern __shared__ __attribute__((aligned(16))) float fn_smem[];
  float* const as = fn_smem;                           // [64][FN_WS]: dh tile
  float* const bs = fn_smem + FN_P * FN_WS;            // [64][FN_WS]: input tile
  float* const cs = fn_smem + 2 * FN_P * FN_WS;        // PROG: [64][4]: coordinates of the tile's points
  float* const cns = cs + FN_P * FN_CS;                // SPATIAL: [64][FN_CN]: their corners
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kq = lane >> 4;
  const int j0 = (blockIdx.x & 1) * FN_WT, k0 = (blockIdx.x >> 1) * KT;
  const int jw = NARROW ? wave * 32 : (wave & 1) * 64, kw = NARROW ? 0 : (wave >> 1) * 64;
  const int chunk = blockIdx.y, nchunks = gridDim.y;

  f32x4 acc[MT][NT];
  zero_acc(acc);
  float bsum = 0.f;
  float csum[FN_DOM] = {0.f, 0.f, 0.f};
  f32x4 va[NU], vb[NU];
  auto fetch = [&](int tile) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int f = tid + FN_NTHR * u;
      const int row = f >> 5, c4 = (f & 31) * 4;
      const size_t g = ((size_t)tile * FN_P + row) * FN_HID;
      va[u] = *reinterpret_cast<const f32x4*>(dh + g + j0 + c4);
      if constexpr (!ENC) vb[u] = *reinterpret_cast<const f32x4*>(in + g + k0 + c4);
    }
  };
  if (chunk < q.ntiles) fetch(chunk);
  for (int tile = chunk; tile < q.ntiles; tile += nchunks) {
    __syncthreads();                                   // the previous tile's MFMAs have read as / bs
    if constexpr (SPATIAL) {
      if (tid < FN_P) {
        const Coord c = point_coord(q, tile * FN_P + tid);
        const Corners cn = corners_of(q.sp, c);
        store_corners(cns + tid * FN_CN, cn);
        if (k0 == 0) *reinterpret_cast<f32x4*>(cs + tid * FN_CS) = masked_coord(q, c, cn);
      }
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int f = tid + FN_NTHR * u;
      const int row = f >> 5, c4 = (f & 31) * 4;
      *reinterpret_cast<f32x4*>(as + row * FN_WS + c4) = va[u];
      if (u < NUB) {
        const int rb = NARROW ? f / (KT / 4) : row, cb = NARROW ? (f % (KT / 4)) * 4 : c4;
        if constexpr (ENC) vb[u] = encode4<KIND, DIM>(q, point_coord_dim<DIM>(q, tile * FN_P + rb), k0 + cb);
        if constexpr (SPATIAL) {
          float mk[4];
          sample_cols<4>(q.sp.grid, load_corners(cns + rb * FN_CN), FN_DOM + k0 + cb, mk);
#pragma unroll
          for (int j = 0; j < 4; ++j) vb[u][j] = mul_rn(vb[u][j], mk[j]);
        }
        *reinterpret_cast<f32x4*>(bs + rb * FN_WS + cb) = vb[u];
      }
    }
    if constexpr (PROG && !SPATIAL) {
      if (k0 == 0 && tid < FN_P) stage_coord_dim<DIM>(q, cs, tile, tid);
    }
    __syncthreads();
    if (tile + nchunks < q.ntiles) fetch(tile + nchunks);
    if (k0 == 0 && tid < FN_WT) {
      float s = 0.f;
      if constexpr (PROG) {
        float st = 0.f, sy = 0.f, sx = 0.f;
#pragma unroll 8
        for (int p = 0; p < FN_P; ++p) {
          const float d = as[p * FN_WS + tid];
          const f32x4 c = *reinterpret_cast<const f32x4*>(cs + p * FN_CS);
          s += d;
          st = fmaf(d, c[0], st);
          sy = fmaf(d, c[1], sy);
          if constexpr (DIM == 3) sx = fmaf(d, c[2], sx);                // DIM = 2: the tile's columns are y, x, 0, 0
        }
        csum[0] += st;
        csum[1] += sy;
        csum[2] += sx;
      } else {
#pragma unroll 8
        for (int p = 0; p < FN_P; ++p) s += as[p * FN_WS + tid];
      }
      bsum += s;
    }
#pragma unroll 2
    for (int ks = 0; ks < FN_P / 4; ++ks) {
      float a[MT], b[NT];
#pragma unroll
      for (int m = 0; m < MT; ++m) a[m] = as[(4 * ks + kq) * FN_WS + jw + 16 * m + li];
#pragma unroll
      for (int n = 0; n < NT; ++n) b[n] = bs[(4 * ks + kq) * FN_WS + kw + 16 * n + li];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[n], acc[m][n], 0, 0, 0);
    }
  }
  float* const out = q.part + (size_t)chunk * PSTRIDE;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)(j0 + jw + 16 * m + 4 * kq + r) * KF + k0 + kw + 16 * n + li] = acc[m][n][r];
  if (k0 == 0 && tid < FN_WT) out[FN_HID * KF + j0 + tid] = bsum;
  if constexpr (PROG) {
    if (k0 == 0 && tid < FN_WT)
      *reinterpret_cast<f32x4*>(out + FN_HID * KF + FN_HID + (j0 + tid) * FN_CS) = (f32x4){csum[0], csum[1], csum[2], 0.f};
  }
}

// gw[i] = sum_c part[c][i] (i < nw), gb[i - nw] = sum_c part[c][i] (nw <= i < nw + nb): chunks in index order, always.  The bias
// sums (nb entries, up to 512 signed terms that largely cancel) are added in double and rounded once; the weights stay in fp32
__global__ __launch_bounds__(FN_NTHR) void flownet_reduce_kernel(const float* part, int nparts, int nw, int nb, float* gw, float* gb) {
  const int i = blockIdx.x * FN_NTHR + threadIdx.x;
  if (i >= nw + nb) return;
  const size_t stride = (size_t)nw + nb;
  if (i < nw) {
    float s = 0.f;
    for (int c = 0; c < nparts; ++c) s += part[c * stride + i];
    gw[i] = s;
  } else {
    double s = 0.0;
    for (int c = 0; c < nparts; ++c) s += (double)part[c * stride + i];
    gb[i - nw] = (float)s;
  }
}

// progressive layer 1: gw [256][515] = mask[k] * sum_c part[c][..] in chunk order (k < 3: the coordinate sums, else encoded column
// k - 3), an exact zero where the mask is zero or the column lies beyond the `kcols` encoded columns that were computed; gb as above.
// mask == nullptr (spatial: the mask is in the partial sums already): the sums as they are, zeros beyond `kcols`.
// EW: columns of a row of the partial sums, LIVE: encoded columns of gw (<E::KW, E::LIVE>).  !PROG (PE): gw [256][LIVE], no mask
// DOMAIN = 2: gw [256][2 + LIVE], the coordinate sums are entries 0 and 1 of a row's four
template <int EW, int LIVE, bool PROG, int DOMAIN = FN_DOM>
__global__ __launch_bounds__(FN_NTHR) void flownet_reduce_l1_kernel(const float* part, int nparts, const float* mask, int kcols, float* gw,
                                                                    float* gb) {
  constexpr int DOM = PROG ? DOMAIN : 0;
  constexpr int WIDTH = DOM + LIVE;
  constexpr int NW = FN_HID * WIDTH;
  constexpr size_t STRIDE = LayerInput<LIVE, EW>::part_stride(PROG);
  const int i = blockIdx.x * FN_NTHR + threadIdx.x;
  if (i >= NW + FN_HID) return;
  size_t src;
  float m = 1.f;
  if (i < NW) {
    const int j = i / WIDTH, k = i - j * WIDTH;
    if constexpr (PROG) {
      if (mask) m = mask[k];
      if (m == 0.f || k - DOM >= kcols) { gw[i] = 0.f; return; }
    }
    src = k < DOM ? (size_t)FN_HID * EW + FN_HID + j * FN_CS + k : (size_t)j * EW + (k - DOM);
  } else {
    src = (size_t)FN_HID * EW + (i - NW);
  }
  float s = 0.f;
  for (int c = 0; c < nparts; ++c) s += part[c * STRIDE + src];
  if (i < NW) gw[i] = s * m;
  else gb[i - NW] = s;
}

// ---- gradient with respect to the Fourier frequencies (the learnable encodings RFF / PRFF) ----
// dE[p][k] = sum_j dh1[p][j] W1[j][k] is one more data-gradient GEMM through layer 1, contracted over the 256 hidden columns with the
// forward's LDS loop on a transposed W1; dE lives in the accumulators only.  Row c of that transposed matrix is CHOSEN: pass c / 256,
// wave (c / 64) % 4, accumulator column block n = (c / 16) % 4, lane c % 16 holds feature 2 f + n / 2 of frequency
// f = 128 pass + 32 wave + 16 (n % 2) + lane, so a lane's accumulators n and n + 2 are the sin and the cos coefficient of ONE frequency
// for the same 16 points and dphi = dE_sin cos(phi) - dE_cos sin(phi) needs no lane movement.
using Fourier = Enc<SININN_FLOWNET_FOURIER>;
constexpr int FN_NF = Fourier::LIVE / 2;             // frequencies
constexpr int FN_EG_PART = FN_DOM * FN_NF;           // floats of one block's partial sums, [3][256]
constexpr size_t FN_EG_FLOATS = (size_t)Fourier::LIVE * FN_HID + (size_t)FN_CHAIN_MAX_BLOCKS * FN_EG_PART;
constexpr float FN_TWO_PI = 6.283185307179586f;

// wt[c][j] = w1[j][feature of row c] (progressive: column 3 + feature, times its mask, an exact zero where the mask is zero; spatial:
// column 3 + feature as it is, the kernel applies the mask to dE); block = row c
__global__ __launch_bounds__(FN_NTHR) void flownet_encgrad_pack_kernel(const float* w1, const float* mask, float* wt, int spatial) {
  const int c = blockIdx.x, j = threadIdx.x;
  const int f = (c >> 8) * 128 + ((c >> 6) & 3) * 32 + ((c >> 4) & 1) * 16 + (c & 15);
  const int k = 2 * f + ((c >> 5) & 1);
  float v;
  if (spatial) {
    v = w1[(size_t)j * Fourier::width(true) + FN_DOM + k];
  } else if (mask) {
    const float m = mask[FN_DOM + k];
    v = m == 0.f ? 0.f : w1[(size_t)j * Fourier::width(true) + FN_DOM + k] * m;
  } else {
    v = w1[(size_t)j * Fourier::width(false) + k];
  }
  wt[(size_t)c * FN_HID + j] = v;
}

// part[block][d][f] = sum over the block's point tiles of coordinate_d[p] dphi[p][f]; grid-stride over tiles like the chain kernel.
// Frequencies from `fopen` on are closed (progressive): a wave whose 32 frequencies are all closed skips its GEMM and leaves zeros.
// SPATIAL: wt is unmasked and dE[p][k] is multiplied by the point's mask of feature k
template <bool SPATIAL>
__global__ __launch_bounds__(FN_NTHR, 2) void flownet_encgrad_kernel(FlowNetDev q, const float* wt, float* part, int fopen) {
  extern __shared__ __attribute__((aligned(16))) float fn_smem[];
  float* const hs = fn_smem;                           // [64][FN_HS]: dh1 tile
  float* const cs = fn_smem + FN_P * FN_HS;            // [64][4]: coordinates of the tile's points
  float* const cns = cs + FN_P * FN_CS;                // SPATIAL: [64][FN_CN]: their corners
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kq = lane >> 4;
  const int cw = wave * 64;

  float g[2][2][FN_DOM];
#pragma unroll
  for (int u = 0; u < 4 * FN_DOM; ++u) (&g[0][0][0])[u] = 0.f;

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    __syncthreads();                                   // the previous tile is done with hs / cs
#pragma unroll 4
    for (int u = 0; u < FN_P * FN_HID / 4 / FN_NTHR; ++u) {
      const int f = tid + FN_NTHR * u;
      const int row = f >> 6, c4 = (f & 63) * 4;
      *reinterpret_cast<f32x4*>(hs + row * FN_HS + c4) = *reinterpret_cast<const f32x4*>(q.dh + ((size_t)tile * FN_P + row) * FN_HID + c4);
    }
    if (tid < FN_P) {
      const Coord c = point_coord(q, tile * FN_P + tid);
      *reinterpret_cast<f32x4*>(cs + tid * FN_CS) = (f32x4){c.t, c.y, c.x, 0.f};
      if constexpr (SPATIAL) store_corners(cns + tid * FN_CN, corners_of(q.sp, c));
    }
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int fw = ps * (FN_NF / 2) + wave * 32;     // this wave's 32 frequencies of the pass
      if (fw >= fopen) continue;                       // wave-uniform; no barrier below
      f32x4 acc[4][4];
      zero_acc(acc);
      gemm_lds(hs, wt + (size_t)ps * FN_HID * FN_HID, cw, li, kq, acc);
      if constexpr (SPATIAL) {
        // point by point, both frequencies of the lane inside: a point's coordinates and corners are read once per pass and dropped
        // (features 2 f, the sine, and 2 f + 1, the cosine, are adjacent grid columns: one 8-byte load per corner); dE * m, then the
        // sums below in the same order over the points.  The accumulators leave no room to keep 16 points' worth of anything
        asm volatile("" ::: "memory");
        float fq[2][3], sm[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int f = fw + 16 * n + li;
          fq[n][0] = q.enc_a[f]; fq[n][1] = q.enc_a[FN_NF + f]; fq[n][2] = q.enc_a[2 * FN_NF + f];
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int pr = 16 * m + 4 * kq + r;
            const f32x4 c = *reinterpret_cast<const f32x4*>(cs + pr * FN_CS);
            const Corners cn = load_corners(cns + pr * FN_CN);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
              float mk[2], sn, co;
              sample_cols<2>(q.sp.grid, cn, FN_DOM + 2 * (fw + 16 * n + li), mk);
              fourier_sincos(Coord{c[0], c[1], c[2]}, fq[n][0], fq[n][1], fq[n][2], sn, co);
              const float d = mul_rn(acc[m][n][r], mk[0]) * co - mul_rn(acc[m][n + 2][r], mk[1]) * sn;
              sm[n][0] = fmaf(c[0], d, sm[n][0]);
              sm[n][1] = fmaf(c[1], d, sm[n][1]);
              sm[n][2] = fmaf(c[2], d, sm[n][2]);
            }
          }
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int d = 0; d < FN_DOM; ++d) g[ps][n][d] += sm[n][d];
        continue;
      }
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int f = fw + 16 * n + li;
        const float fa = q.enc_a[f], fb = q.enc_a[FN_NF + f], fc = q.enc_a[2 * FN_NF + f];
        float st = 0.f, sy = 0.f, sx = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const f32x4 c = *reinterpret_cast<const f32x4*>(cs + (16 * m + 4 * kq + r) * FN_CS);
            float sn, co;
            fourier_sincos(Coord{c[0], c[1], c[2]}, fa, fb, fc, sn, co);
            const float d = acc[m][n][r] * co - acc[m][n + 2][r] * sn;
            st = fmaf(c[0], d, st);
            sy = fmaf(c[1], d, sy);
            sx = fmaf(c[2], d, sx);
          }
        g[ps][n][0] += st;
        g[ps][n][1] += sy;
        g[ps][n][2] += sx;
      }
    }
  }
  // the four lanes li, li + 16, li + 32, li + 48 hold the four row groups of one frequency: (0 + 1) + (2 + 3)
  float* const out = part + (size_t)blockIdx.x * FN_EG_PART;
#pragma unroll
  for (int ps = 0; ps < 2; ++ps)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int d = 0; d < FN_DOM; ++d) {
        float v = g[ps][n][d];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (kq == 0) out[d * FN_NF + ps * (FN_NF / 2) + wave * 32 + 16 * n + li] = v;
      }
}

// g[d][f] = 2 pi sum_c part[c][d][f], blocks in index order; an exact +0 for a frequency from `fopen` on or (progressive) one whose two
// features are both closed by the mask, whatever the partial sums hold
__global__ __launch_bounds__(FN_NTHR) void flownet_reduce_enc_kernel(const float* part, int nparts, const float* mask, int fopen, float* g) {
  const int i = blockIdx.x * FN_NTHR + threadIdx.x;
  if (i >= FN_EG_PART) return;
  const int f = i % FN_NF;
  if (f >= fopen || (mask && mask[FN_DOM + 2 * f] == 0.f && mask[FN_DOM + 2 * f + 1] == 0.f)) { g[i] = 0.f; return; }
  float s = 0.f;
  for (int c = 0; c < nparts; ++c) s += part[(size_t)c * FN_EG_PART + i];
  g[i] = s * FN_TWO_PI;
}

// out[p][k] = m_k(p): thread = (point, group g of 129: g == 0 the three coordinate columns, else encoded features 4 (g - 1) ..)
constexpr int FN_GROUPS = 1 + (FN_GW - FN_DOM) / 4;
__global__ __launch_bounds__(FN_NTHR) void flownet_sample_mask_kernel(FlowNetDev q, float* out) {
  const size_t total = (size_t)q.N * FN_GROUPS;
  for (size_t i = (size_t)blockIdx.x * FN_NTHR + threadIdx.x; i < total; i += (size_t)gridDim.x * FN_NTHR) {
    const int p = (int)(i / FN_GROUPS), g = (int)(i - (size_t)p * FN_GROUPS);
    const Corners cn = corners_of(q.sp, point_coord(q, p));
    float* const o = out + (size_t)p * FN_GW;
    if (g == 0) {
#pragma unroll
      for (int k = 0; k < FN_DOM; ++k) {
        float mk[1];
        sample_cols<1>(q.sp.grid, cn, k, mk);
        o[k] = mk[0];
      }
    } else {
      const int k = FN_DOM + 4 * (g - 1);
      float mk[4];
      sample_cols<4>(q.sp.grid, cn, k, mk);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[k + j] = mk[j];
    }
  }
}

// ---- gradient with respect to the coordinates (points mode): g_poses[p][d] = sum_k dE[p][k] m_k dz_k / dx_d (p) ----
// dE = dh1 W1 is the data-gradient GEMM of flownet_encgrad_kernel, for every encoding, in passes of 256 feature columns; what differs is
// the contraction: over the FEATURES of a point, not over the points of a feature.  A tile owns its points, so nothing crosses blocks.
// Column c of a pass is CHOSEN so that a lane owns four consecutive features, the unit of encode4: wave c / 64, accumulator column block
// n = (c / 16) % 4, lane li = c % 16 holds feature 256 pass + 64 wave + 4 li + n.
constexpr int FN_PG_ROW = 4;        // floats per point of a slot of partial sums in LDS: d = 0 .. 2 and a pad
template <int KIND> constexpr int posegrad_passes() { return (Enc<KIND>::KW + FN_HID - 1) / FN_HID; }
template <int KIND> constexpr size_t posegrad_pack_floats() { return (size_t)(posegrad_passes<KIND>() * FN_HID + FN_CS) * FN_HID; }
template <int KIND> constexpr size_t posegrad_lds() { return FN_LDS + (size_t)(posegrad_passes<KIND>() * 4 * FN_P * FN_PG_ROW) * sizeof(float); }

// wt[c][j] = w1[j][feature of row c] for the rows of every pass (progressive: column 3 + feature, times its mask, an exact zero where the
// mask is zero; a feature from LIVE on: zero), then four rows of the coordinate columns, wt[NP 256 + d][j] = w1[j][d] (progressive, d < 3;
// else zero): their mask multiplies the finished sum, so the value is not scaled here, but a closed coordinate (m_d == 0) is an exact zero
// as well: 0 x (a sum over a W1 column that holds NaN) would be NaN.  spatial (with prog): column 3 + feature and the coordinate columns
// as they are, the kernel applies the point's mask to dE.  block = row c; <E::LIVE, E::KW>: encodings of one shape share one kernel
template <int LIVE, int KW>
__global__ __launch_bounds__(FN_NTHR) void flownet_posegrad_pack_kernel(const float* w1, const float* mask, float* wt, int prog, int spatial) {
  constexpr int ROWS = (KW + FN_HID - 1) / FN_HID * FN_HID;
  const int c = blockIdx.x, j = threadIdx.x;
  const float* row = w1 + (size_t)j * (LIVE + (prog ? FN_DOM : 0));
  float v = 0.f;
  if (c >= ROWS) {
    if (prog && c - ROWS < FN_DOM) v = !spatial && mask[c - ROWS] == 0.f ? 0.f : row[c - ROWS];
  } else {
    const int k = (c & ~63) + 4 * (c & 15) + ((c >> 4) & 3);
    if (k < LIVE) {
      if (spatial) {
        v = row[FN_DOM + k];
      } else if (prog) {
        const float m = mask[FN_DOM + k];
        v = m == 0.f ? 0.f : row[FN_DOM + k] * m;
      } else {
        v = row[k];
      }
    }
  }
  wt[(size_t)c * FN_HID + j] = v;
}

// the constants of features f0 .. f0 + 3 (f0 % 4 == 0), loaded once per pass, and the derivative of encode4 at one point:
// grad(c, dz, g): g[d] += sum_j dz[j] d feature_{f0 + j} / d x_d, j in index order.  The inputs and the operations up to the feature are
// encode4's; every sum is an explicit fmaf, so each unrolled copy (each row of a tile) rounds the same way
template <int KIND>
struct FeatureGrad4 {
  float par[16];
  int f0;
  __device__ __forceinline__ FeatureGrad4(const FlowNetDev& q, int f0_) : f0(f0_) {
    if constexpr (KIND == SININN_FLOWNET_RBF) {          // centres [4][3], sigma^2 [4]
      const f32x4* cp = reinterpret_cast<const f32x4*>(q.enc_a + 3 * f0);
      const f32x4 c0 = cp[0], c1 = cp[1], c2 = cp[2];
      const f32x4 sg = *reinterpret_cast<const f32x4*>(q.enc_b + f0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        par[i] = c0[i]; par[4 + i] = c1[i]; par[8 + i] = c2[i];
        par[12 + i] = sg[i] * sg[i];
      }
    } else if constexpr (KIND == SININN_FLOWNET_RBFG) {  // offsets [2][3], sigma [2]
      const int f = f0 >> 1;
      const f32x2* op = reinterpret_cast<const f32x2*>(q.enc_a + 3 * f);
      const f32x2 o0 = op[0], o1 = op[1], o2 = op[2];
      const f32x2 sg = *reinterpret_cast<const f32x2*>(q.enc_b + f);
      par[0] = o0[0]; par[1] = o0[1]; par[2] = o1[0]; par[3] = o1[1]; par[4] = o2[0]; par[5] = o2[1];
      par[6] = sg[0]; par[7] = sg[1];
    } else if constexpr (KIND == SININN_FLOWNET_PE) {    // the frequency of each of the four features
#pragma unroll
      for (int j = 0; j < 4; ++j) par[j] = f0 + j < Enc<KIND>::LIVE ? q.enc_a[(f0 + j) / 6] : 0.f;
    } else {                                             // frequencies [3][2]
      const int f = f0 >> 1;
      const f32x2 fa = *reinterpret_cast<const f32x2*>(q.enc_a + f);
      const f32x2 fb = *reinterpret_cast<const f32x2*>(q.enc_a + 256 + f);
      const f32x2 fc = *reinterpret_cast<const f32x2*>(q.enc_a + 512 + f);
      par[0] = fa[0]; par[1] = fb[0]; par[2] = fc[0]; par[3] = fa[1]; par[4] = fb[1]; par[5] = fc[1];
    }
  }

  __device__ __forceinline__ void grad(const Coord c, const float (&dz)[4], float (&g)[FN_DOM]) const {
#pragma clang fp contract(off)
    if constexpr (KIND == SININN_FLOWNET_RBF) {          // d e / d x_d = -2 sigma^2 (x_d - c_d) e
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dt = c.t - par[3 * j], dy = c.y - par[3 * j + 1], dx = c.x - par[3 * j + 2];
        const float d = fmaf(dx, dx, fmaf(dy, dy, dt * dt));
        const float t = dz[j] * ((-2.f * par[12 + j]) * expf(-(d * par[12 + j])));
        g[0] = fmaf(t, dt, g[0]);
        g[1] = fmaf(t, dy, g[1]);
        g[2] = fmaf(t, dx, g[2]);
      }
    } else if constexpr (KIND == SININN_FLOWNET_RBFG) {  // d e / d x_d = -4 sigma^2 u_d (e + 1): d u_d / d x_d = 2, the remainder's slope is 1
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float sg = par[6 + u];
        const float is = 1.f / sg, p = 2.f * is, hp = 0.5f * sg, s2 = sg * sg;
        const float xa[3] = {c.t + par[3 * u], c.y + par[3 * u + 1], c.x + par[3 * u + 2]};
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          float w[3];
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const float x = v ? xa[d] + is : xa[d];
            const float r = fmaf(-floorf(x * hp), p, x);
            w[d] = fmaf(r, 2.f, -p);
          }
          const float d = fmaf(w[2], w[2], fmaf(w[1], w[1], w[0] * w[0]));
          const float t = dz[2 * u + v] * ((-4.f * s2) * (expf(-(d * s2)) * 2.f));
          g[0] = fmaf(t, w[0], g[0]);
          g[1] = fmaf(t, w[1], g[1]);
          g[2] = fmaf(t, w[2], g[2]);
        }
      }
    } else if constexpr (KIND == SININN_FLOWNET_PE) {    // feature 6 f + d: -w sin(w x_d), 6 f + 3 + d: w cos(w x_d); its own coordinate only
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = f0 + j;
        const int r = k % 6, d = r < 3 ? r : r - 3;
        const float xd = d == 0 ? c.t : d == 1 ? c.y : c.x;
        float sn, co;
        sincosf(__fmul_rn(par[j], xd), &sn, &co);
        const float t = dz[j] * (r < 3 ? -(par[j] * sn) : par[j] * co);   // par = 0 beyond LIVE: an exact zero
        g[0] = d == 0 ? g[0] + t : g[0];
        g[1] = d == 1 ? g[1] + t : g[1];
        g[2] = d == 2 ? g[2] + t : g[2];
      }
    } else if constexpr (KIND == SININN_FLOWNET_PIECEWISE) {   // d e / d x_d = s F[d][f], s = +2 where the forward's own r < 0, else -2
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float w = piecewise_arg(c, par[3 * u], par[3 * u + 1], par[3 * u + 2]);
        const float s0 = piecewise_rem(w) < 0.f ? 2.f : -2.f, s1 = piecewise_rem(w + 1.f) < 0.f ? 2.f : -2.f;
        const float t = fmaf(dz[2 * u + 1], s1, dz[2 * u] * s0);             // both products are exact
        g[0] = fmaf(t, par[3 * u], g[0]);
        g[1] = fmaf(t, par[3 * u + 1], g[1]);
        g[2] = fmaf(t, par[3 * u + 2], g[2]);
      }
    } else {                                             // 2 pi F[d][f] (dz_sin cos(phi) - dz_cos sin(phi))
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float s, co;
        fourier_sincos(c, par[3 * u], par[3 * u + 1], par[3 * u + 2], s, co);
        const float t = FN_TWO_PI * fmaf(dz[2 * u], co, -(dz[2 * u + 1] * s));
        g[0] = fmaf(t, par[3 * u], g[0]);
        g[1] = fmaf(t, par[3 * u + 1], g[1]);
        g[2] = fmaf(t, par[3 * u + 2], g[2]);
      }
    }
  }
};

// one step of the xor butterfly over the 16 column lanes: the lanes of a pair split the N values, each keeps one half and adds the
// partner's share of it; after the steps 1, 2, 4, 8 a lane holds the three sums of ONE point
template <int N, int B>
__device__ __forceinline__ void butterfly_step(float (&v)[16 * FN_DOM], int li) {
  const bool up = (li & B) != 0;
#pragma unroll
  for (int i = 0; i < N / 2; ++i) {
    const float send = up ? v[i] : v[i + N / 2], keep = up ? v[i + N / 2] : v[i];
    v[i] = keep + __shfl_xor(send, B);
  }
}

// wt: flownet_posegrad_pack_kernel's matrix; mask: the global mask (PROG) for the coordinate columns; kopen: encoded features in front of
// the last open one (not PROG: all), a wave whose 64 columns lie beyond it skips its GEMM and contributes exact zeros.
// The order of every sum is fixed: a lane's four columns in index order (fmaf), the 16 lanes by the butterfly, then the slots
// (pass, wave) in index order, then (PROG) m_d times the coordinate column's sum.  Rows p >= N are not written
// SPATIAL (with PROG): wt is unmasked, `mask` unused; a lane's four features of a point are multiplied by the point's mask of those features
// (sample_cols on the corner tile, one rounded product each) before FeatureGrad4::grad, the coordinate column's sum by m_d(p).  Grid columns
// from k_active on are zero, so the skipped waves would have added dE * 0: kopen skips exactly, as above
template <int KIND, bool PROG, bool SPATIAL = false>
__global__ __launch_bounds__(FN_NTHR, 2) void flownet_posegrad_kernel(FlowNetDev q, const float* wt, const float* mask, float* g_poses,
                                                                     int kopen) {
  static_assert(PROG || !SPATIAL, "a spatial mask is a progressive network's");
  constexpr int NP = posegrad_passes<KIND>();
  extern __shared__ __attribute__((aligned(16))) float fn_smem[];
  float* const hs = fn_smem;                           // [64][FN_HS]: dh1 tile
  float* const cs = fn_smem + FN_P * FN_HS;            // [64][4]: coordinates of the tile's points
  float* const red = cs + FN_P * FN_CS;                // [NP * 4][64][FN_PG_ROW]: a wave's sums of a pass
  float* const cns = red + NP * 4 * FN_P * FN_PG_ROW;  // SPATIAL: [64][FN_CN]: the corners of the tile's points
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kq = lane >> 4;
  const int cw = wave * 64;
  // the point whose sums this lane holds after the butterfly: bit b of li chose the upper half at step b
  const int pt = ((li & 1) << 3) | ((li & 2) << 1) | ((li & 4) >> 1) | ((li & 8) >> 3);
  const int prow = 16 * (pt >> 2) + 4 * kq + (pt & 3);

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    __syncthreads();                                   // the previous tile is done with hs / cs / red
#pragma unroll 4
    for (int u = 0; u < FN_P * FN_HID / 4 / FN_NTHR; ++u) {
      const int f = tid + FN_NTHR * u;
      const int row = f >> 6, c4 = (f & 63) * 4;
      *reinterpret_cast<f32x4*>(hs + row * FN_HS + c4) = *reinterpret_cast<const f32x4*>(q.dh + ((size_t)tile * FN_P + row) * FN_HID + c4);
    }
    if constexpr (SPATIAL) {
      if (tid < FN_P) {
        const Coord c = point_coord(q, tile * FN_P + tid);
        *reinterpret_cast<f32x4*>(cs + tid * FN_CS) = (f32x4){c.t, c.y, c.x, 0.f};
        store_corners(cns + tid * FN_CN, corners_of(q.sp, c));
      }
    } else {
      if (tid < FN_P) stage_coord(q, cs, tile, tid);
    }
    __syncthreads();
    // ---- the coordinate columns on the vector ALU: thread = (coordinate tid / 64, point tid % 64) ----
    float csum = 0.f;
    if constexpr (PROG) {
      if (wave < FN_DOM) {
        const float* wc = wt + (size_t)(NP * FN_HID + wave) * FN_HID;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
        for (int k = 0; k < FN_HID; k += 4) {
          const f32x4 h = *reinterpret_cast<const f32x4*>(hs + lane * FN_HS + k);
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wc + k);
          a0 = fmaf(h[0], wv[0], a0);
          a1 = fmaf(h[1], wv[1], a1);
          a2 = fmaf(h[2], wv[2], a2);
          a3 = fmaf(h[3], wv[3], a3);
        }
        csum = (a0 + a1) + (a2 + a3);
      }
    }
    // ---- the encoded features: 256 columns per pass, 64 per wave ----
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
      const int k0 = ps * FN_HID + cw;
      float v[16 * FN_DOM];
#pragma unroll
      for (int i = 0; i < 16 * FN_DOM; ++i) v[i] = 0.f;
      if (k0 < kopen) {                                // wave-uniform; no barrier inside
        f32x4 acc[4][4];
        zero_acc(acc);
        gemm_lds(hs, wt + (size_t)ps * FN_HID * FN_HID, cw, li, kq, acc);
        const FeatureGrad4<KIND> fg(q, k0 + 4 * li);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const f32x4 c = *reinterpret_cast<const f32x4*>(cs + (16 * m + 4 * kq + r) * FN_CS);
            float dz[4] = {acc[m][0][r], acc[m][1][r], acc[m][2][r], acc[m][3][r]};
            if constexpr (SPATIAL) {
              float mk[4];
              sample_cols<4>(q.sp.grid, load_corners(cns + (16 * m + 4 * kq + r) * FN_CN), FN_DOM + k0 + 4 * li, mk);
#pragma unroll
              for (int j = 0; j < 4; ++j) dz[j] = mul_rn(dz[j], mk[j]);
            }
            float g[FN_DOM] = {0.f, 0.f, 0.f};
            fg.grad(Coord{c[0], c[1], c[2]}, dz, g);
#pragma unroll
            for (int d = 0; d < FN_DOM; ++d) v[(4 * m + r) * FN_DOM + d] = g[d];
            if constexpr (SPATIAL) __builtin_amdgcn_sched_barrier(0);   // one point's eight grid rows in flight at a time, as in the forward kernel
          }
        butterfly_step<48, 1>(v, li);
        butterfly_step<24, 2>(v, li);
        butterfly_step<12, 4>(v, li);
        butterfly_step<6, 8>(v, li);
      }
      *reinterpret_cast<f32x4*>(red + ((size_t)(ps * 4 + wave) * FN_P + prow) * FN_PG_ROW) = (f32x4){v[0], v[1], v[2], 0.f};
    }
    __syncthreads();
    const int p = tile * FN_P + lane;
    if (wave < FN_DOM && p < q.N) {
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < NP * 4; ++u) s += red[(u * FN_P + lane) * FN_PG_ROW + wave];
      if constexpr (SPATIAL) {
        float md[1];
        sample_cols<1>(q.sp.grid, load_corners(cns + lane * FN_CN), wave, md);
        s += mul_rn(md[0], csum);
      } else if constexpr (PROG) {
        s += mul_rn(mask[wave], csum);
      }
      g_poses[(size_t)p * FN_DOM + wave] = s;
    }
  }
}

int wgrad_chunks(int ntiles, int kf) {
  const int want = FN_CHUNK_ELEMS / kf;                // 128 chunks x 4 output tiles, 64 x 8 (narrow: 256 x 2) for layer 1
  return ntiles < want ? ntiles : want;
}


// the largest set of partial sums of a backward call: a hidden layer's, any encoding's progressive layer 1, the chain kernel's
size_t part_floats(int ntiles) {
  size_t n = (size_t)wgrad_chunks(ntiles, Hidden::CHUNK_KF) * Hidden::part_stride(false);
  const size_t c = (size_t)chain_blocks(ntiles) * (FN_OUT * FN_HID + FN_OUT);
  n = n > c ? n : c;
  for (int kind : FN_KINDS) {
    const size_t b = for_kind(kind, (size_t)0, [&](auto k) {
      using E = Enc<decltype(k)::value>;
      return (size_t)wgrad_chunks(ntiles, E::CHUNK_KF) * E::part_stride(true);
    });
    n = n > b ? n : b;
  }
  return n;
}

// encoded features in front of the last open one
int open_encoded(const sininn_flownet_args* a, int dim = FN_DOM) { return a->k_active > dim ? a->k_active - dim : 0; }

void reduce_launch(const FlowNetDev& q, int nparts, int nw, int nb, float* gw, float* gb, hipStream_t st) {
  hipLaunchKernelGGL(flownet_reduce_kernel, dim3((nw + nb + FN_NTHR - 1) / FN_NTHR), dim3(FN_NTHR), 0, st, (const float*)q.part, nparts, nw, nb, gw, gb);
}

}  // namespace

// gW [256][256] = dh^T in, gb [256] = sum_p dh for one hidden layer, from two [64 ntiles][256] arrays: the split-over-points kernel, then
// its partial sums in chunk order.  `part`: hidden_wgrad_part_floats(ntiles) floats.  Shared with siren.hip
size_t hidden_wgrad_part_floats(int ntiles) { return (size_t)wgrad_chunks(ntiles, Hidden::CHUNK_KF) * Hidden::part_stride(false); }

int hidden_wgrad_launch(int ntiles, const float* dh, const float* in, float* part, float* gw, float* gb, hipStream_t st) {
  FlowNetDev q = {};
  q.ntiles = ntiles;
  q.part = part;
  auto k = flownet_wgrad_kernel<SININN_FLOWNET_RBF, false>;
  if (raise_lds(k, wgrad_lds(false, false), "flownet_wgrad")) return 1;
  const int nc = wgrad_chunks(ntiles, Hidden::CHUNK_KF);
  hipLaunchKernelGGL(k, dim3(2 * Hidden::KW / Hidden::KT, nc), dim3(FN_NTHR), wgrad_lds(false, false), st, q, dh, in);
  SININN_LAUNCH_CHECK("flownet_wgrad");
  reduce_launch(q, nc, FN_HID * FN_HID, FN_HID, gw, gb, st);
  SININN_LAUNCH_CHECK("flownet_reduce");
  return 0;
}

// the support table; a refusal leaves its reason, with the table, as the library's last error
static int flownet_supported(const sininn_flownet_args* a, const char* who);

// two coordinates per point (domain_dim = 2): the encodings whose Enc<> row says PAIR, 512 wide, progressive 514
static int flownet_supported_pair(const sininn_flownet_args* a, const char* who) {
  const bool prog = a->progressive == 1;
  const bool ok = (a->progressive == 0 || prog) && a->hidden == FN_HID && a->layers == 3 && a->out_dim == FN_OUT &&
                  for_kind(a->encoding, false, [&](auto k) {
                    using E = Enc<decltype(k)::value>;
                    return E::PAIR && a->enc_dim == E::width(prog, 2);
                  });
  if (!ok) {
    std::string table;
    for (int kind : FN_KINDS)
      for_kind(kind, 0, [&](auto k) {
        using E = Enc<decltype(k)::value>;
        if (E::PAIR)
          table += std::string(table.empty() ? "" : ", ") + E::NAME + " " + std::to_string(E::width(false, 2)) + " (progressive: " +
                   std::to_string(E::width(true, 2)) + ")";
        return 0;
      });
    set_error("%s: unsupported network at domain_dim 2 (encoding %d, %d -> %d x %d -> %d, progressive %d; with two coordinates per point the "
              "kernels are built for %s -> %d x 3 -> %d; PE and PieceWise take three coordinates only)", who, a->encoding, a->enc_dim, a->hidden,
              a->layers, a->out_dim, a->progressive, table.c_str(), FN_HID, FN_OUT);
  }
  return ok;
}

static int flownet_supported_dim(const sininn_flownet_args* a, int dim, const char* who) {
  if (a == nullptr || a->struct_bytes != sizeof(sininn_flownet_args)) return 0;
  if (dim == FN_DOM) return flownet_supported(a, who);
  if (dim == 2) return flownet_supported_pair(a, who);
  set_error("%s: domain_dim %d: the kernels take 3 coordinates per point (t, y, x) or 2 (y, x)", who, dim);
  return 0;
}

static int flownet_supported(const sininn_flownet_args* a, const char* who) {
  if (a == nullptr || a->struct_bytes != sizeof(sininn_flownet_args)) return 0;
  const bool prog = a->progressive == 1;
  const bool ok = (a->progressive == 0 || prog) && a->hidden == FN_HID && a->layers == 3 && a->out_dim == FN_OUT &&
                  for_kind(a->encoding, false, [&](auto k) {
                    using E = Enc<decltype(k)::value>;
                    return a->enc_dim == E::width(prog) && (prog || E::PLAIN);
                  });
  if (!ok) {
    std::string table;
    for (int kind : FN_KINDS)
      for_kind(kind, 0, [&](auto k) {
        using E = Enc<decltype(k)::value>;
        table += std::string(table.empty() ? "" : ", ") + E::NAME + " " +
                 (E::PLAIN ? std::to_string(E::width(false)) + " (progressive: " + std::to_string(E::width(true)) + ")"
                           : "progressive only: " + std::to_string(E::width(true)));
        return 0;
      });
    set_error("%s: unsupported network (encoding %d, %d -> %d x %d -> %d, progressive %d; built for %s -> %d x 3 -> %d)", who, a->encoding,
              a->enc_dim, a->hidden, a->layers, a->out_dim, a->progressive, table.c_str(), FN_HID, FN_OUT);
  }
  return ok;
}

extern "C" int sininn_flownet_supported(const sininn_flownet_args* a) { return flownet_supported(a, "sininn_flownet_supported"); }
extern "C" int sininn_flownet_supported_dim(const sininn_flownet_args* a, int dim) {
  return flownet_supported_dim(a, dim, "sininn_flownet_supported_dim");
}

extern "C" size_t sininn_flownet_forward_workspace_bytes(const sininn_flownet_args* a) {
  if (a == nullptr || a->struct_bytes != sizeof(sininn_flownet_args) || !a->progressive) return 0;   // plain PE reads W1 in place
  return for_kind(a->encoding, (size_t)0, [](auto k) { return Enc<decltype(k)::value>::PACK_FLOATS * sizeof(float); });
}

extern "C" size_t sininn_flownet_saved_bytes(int64_t n) {
  if (n <= 0) return 0;
  return (size_t)3 * (size_t)((n + FN_P - 1) / FN_P) * FN_P * FN_HID * sizeof(float);
}

extern "C" size_t sininn_flownet_workspace_bytes(int64_t n) {
  if (n <= 0 || n > ((int64_t)1 << 22)) return 0;
  const int ntiles = (int)((n + FN_P - 1) / FN_P);
  return sininn_flownet_saved_bytes(n) + ((size_t)2 * FN_HID * FN_HID + part_floats(ntiles)) * sizeof(float);
}

extern "C" size_t sininn_flownet_encgrad_workspace_bytes(const sininn_flownet_args* a) {
  const bool has = a != nullptr && a->struct_bytes == sizeof(sininn_flownet_args) &&
                   for_kind(a->encoding, false, [](auto k) { return Enc<decltype(k)::value>::FREQ_GRAD; });
  return has ? FN_EG_FLOATS * sizeof(float) : 0;
}

// the head of every entry point: a struct of this library's size that describes a network the kernels are built for; spatial != nullptr:
// and the spatial mode, a 515-wide progressive network and a grid the kernels can index.  Everything a launch would trip over, before any
// launch
// dim: coordinates per point; 2 exists without a spatial mask only (check_call has refused the grid there)
static int check_head(const sininn_flownet_args* a, const char* who, const SpatialArgs* spatial, int dim = FN_DOM) {
  SININN_CHECK(a != nullptr, "%s: null args", who);
  SININN_CHECK(a->struct_bytes == sizeof(sininn_flownet_args), "%s: struct_bytes is %zu, this library was built with %zu", who,
               a->struct_bytes, sizeof(sininn_flownet_args));
  if (!flownet_supported_dim(a, dim, who)) return 1;
  if (!spatial) return 0;
  SININN_CHECK(a->progressive == 1, "%s: a spatial mask needs a progressive network (progressive = 1)", who);
  SININN_CHECK(a->enc_dim == FN_GW,
               "%s: spatial masks are built for the %d-wide progressive encodings (PRBF, PFF / PUFF / PRFF, PRBFG, MPFF); PPE (enc_dim %d, a packed "
               "narrow layer 1 of its own) is out of scope for this mode", who, FN_GW, a->enc_dim);
  SININN_CHECK(spatial->grid != nullptr && spatial->centre_scale != nullptr, "%s: null grid / centre_scale", who);
  SININN_CHECK(spatial->res >= 3, "%s: res %d (at least 3)", who, spatial->res);
  SININN_CHECK((int64_t)spatial->res * spatial->res * spatial->res * FN_GW <= (int64_t)INT32_MAX,
               "%s: res %d: res^3 * %d exceeds the kernels' 32-bit indexing", who, spatial->res, FN_GW);
  return 0;
}

// the kernels' view of a grid that check_head has accepted; nullptr: none
static Spatial spatial_of(const SpatialArgs* s) {
  Spatial sp{};
  if (s) {
    sp.grid = s->grid;
    sp.res = s->res;
    sp.span = (float)(s->res - 2 > 1 ? s->res - 2 : 1);
    for (int d = 0; d < 3; ++d) {
      sp.centre[d] = s->centre_scale[d];
      sp.scale[d] = s->centre_scale[3 + d];
    }
  }
  return sp;
}

// the descriptor of a call whose entry point has called check_head, checked and copied into q.  spatial != nullptr: the descriptor's mask
// is ignored, the grid goes to q.sp.  pl != nullptr: the points are that pose list, not the descriptor's grid (with or without spatial)
// dim = 2: the grid is (ys, xs) with T = 1, `times` is not read; a pose list is [n][2]
static int fill_args(const sininn_flownet_args* a, const char* who, FlowNetDev& q, const SpatialArgs* spatial, const PoseList* pl = nullptr,
                     int dim = FN_DOM) {
  q = FlowNetDev{};
  q.sp = spatial_of(spatial);
  if (a->progressive) {
    SININN_CHECK(spatial || a->mask != nullptr, "%s: progressive network without a mask", who);
    SININN_CHECK(a->k_active >= 0 && a->k_active <= a->enc_dim, "%s: k_active %d (0 .. %d)", who, a->k_active, a->enc_dim);
  }
  const bool enc_b = for_kind(a->encoding, false, [](auto k) { return Enc<decltype(k)::value>::ENC_B; });
  if (dim == 2 && !pl) {
    SININN_CHECK(a->T == 1 && a->H > 0 && a->W > 0 && (int64_t)a->H * a->W <= (int64_t)1 << 22,
                 "%s: domain_dim 2: grid %d x %d x %d (T = 1: one frame pair; 1 .. 2^22 points)", who, a->T, a->H, a->W);
    SININN_CHECK(a->ys && a->xs && a->enc_a && (a->enc_b || !enc_b), "%s: null axis / encoding pointer", who);
    q.T = 1; q.H = a->H; q.W = a->W;
    q.ys = a->ys; q.xs = a->xs;
    q.N = q.H * q.W;
    q.ntiles = (q.N + FN_P - 1) / FN_P;
  } else if (int rc = check_points(a, who, q, pl, a->enc_a && (a->enc_b || !enc_b), pl ? "encoding" : "axis / encoding")) {
    return rc;
  }
  SININN_CHECK(aligned16(a->enc_a) && aligned16(a->enc_b), "%s: encoding buffers must be 16-byte aligned", who);
  if (int rc = check_layers<4>(a, who, q)) return rc;
  q.scale = a->scale;
  q.enc_a = a->enc_a; q.enc_b = a->enc_b;
  return 0;
}

// f(KIND, PROG, SPATIAL) as integral constants for the run-time mode of a call, next to for_kind.  The spatial instantiations exist for
// the FN_GW-wide progressive networks, the only ones check_head lets into that mode
template <class F>
static int for_mode(const sininn_flownet_args* a, bool spatial, F&& f) {
  return for_kind(a->encoding, 1, [&](auto k) {
    using E = Enc<decltype(k)::value>;
    if constexpr (E::width(true) == FN_GW) {
      if (spatial) return f(k, std::true_type{}, std::true_type{});
    }
    if constexpr (!E::PLAIN) return f(k, std::true_type{}, std::false_type{});   // flownet_supported has refused the plain form
    else return a->progressive ? f(k, std::true_type{}, std::false_type{}) : f(k, std::false_type{}, std::false_type{});
  });
}

// f(KIND, PROG) for a network that flownet_supported_pair has accepted: the kinds with two-coordinate kernels
template <class F>
static int for_pair(const sininn_flownet_args* a, F&& f) {
  return for_kind(a->encoding, 1, [&](auto k) {
    using E = Enc<decltype(k)::value>;
    if constexpr (E::PAIR) return a->progressive ? f(k, std::true_type{}) : f(k, std::false_type{});
    else return 1;
  });
}

// layer 1: gW1 = dh1^T (regenerated input), gb1, and their reduction into nn.Linear's layout
template <int KIND, bool PROG, bool SPATIAL, int DIM = FN_DOM>
static int wgrad_l1_launch(const sininn_flownet_args* a, const FlowNetDev& q, hipStream_t st) {
  using E = Enc<KIND>;
  constexpr size_t lds = wgrad_lds(PROG, SPATIAL);
  auto k = flownet_wgrad_kernel<KIND, true, PROG, SPATIAL, DIM>;
  if (raise_lds(k, lds, "flownet_wgrad")) return 1;
  const int nc = wgrad_chunks(q.ntiles, E::CHUNK_KF);  // not a function of k_active: the order of every sum stays the same
  // progressive, wide: the open 128-column tiles of the encoded features only (at least one: it carries gb1 and the coordinate
  // columns); narrow: the one column tile, always whole
  const int oe = open_encoded(a, DIM);
  const int ktiles = PROG && !E::NARROW ? (oe > 0 ? (oe + FN_WT - 1) / FN_WT : 1) : E::KW / E::KT;
  hipLaunchKernelGGL(k, dim3(2 * ktiles, nc), dim3(FN_NTHR), lds, st, q, (const float*)q.dh, (const float*)nullptr);
  SININN_LAUNCH_CHECK("flownet_wgrad");
  if constexpr (!PROG && E::LIVE == E::KW) {           // the partial sums are in nn.Linear's layout already
    reduce_launch(q, nc, FN_HID * E::LIVE, FN_HID, a->gw[0], a->gb[0], st);
  } else {
    const int kcols = !PROG ? E::LIVE : E::NARROW ? oe : ktiles * FN_WT;
    hipLaunchKernelGGL((flownet_reduce_l1_kernel<E::KW, E::LIVE, PROG, DIM>), dim3((FN_HID * E::width(PROG, DIM) + FN_HID + FN_NTHR - 1) / FN_NTHR),
                       dim3(FN_NTHR), 0, st, (const float*)q.part, nc, PROG && !SPATIAL ? a->mask : (const float*)nullptr, kcols, a->gw[0], a->gb[0]);
  }
  SININN_LAUNCH_CHECK("flownet_reduce");
  return 0;
}

// ENCGRAD: also the gradient of the frequencies, from dh1 (which the weight-gradient kernels only read) and a workspace of its own, enc_ws
// SPATIAL: layer 1 under the per-point mask of that grid.  AT_POINTS: at that pose list.  The caller has called check_head
// Every refusal is made under the call's own name where that is the posegrad call or the spatial call at a pose list, else under the names
// the backward calls have always used.
// out_q != nullptr: receives the kernels' descriptor of the call (dh1 is slot 0 of q.dh) for a kernel the caller launches after these
// domain_dim 2: two coordinates per point; no grid, no frequency gradient (check_call has refused both)
static int backward_launch(const sininn_flownet_args* a, const Call& c, float* enc_ws, hipStream_t st, FlowNetDev* out_q = nullptr) {
  const SpatialArgs* const spatial = c.spatial();
  const PoseList* const pl = c.pl();
  const int dim = c.c.domain_dim;
  float* const g_enc_a = c.has(SININN_FLOWNET_ENCGRAD) ? c.c.g_enc_a : nullptr;
  const char* const who = c.has(SININN_FLOWNET_POSEGRAD) || (spatial && pl) ? c.who() : nullptr;
  FlowNetDev q;
  if (int rc = fill_args(a, who ? who : spatial ? "flownet_backward_spatial" : pl ? "flownet_backward_points" : "flownet_backward", q, spatial, pl, dim)) return rc;
  if (int rc = check_backward_buffers<4>(a, who ? who : pl ? "flownet_backward_points" : "flownet_backward", sininn_flownet_saved_bytes(q.N), sininn_flownet_workspace_bytes(q.N), q))
    return rc;
  const size_t lstride = (size_t)q.ntiles * FN_P * FN_HID;
  float* const ws = static_cast<float*>(a->workspace);
  float* const wt = ws + 3 * lstride;
  q.dh = ws;
  q.wt = wt;
  q.part = wt + 2 * FN_HID * FN_HID;

  hipLaunchKernelGGL(flownet_transpose_kernel, dim3(FN_HID, 2), dim3(FN_NTHR), 0, st, a->w[1], a->w[2], wt);
  SININN_LAUNCH_CHECK("flownet_transpose");
  if (raise_lds(flownet_bwd_chain_kernel, tile_lds(false), "flownet_backward")) return 1;
  const int cb = chain_blocks(q.ntiles);
  hipLaunchKernelGGL(flownet_bwd_chain_kernel, dim3(cb), dim3(FN_NTHR), tile_lds(false), st, q);
  SININN_LAUNCH_CHECK("flownet_bwd_chain");
  reduce_launch(q, cb, FN_OUT * FN_HID, FN_OUT, a->gw[3], a->gb[3], st);
  SININN_LAUNCH_CHECK("flownet_reduce");
  for (int l = 2; l >= 1; --l)                         // gW3 = dh3^T h2, gW2 = dh2^T h1
    if (int rc = hidden_wgrad_launch(q.ntiles, q.dh + l * lstride, q.saved + (l - 1) * lstride, q.part, a->gw[l], a->gb[l], st)) return rc;
  if (dim == 2) {
    if (int rc = for_pair(a, [&](auto k, auto prog) { return wgrad_l1_launch<decltype(k)::value, decltype(prog)::value, false, 2>(a, q, st); }))
      return rc;
  } else if (int rc = for_mode(a, spatial != nullptr, [&](auto k, auto prog, auto sp) {
               return wgrad_l1_launch<decltype(k)::value, decltype(prog)::value, decltype(sp)::value>(a, q, st);
             })) {
    return rc;
  }
  if (g_enc_a) {
    float* const epart = enc_ws + (size_t)Fourier::LIVE * FN_HID;
    const float* const mask = a->progressive && !spatial ? a->mask : nullptr;
    const int fopen = a->progressive ? (open_encoded(a) + 1) / 2 : FN_NF;   // a frequency is open if its sin or its cos is
    hipLaunchKernelGGL(flownet_encgrad_pack_kernel, dim3(Fourier::LIVE), dim3(FN_NTHR), 0, st, a->w[0], mask, enc_ws, spatial ? 1 : 0);
    SININN_LAUNCH_CHECK("flownet_encgrad_pack");
    const size_t elds = tile_lds(spatial != nullptr);
    auto ek = spatial ? flownet_encgrad_kernel<true> : flownet_encgrad_kernel<false>;
    if (raise_lds(ek, elds, "flownet_encgrad")) return 1;
    hipLaunchKernelGGL(ek, dim3(cb), dim3(FN_NTHR), elds, st, q, (const float*)enc_ws, epart, fopen);   // not a function of k_active
    SININN_LAUNCH_CHECK("flownet_encgrad");
    hipLaunchKernelGGL(flownet_reduce_enc_kernel, dim3((FN_EG_PART + FN_NTHR - 1) / FN_NTHR), dim3(FN_NTHR), 0, st, (const float*)epart, cb, mask,
                       fopen, g_enc_a);
    SININN_LAUNCH_CHECK("flownet_reduce_enc");
  }
  if (out_q) *out_q = q;
  return 0;
}

// PROG without SPATIAL: the pack step, W1 times the global mask into the workspace; SPATIAL: W1 in place, no pack kernel, no workspace
template <int KIND, bool PROG, bool SPATIAL, int DIM = FN_DOM>
static int forward_kind_launch(const sininn_flownet_args* a, FlowNetDev& q, hipStream_t st) {
  using E = Enc<KIND>;
  constexpr const char* who = SPATIAL ? "flownet_forward_spatial" : "flownet_forward";
  if constexpr (PROG && !SPATIAL) {
    SININN_CHECK(a->workspace != nullptr && a->workspace_bytes >= sininn_flownet_forward_workspace_bytes(a),
                 "flownet_forward: the progressive forward packs W1 into a workspace of %zu bytes, %zu given", sininn_flownet_forward_workspace_bytes(a),
                 a->workspace ? a->workspace_bytes : (size_t)0);
    SININN_CHECK(aligned16(a->workspace), "flownet_forward: workspace must be 16-byte aligned");
    float* const w1p = static_cast<float*>(a->workspace);
    float* const wc = w1p + (size_t)FN_HID * E::KW;
    hipLaunchKernelGGL((flownet_pack_kernel<E::KW, E::LIVE, DIM>), dim3(FN_HID), dim3(FN_NTHR), 0, st, a->w[0], a->mask, w1p, wc);
    SININN_LAUNCH_CHECK("flownet_pack");
    q.w[0] = w1p;
    q.wc = wc;
  }
  if constexpr (PROG) q.ksteps = (open_encoded(a, DIM) + 15) / 16;
  auto k = flownet_fwd_kernel<KIND, PROG, SPATIAL, DIM>;
  if (raise_lds(k, tile_lds(SPATIAL), who)) return 1;
  const int blocks = q.ntiles < FN_FWD_MAX_BLOCKS ? q.ntiles : FN_FWD_MAX_BLOCKS;
  hipLaunchKernelGGL(k, dim3(blocks), dim3(FN_NTHR), tile_lds(SPATIAL), st, q);
  SININN_LAUNCH_CHECK(who);
  return 0;
}

extern "C" int sininn_flownet_forward(const sininn_flownet_args* a, const sininn_flownet_call* call, void* stream) {
  hipStream_t st = ST(stream);
  Call c;
  if (int rc = check_call(call, "flownet", CALL_FORWARD, c)) return rc;
  const SpatialArgs* const spatial = c.spatial();
  const PoseList* const pl = c.pl();
  const int dim = c.c.domain_dim;
  const char* const who = c.who();
  FlowNetDev q;
  if (int rc = check_head(a, who, spatial, dim)) return rc;
  if (int rc = fill_args(a, who, q, spatial, pl, dim)) return rc;
  if (int rc = check_forward_buffers(a, pl ? who : "flownet_forward", sininn_flownet_saved_bytes(q.N), q)) return rc;
  if (dim == 2)
    return for_pair(a, [&](auto k, auto prog) { return forward_kind_launch<decltype(k)::value, decltype(prog)::value, false, 2>(a, q, st); });
  return for_mode(a, spatial != nullptr, [&](auto k, auto prog, auto sp) {
    return forward_kind_launch<decltype(k)::value, decltype(prog)::value, decltype(sp)::value>(a, q, st);
  });
}

extern "C" int sininn_flownet_sample_mask(const sininn_flownet_args* a, const sininn_flownet_call* call, float* out, void* stream) {
  hipStream_t st = ST(stream);
  Call c;
  if (int rc = check_call(call, "flownet", CALL_SAMPLE_MASK, c)) return rc;
  const char* const who = c.who();
  if (int rc = check_head(a, who, c.spatial())) return rc;
  SININN_CHECK(out != nullptr, "%s: null out", who);
  FlowNetDev q{};
  if (int rc = check_points(a, who, q, c.pl())) return rc;
  q.sp = spatial_of(c.spatial());
  const size_t units = ((size_t)q.N * FN_GROUPS + FN_NTHR - 1) / FN_NTHR;
  hipLaunchKernelGGL(flownet_sample_mask_kernel, dim3((unsigned)(units < 8192 ? units : 8192)), dim3(FN_NTHR), 0, st, q, out);
  SININN_LAUNCH_CHECK("flownet_sample_mask");
  return 0;
}

// the head under this call's own name, so that a refusal of the spatial mode (PPE, a null grid, res) comes before the Fourier-only
// refusal, which would hide it
static int backward_encgrad_launch(const sininn_flownet_args* a, const Call& c, hipStream_t st) {
  const char* const who = c.who();
  if (int rc = check_head(a, who, c.spatial())) return rc;
  SININN_CHECK(sininn_flownet_encgrad_workspace_bytes(a) != 0, "%s: encoding is %d; the gradient of enc_a exists for SININN_FLOWNET_FOURIER only", who,
               a->encoding);
  SININN_CHECK(c.c.g_enc_a != nullptr, "%s: null g_enc_a", who);
  SININN_CHECK(c.c.enc_workspace != nullptr && c.c.enc_workspace_bytes >= sininn_flownet_encgrad_workspace_bytes(a),
               "%s: enc_workspace holds %zu bytes, %zu needed", who, c.c.enc_workspace ? c.c.enc_workspace_bytes : (size_t)0,
               sininn_flownet_encgrad_workspace_bytes(a));
  SININN_CHECK(aligned16(c.c.enc_workspace), "%s: enc_workspace must be 16-byte aligned", who);
  return backward_launch(a, c, static_cast<float*>(c.c.enc_workspace), st);
}

// ---- POSEGRAD: the gradient of the coordinates.  extra workspace: the packed W1 of flownet_posegrad_pack_kernel, then (with ENCGRAD) the
// workspace of the frequency gradient ----
static size_t posegrad_pack_bytes(const sininn_flownet_args* a) {
  return for_kind(a->encoding, (size_t)0, [](auto k) { return posegrad_pack_floats<decltype(k)::value>() * sizeof(float); });
}

extern "C" size_t sininn_flownet_posegrad_workspace_bytes(const sininn_flownet_args* a, int with_enc_grad) {
  if (a == nullptr || a->struct_bytes != sizeof(sininn_flownet_args)) return 0;
  const size_t pack = posegrad_pack_bytes(a);
  return pack ? pack + (with_enc_grad ? sininn_flownet_encgrad_workspace_bytes(a) : 0) : 0;
}

// SPATIAL: the pack is unmasked and no global mask is read; the corner tile comes on top of posegrad_lds
template <int KIND, bool PROG, bool SPATIAL>
static int posegrad_kind_launch(const sininn_flownet_args* a, const FlowNetDev& q, float* wt, float* g_poses, hipStream_t st) {
  using E = Enc<KIND>;
  constexpr int NP = posegrad_passes<KIND>();
  constexpr size_t lds = posegrad_lds<KIND>() + (SPATIAL ? FN_CN_LDS : 0);
  const float* const mask = PROG && !SPATIAL ? a->mask : (const float*)nullptr;
  hipLaunchKernelGGL((flownet_posegrad_pack_kernel<E::LIVE, E::KW>), dim3(NP * FN_HID + FN_CS), dim3(FN_NTHR), 0, st, a->w[0], mask, wt,
                     PROG ? 1 : 0, SPATIAL ? 1 : 0);
  SININN_LAUNCH_CHECK("flownet_posegrad_pack");
  auto k = flownet_posegrad_kernel<KIND, PROG, SPATIAL>;
  if (raise_lds(k, lds, "flownet_posegrad")) return 1;
  hipLaunchKernelGGL(k, dim3(chain_blocks(q.ntiles)), dim3(FN_NTHR), lds, st, q, (const float*)wt, mask, g_poses,
                     PROG ? open_encoded(a) : E::KW);
  SININN_LAUNCH_CHECK("flownet_posegrad");
  return 0;
}

static int backward_posegrad_launch(const sininn_flownet_args* a, const Call& c, hipStream_t st) {
  const char* const who = c.who();
  const bool enc_grad = c.has(SININN_FLOWNET_ENCGRAD);
  if (int rc = check_head(a, who, c.spatial())) return rc;
  SININN_CHECK(c.c.g_poses != nullptr, "%s: null g_poses", who);
  SININN_CHECK(!enc_grad || sininn_flownet_encgrad_workspace_bytes(a) != 0,
               "%s: encoding is %d; the gradient of enc_a exists for SININN_FLOWNET_FOURIER only (pass a null g_enc_a)", who, a->encoding);
  SININN_CHECK(!enc_grad || c.c.g_enc_a != nullptr, "%s: null g_enc_a", who);
  const size_t need = sininn_flownet_posegrad_workspace_bytes(a, enc_grad);
  SININN_CHECK(c.c.extra_workspace != nullptr && c.c.extra_workspace_bytes >= need, "%s: extra_workspace holds %zu bytes, %zu needed", who,
               c.c.extra_workspace ? c.c.extra_workspace_bytes : (size_t)0, need);
  SININN_CHECK(aligned16(c.c.extra_workspace), "%s: extra_workspace must be 16-byte aligned", who);
  float* const wt = static_cast<float*>(c.c.extra_workspace);
  float* const enc_ws = enc_grad ? wt + posegrad_pack_bytes(a) / sizeof(float) : nullptr;
  FlowNetDev q;                                        // every check is backward_launch's, made before its first launch
  if (int rc = backward_launch(a, c, enc_ws, st, &q)) return rc;
  return for_mode(a, c.spatial() != nullptr, [&](auto k, auto prog, auto sp) {
    return posegrad_kind_launch<decltype(k)::value, decltype(prog)::value, decltype(sp)::value>(a, q, wt, c.c.g_poses, st);
  });
}

extern "C" int sininn_flownet_backward(const sininn_flownet_args* a, const sininn_flownet_call* call, void* stream) {
  hipStream_t st = ST(stream);
  Call c;
  if (int rc = check_call(call, "flownet", CALL_BACKWARD, c)) return rc;
  if (c.has(SININN_FLOWNET_POSEGRAD)) return backward_posegrad_launch(a, c, st);
  if (c.has(SININN_FLOWNET_ENCGRAD)) return backward_encgrad_launch(a, c, st);
  if (int rc = check_head(a, c.who(), c.spatial(), c.c.domain_dim)) return rc;
  return backward_launch(a, c, nullptr, st);
}

#include "flownet_jacobian.h"   // the Jacobian as an output: new kernels beside the ones above, which it launches and does not change

}  // namespace sininn
