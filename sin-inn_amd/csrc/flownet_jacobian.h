// The Jacobian of the flow-field network as an OUTPUT: jac[d][c][p] = scale * d out_c / d x_d at a pose list, d in a direction set D of
// (t, y, x), with a gradient to the parameters.  Included at the end of flownet.hip, inside namespace sininn: Enc<>, encode4's
// helpers, FlowNetDev, the host checks and the plain launches are that file's, and no kernel of that file is touched.
//
// The networks are ReLU MLPs, so the derivative of the output along a coordinate is the same network without biases, applied to the
// derivative of the encoding, under the gates g_l = [h_l > 0] of the value pass:
//     t_1 = g_1 . (W1' dE_d [+ wc[:, d]])    t_2 = g_2 . (W2 t_1)    t_3 = g_3 . (W3 t_2)    jac_d = scale W4 t_3
// forward   the value pass is flownet_fwd_kernel itself, launched by the plain forward call in its training mode: the flows and `saved` are
//           that call's bits by construction.  flownet_jac_fwd_kernel then runs one tangent pass per direction over the same 64-point
//           tiles: layer 1's A fragment is dencode4 (encode4's own e_k / sin, cos, times the analytic factor), the progressive coordinate
//           K group is the unit vector e_d, the epilogue is "gate, no bias" with the gates read from `saved`, layers 2 / 3 are gemm_lds,
//           layer 4 the vector-ALU dot product without b4.  The gated tangents go to tsaved [|D|][3][Npad][256].
// backward  the plain backward call runs unchanged for dflows.  Per direction, in the order t, y, x: flownet_jac_chain_kernel
//           (dt_3 = g_3 . (W4^T scale djac_d), dt_2, dt_1 with the transposed weights the plain call left in its workspace; gW4 partials;
//           gates from the VALUE `saved`; no bias sums), the existing hidden-layer weight gradient on (dt_l, t_{l-1}), and
//           flownet_jac_wgrad_kernel, the layer-1 weight gradient on dencode4, whose column sum of dt_1 is the gradient of the coordinate
//           column d.  Every partial sum goes to the workspace and is reduced in index order by the existing reduce kernels into a
//           scratch gradient, which flownet_jac_add_kernel adds to the call's gradient, one launch a direction: (((value + t) + y) + x), no atomics.
// Rows past N: computed on the clamped point in the forward pass, djac = 0 in the backward pass: exact zeros in every sum.

namespace {

// d / d x_d of features f0 .. f0 + 3 of one point: encode4's loads and arithmetic up to e_k / (sin, cos), then
//   RBF      -2 sigma_k^2 (x_d - c_kd) e_k
//   Fourier  2 pi F[d][f] cos(phi) for feature 2 f (the sine), -2 pi F[d][f] sin(phi) for feature 2 f + 1 (the cosine)
// d is wave-uniform (a kernel argument)
template <int KIND>
__device__ __forceinline__ f32x4 dencode4(const FlowNetDev& q, const Coord c, int f0, int d) {
#pragma clang fp contract(off)
  static_assert(KIND == SININN_FLOWNET_RBF || KIND == SININN_FLOWNET_FOURIER, "the Jacobian exists for RBF and Fourier");
  f32x4 o;
  if constexpr (KIND == SININN_FLOWNET_RBF) {
    const f32x4* cp = reinterpret_cast<const f32x4*>(q.enc_a + 3 * f0);   // centres [512][3]
    const f32x4 c0 = cp[0], c1 = cp[1], c2 = cp[2];
    const f32x4 sg = *reinterpret_cast<const f32x4*>(q.enc_b + f0);
    const float cc[12] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3], c2[0], c2[1], c2[2], c2[3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dt = c.t - cc[3 * j], dy = c.y - cc[3 * j + 1], dx = c.x - cc[3 * j + 2];
      const float dd = fmaf(dx, dx, fmaf(dy, dy, dt * dt));               // encode4's sum
      const float s2 = sg[j] * sg[j];
      const float e = expf(-(dd * s2));
      const float xd = d == 0 ? dt : d == 1 ? dy : dx;
      o[j] = ((-2.f * s2) * e) * xd;
    }
  } else {
    const int f = f0 >> 1;                                                 // frequencies [3][256]
    const f32x2 fa = *reinterpret_cast<const f32x2*>(q.enc_a + f);
    const f32x2 fb = *reinterpret_cast<const f32x2*>(q.enc_a + 256 + f);
    const f32x2 fc = *reinterpret_cast<const f32x2*>(q.enc_a + 512 + f);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float s, co;
      fourier_sincos(c, fa[u], fb[u], fc[u], s, co);                       // the forward pass's own phase
      const float w = FN_TWO_PI * (d == 0 ? fa[u] : d == 1 ? fb[u] : fc[u]);
      o[2 * u] = w * co;
      o[2 * u + 1] = -(w * s);
    }
  }
  return o;
}

// the hidden tile in LDS under the gates of the value pass: v = [gate > 0] v, written to rows [64 tile, 64 tile + 64) of dst and back to
// the tile.  A thread touches the same elements of hs it reads: barriers are the caller's
__device__ __forceinline__ void gate_tile(float* hs, const float* gate, float* dst, int tile, int tid) {
#pragma unroll 4
  for (int u = 0; u < FN_P * FN_HID / 4 / FN_NTHR; ++u) {
    const int f = tid + FN_NTHR * u;
    const int row = f >> 6, c4 = (f & 63) * 4;
    const size_t g = ((size_t)tile * FN_P + row) * FN_HID + c4;
    const f32x4 h = *reinterpret_cast<const f32x4*>(gate + g);
    f32x4 v = *reinterpret_cast<const f32x4*>(hs + row * FN_HS + c4);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = h[j] > 0.f ? v[j] : 0.f;
    *reinterpret_cast<f32x4*>(dst + g) = v;
    *reinterpret_cast<f32x4*>(hs + row * FN_HS + c4) = v;
  }
}

// one tangent pass, direction d: jac [4][N] and tsaved [3][Npad][256] of that direction.  q.saved: the value pass's hidden layers (the
// gates).  PROG: q.w[0] / q.wc / q.ksteps are the packed, mask-folded layer 1 of the value pass
template <int KIND, bool PROG>
__global__ __launch_bounds__(FN_NTHR, 2) void flownet_jac_fwd_kernel(FlowNetDev q, int d, float* jac, float* tsaved) {
  using E = Enc<KIND>;
  constexpr int EW = E::w1_stride(PROG);
  extern __shared__ __attribute__((aligned(16))) float fn_smem[];
  float* const hs = fn_smem;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kq = lane >> 4;
  const int cw = wave * 64;
  const size_t lstride = (size_t)q.ntiles * FN_P * FN_HID;

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    Coord pc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) pc[m] = point_coord(q, tile * FN_P + 16 * m + li);
    f32x4 acc[4][4];
    zero_acc(acc);
    if constexpr (PROG) {
      // the tangent of cat((t, y, x), enc) along d: the unit vector e_d in the coordinate K group
      float a[4], b[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) a[m] = kq == d ? 1.f : 0.f;
#pragma unroll
      for (int n = 0; n < 4; ++n) b[n] = q.wc[(cw + 16 * n + li) * FN_CS + kq];
      mfma_k4(a, b, acc);
    }
    const int ksteps = PROG ? q.ksteps : E::KSTEPS;
#pragma unroll 1
    for (int s = 0; s < ksteps; ++s) {
      f32x4 bf[4], af[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) bf[n] = *reinterpret_cast<const f32x4*>(q.w[0] + (size_t)(cw + 16 * n + li) * EW + 16 * s + 4 * kq);
#pragma unroll
      for (int m = 0; m < 4; ++m) af[m] = dencode4<KIND>(q, pc[m], 16 * s + 4 * kq, d);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m][j], bf[n][j], acc[m][n], 0, 0, 0);
    }
    __syncthreads();                       // the previous tile's layer 4 has read hs
    store_acc(hs, cw, li, kq, acc, Plain{});
    __syncthreads();
    gate_tile(hs, q.saved, tsaved, tile, tid);
    __syncthreads();
#pragma unroll 1
    for (int l = 1; l < 3; ++l) {
      zero_acc(acc);
      gemm_lds(hs, q.w[l], cw, li, kq, acc);
      __syncthreads();                     // every wave has read the whole tile
      store_acc(hs, cw, li, kq, acc, Plain{});
      __syncthreads();
      gate_tile(hs, q.saved + l * lstride, tsaved + l * lstride, tile, tid);
      __syncthreads();
    }
    // ---- layer 4 on the vector ALU, no bias: thread = (channel tid / 64, point tid % 64) ----
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
      if (p < q.N) jac[(size_t)c * q.N + p] = ((a0 + a1) + (a2 + a3)) * q.scale;
    }
  }
}

// the chain of one direction: djac [4][N] of that direction, tsaved its tangents, dt [3][Npad][256] receives dt_1 .. dt_3; gW4 partials
// [block][4][256] to q.part.  q.saved: the VALUE pass's hidden layers (a tangent row may be negative: it is no gate), q.wt: W2^T, W3^T
__global__ __launch_bounds__(FN_NTHR, 2) void flownet_jac_chain_kernel(FlowNetDev q, const float* djac, const float* tsaved, float* dt) {
  extern __shared__ __attribute__((aligned(16))) float fn_smem[];
  float* const hs = fn_smem;
  float* const dos = fn_smem + FN_P * FN_HS;           // [64][4]: scale djac of the tile
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kq = lane >> 4;
  const int cw = wave * 64;
  const size_t lstride = (size_t)q.ntiles * FN_P * FN_HID;

  float w4k[4], gw4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c) w4k[c] = q.w[3][c * FN_HID + tid];

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    __syncthreads();                                   // the previous tile is done with hs / dos
#pragma unroll 4
    for (int u = 0; u < FN_P * FN_HID / 4 / FN_NTHR; ++u) {
      const int f = tid + FN_NTHR * u;
      const int row = f >> 6, c4 = (f & 63) * 4;
      *reinterpret_cast<f32x4*>(hs + row * FN_HS + c4) =
          *reinterpret_cast<const f32x4*>(tsaved + 2 * lstride + ((size_t)tile * FN_P + row) * FN_HID + c4);
    }
    {
      const int c = tid >> 6, pl = tid & 63;
      const int p = tile * FN_P + pl;
      dos[pl * FN_OUT + c] = p < q.N ? djac[(size_t)c * q.N + p] * q.scale : 0.f;
    }
    __syncthreads();
    // gW4 += dout^T t_3;  (dout W4) over the t_3 tile: thread = hidden column tid
#pragma unroll 4
    for (int p = 0; p < FN_P; ++p) {
      const f32x4 dd = *reinterpret_cast<const f32x4*>(dos + p * FN_OUT);
      const float h = hs[p * FN_HS + tid];
      float v = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        gw4[c] = fmaf(dd[c], h, gw4[c]);
        v = fmaf(dd[c], w4k[c], v);
      }
      hs[p * FN_HS + tid] = v;
    }
    __syncthreads();
    gate_tile(hs, q.saved + 2 * lstride, dt + 2 * lstride, tile, tid);
    __syncthreads();
#pragma unroll 1
    for (int l = 1; l >= 0; --l) {
      f32x4 acc[4][4];
      zero_acc(acc);
      gemm_lds(hs, q.wt + (size_t)l * FN_HID * FN_HID, cw, li, kq, acc);
      __syncthreads();
      store_acc(hs, cw, li, kq, acc, Plain{});
      __syncthreads();
      gate_tile(hs, q.saved + l * lstride, dt + l * lstride, tile, tid);
      __syncthreads();
    }
  }
  float* const out = q.part + (size_t)blockIdx.x * (FN_OUT * FN_HID);
#pragma unroll
  for (int c = 0; c < 4; ++c) out[c * FN_HID + tid] = gw4[c];
}

// layer 1 of one direction: part[chunk][j][k] = sum over the chunk's point tiles of dt_1[p][j] dE_d,k(p), flownet_wgrad_kernel's wide tile
// on dencode4; [chunk][256 * KW + j] = sum_p dt_1[p][j], which is the gradient of the coordinate column d (PROG: also written to slot d of
// [chunk][256 * KW + 256 + 4 j + c], zeros in the other slots, the layout flownet_reduce_l1_kernel scatters).  grid = (2 * k tiles, chunks)
template <int KIND, bool PROG>
__global__ __launch_bounds__(FN_NTHR, 2) void flownet_jac_wgrad_kernel(FlowNetDev q, const float* dh, int d) {
  using L = Enc<KIND>;
  static_assert(!L::NARROW, "RBF and Fourier: 512 features");
  constexpr int KF = L::KW;
  constexpr int PSTRIDE = L::part_stride(PROG);
  constexpr int NU = FN_P * FN_WT / 4 / FN_NTHR;       // 16-byte units per thread and operand tile
  extern __shared__ __attribute__((aligned(16))) float fn_smem[];
  float* const as = fn_smem;                           // [64][FN_WS]: dt_1 tile
  float* const bs = fn_smem + FN_P * FN_WS;            // [64][FN_WS]: dE_d tile
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kq = lane >> 4;
  const int j0 = (blockIdx.x & 1) * FN_WT, k0 = (blockIdx.x >> 1) * FN_WT;
  const int jw = (wave & 1) * 64, kw = (wave >> 1) * 64;
  const int chunk = blockIdx.y, nchunks = gridDim.y;

  f32x4 acc[4][4];
  zero_acc(acc);
  float bsum = 0.f;
  f32x4 va[NU];
  auto fetch = [&](int tile) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int f = tid + FN_NTHR * u;
      const int row = f >> 5, c4 = (f & 31) * 4;
      va[u] = *reinterpret_cast<const f32x4*>(dh + ((size_t)tile * FN_P + row) * FN_HID + j0 + c4);
    }
  };
  if (chunk < q.ntiles) fetch(chunk);
  for (int tile = chunk; tile < q.ntiles; tile += nchunks) {
    __syncthreads();                                   // the previous tile's MFMAs have read as / bs
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int f = tid + FN_NTHR * u;
      const int row = f >> 5, c4 = (f & 31) * 4;
      *reinterpret_cast<f32x4*>(as + row * FN_WS + c4) = va[u];
      *reinterpret_cast<f32x4*>(bs + row * FN_WS + c4) = dencode4<KIND>(q, point_coord(q, tile * FN_P + row), k0 + c4, d);
    }
    __syncthreads();
    if (tile + nchunks < q.ntiles) fetch(tile + nchunks);
    if (k0 == 0 && tid < FN_WT) {
      float s = 0.f;
#pragma unroll 8
      for (int p = 0; p < FN_P; ++p) s += as[p * FN_WS + tid];
      bsum += s;
    }
#pragma unroll 2
    for (int ks = 0; ks < FN_P / 4; ++ks) {
      float a[4], b[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) a[m] = as[(4 * ks + kq) * FN_WS + jw + 16 * m + li];
#pragma unroll
      for (int n = 0; n < 4; ++n) b[n] = bs[(4 * ks + kq) * FN_WS + kw + 16 * n + li];
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[n], acc[m][n], 0, 0, 0);
    }
  }
  float* const out = q.part + (size_t)chunk * PSTRIDE;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)(j0 + jw + 16 * m + 4 * kq + r) * KF + k0 + kw + 16 * n + li] = acc[m][n][r];
  if (k0 == 0 && tid < FN_WT) {
    out[FN_HID * KF + j0 + tid] = bsum;
    if constexpr (PROG)
      *reinterpret_cast<f32x4*>(out + FN_HID * KF + FN_HID + (j0 + tid) * FN_CS) =
          (f32x4){d == 0 ? bsum : 0.f, d == 1 ? bsum : 0.f, d == 2 ? bsum : 0.f, 0.f};
  }
}

// a direction's four scratch gradients onto the call's, one launch: dst_l[i] = dst_l[i] + src_l[i], one rounded sum per element
struct JacAdd {
  float* dst[4];
  const float* src[4];
  int n[4];
};
__global__ __launch_bounds__(FN_NTHR) void flownet_jac_add_kernel(JacAdd a) {
  int i = blockIdx.x * FN_NTHR + threadIdx.x;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    if (i < a.n[l]) { a.dst[l][i] = a.dst[l][i] + a.src[l][i]; return; }
    i -= a.n[l];
  }
}

constexpr size_t JAC_GW1 = (size_t)FN_HID * (FN_GW + 1);   // the scratch gradient of layer 1, rows of 515 rounded up to a multiple of four floats
constexpr size_t JAC_SCRATCH = JAC_GW1 + FN_HID + 2 * (size_t)FN_HID * FN_HID + FN_OUT * FN_HID;

int jac_ndirs(unsigned dirs) { return (int)((dirs & 1u) + ((dirs >> 1) & 1u) + ((dirs >> 2) & 1u)); }

}  // namespace

extern "C" size_t sininn_flownet_jacobian_saved_bytes(int64_t n, int n_dirs) {
  if (n <= 0 || n_dirs < 1 || n_dirs > FN_DOM) return 0;
  return (size_t)n_dirs * sininn_flownet_saved_bytes(n);
}

// dt [3][Npad][256], the partial sums of one launch, one scratch gradient per layer: the directions run one after the other
extern "C" size_t sininn_flownet_jacobian_workspace_bytes(const sininn_flownet_args* a, int64_t n, int n_dirs) {
  if (a == nullptr || a->struct_bytes != sizeof(sininn_flownet_args)) return 0;
  if (n <= 0 || n > ((int64_t)1 << 22) || n_dirs < 1 || n_dirs > FN_DOM) return 0;
  const int ntiles = (int)((n + FN_P - 1) / FN_P);
  return sininn_flownet_saved_bytes(n) + (part_floats(ntiles) + JAC_SCRATCH) * sizeof(float);
}

// the head of both entry points: the direction set, the call descriptor as this feature takes it, then the network.  Every refusal is one
// sentence under the entry point's own name, before any launch
static int jac_check_head(const sininn_flownet_args* a, const sininn_flownet_call* call, unsigned dirs, const char* who, CallKind kind, Call& c) {
  SININN_CHECK(dirs >= 1u && dirs <= 7u, "%s: dirs 0x%x: a non-empty set of bit 0 (t), bit 1 (y), bit 2 (x)", who, dirs);
  SININN_CHECK(call != nullptr, "%s: null call descriptor: the Jacobian is evaluated at a pose list (AT_POINTS)", who);
  SININN_CHECK(call->struct_bytes == sizeof(sininn_flownet_call), "%s: call descriptor: struct_bytes is %zu, this library was built with %zu", who,
               call->struct_bytes, sizeof(sininn_flownet_call));
  const unsigned known = SININN_FLOWNET_AT_POINTS | SININN_FLOWNET_SPATIAL | SININN_FLOWNET_ENCGRAD | SININN_FLOWNET_POSEGRAD;
  SININN_CHECK((call->mode & ~known) == 0, "%s: call descriptor: unknown mode bits 0x%x (AT_POINTS 1, SPATIAL 2, ENCGRAD 4, POSEGRAD 8)", who,
               call->mode & ~known);
  SININN_CHECK(!(call->mode & SININN_FLOWNET_SPATIAL), "%s: SPATIAL: a per-point mask is out of scope for the Jacobian (global masks only)", who);
  SININN_CHECK(!(call->mode & SININN_FLOWNET_ENCGRAD),
               "%s: ENCGRAD: learnable frequencies would need the second derivative of the encoding, which no kernel evaluates", who);
  SININN_CHECK(!(call->mode & SININN_FLOWNET_POSEGRAD), "%s: POSEGRAD: there is no gradient to the poses through the Jacobian", who);
  SININN_CHECK(call->domain_dim == 3, "%s: domain_dim %d: the Jacobian kernels take three coordinates per point (t, y, x)", who, call->domain_dim);
  SININN_CHECK(call->mode & SININN_FLOWNET_AT_POINTS, "%s: without AT_POINTS: the Jacobian is evaluated at a pose list", who);
  if (int rc = check_call(call, "flownet", kind, c)) return rc;
  if (int rc = check_head(a, who, nullptr)) return rc;
  SININN_CHECK(a->encoding == SININN_FLOWNET_RBF || a->encoding == SININN_FLOWNET_FOURIER,
               "%s: encoding %d: the Jacobian kernels exist for SININN_FLOWNET_RBF and SININN_FLOWNET_FOURIER (RBFG, PE and PieceWise are out of scope)",
               who, a->encoding);
  SININN_CHECK(c.points.n >= 1 && c.points.n <= (int64_t)1 << 22, "%s: %lld points (1 .. 2^22)", who, (long long)c.points.n);
  return 0;
}

// f(KIND, PROG) for a network jac_check_head has accepted
template <class F>
static int for_jac(const sininn_flownet_args* a, F&& f) {
  if (a->encoding == SININN_FLOWNET_RBF)
    return a->progressive ? f(std::integral_constant<int, SININN_FLOWNET_RBF>{}, std::true_type{})
                          : f(std::integral_constant<int, SININN_FLOWNET_RBF>{}, std::false_type{});
  return a->progressive ? f(std::integral_constant<int, SININN_FLOWNET_FOURIER>{}, std::true_type{})
                        : f(std::integral_constant<int, SININN_FLOWNET_FOURIER>{}, std::false_type{});
}

extern "C" int sininn_flownet_jacobian_forward(const sininn_flownet_args* a, const sininn_flownet_call* call, unsigned dirs, float* jac,
                                               float* tsaved, size_t tsaved_bytes, void* stream) {
  hipStream_t st = ST(stream);
  const char* const who = "flownet_jacobian_forward";
  Call c;
  if (int rc = jac_check_head(a, call, dirs, who, CALL_FORWARD, c)) return rc;
  const int nd = jac_ndirs(dirs);
  SININN_CHECK(jac != nullptr && tsaved != nullptr, "%s: null jac / tsaved", who);
  SININN_CHECK(tsaved_bytes >= sininn_flownet_jacobian_saved_bytes(c.points.n, nd), "%s: tsaved holds %zu bytes, %zu needed", who, tsaved_bytes,
               sininn_flownet_jacobian_saved_bytes(c.points.n, nd));
  SININN_CHECK(aligned16(tsaved) && ((uintptr_t)jac & 3u) == 0, "%s: tsaved must be 16-byte aligned, jac 4-byte aligned", who);
  SININN_CHECK(a->saved != nullptr, "%s: null saved: the tangent passes take their gates from the value pass's hidden layers", who);
  FlowNetDev q;
  if (int rc = fill_args(a, who, q, nullptr, c.pl())) return rc;
  if (int rc = check_forward_buffers(a, "flownet_forward", sininn_flownet_saved_bytes(q.N), q)) return rc;
  if (a->progressive) {
    SININN_CHECK(a->workspace != nullptr && a->workspace_bytes >= sininn_flownet_forward_workspace_bytes(a),
                 "%s: the progressive forward packs W1 into a workspace of %zu bytes, %zu given", who, sininn_flownet_forward_workspace_bytes(a),
                 a->workspace ? a->workspace_bytes : (size_t)0);
    SININN_CHECK(aligned16(a->workspace), "%s: workspace must be 16-byte aligned", who);
  }
  // every host check of the plain call has passed; what can still fail does so here, before anything is written
  if (int rc = for_jac(a, [&](auto k, auto prog) { return raise_lds(flownet_jac_fwd_kernel<decltype(k)::value, decltype(prog)::value>, tile_lds(false), who); }))
    return rc;
  // the value pass: the plain training-mode call, with its own checks in front of its launches.  Nothing below it refuses
  if (int rc = sininn_flownet_forward(a, call, st)) return rc;
  const size_t lstride = (size_t)q.ntiles * FN_P * FN_HID;
  return for_jac(a, [&](auto k, auto prog) {
    constexpr int KIND = decltype(k)::value;
    constexpr bool PROG = decltype(prog)::value;
    using E = Enc<KIND>;
    if constexpr (PROG) {                              // the pack the value pass has just made
      float* const w1p = static_cast<float*>(a->workspace);
      q.w[0] = w1p;
      q.wc = w1p + (size_t)FN_HID * E::KW;
      q.ksteps = (open_encoded(a) + 15) / 16;
    }
    auto kern = flownet_jac_fwd_kernel<KIND, PROG>;
    const int blocks = q.ntiles < FN_FWD_MAX_BLOCKS ? q.ntiles : FN_FWD_MAX_BLOCKS;
    int slot = 0;
    for (int d = 0; d < FN_DOM; ++d) {
      if (!(dirs >> d & 1u)) continue;
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(FN_NTHR), tile_lds(false), st, q, d, jac + (size_t)slot * FN_OUT * q.N,
                         tsaved + (size_t)slot * 3 * lstride);
      SININN_LAUNCH_CHECK("flownet_jac_fwd");
      ++slot;
    }
    return 0;
  });
}

extern "C" int sininn_flownet_jacobian_backward(const sininn_flownet_args* a, const sininn_flownet_call* call, unsigned dirs, const float* djac,
                                                const float* tsaved, size_t tsaved_bytes, void* jac_workspace, size_t jac_workspace_bytes,
                                                void* stream) {
  hipStream_t st = ST(stream);
  const char* const who = "flownet_jacobian_backward";
  Call c;
  if (int rc = jac_check_head(a, call, dirs, who, CALL_BACKWARD, c)) return rc;
  const int nd = jac_ndirs(dirs);
  SININN_CHECK(djac != nullptr && tsaved != nullptr && jac_workspace != nullptr, "%s: null djac / tsaved / jac_workspace", who);
  SININN_CHECK(tsaved_bytes >= sininn_flownet_jacobian_saved_bytes(c.points.n, nd), "%s: tsaved holds %zu bytes, %zu needed", who, tsaved_bytes,
               sininn_flownet_jacobian_saved_bytes(c.points.n, nd));
  SININN_CHECK(jac_workspace_bytes >= sininn_flownet_jacobian_workspace_bytes(a, c.points.n, nd), "%s: jac_workspace holds %zu bytes, %zu needed", who,
               jac_workspace_bytes, sininn_flownet_jacobian_workspace_bytes(a, c.points.n, nd));
  SININN_CHECK(aligned16(tsaved) && aligned16(jac_workspace) && ((uintptr_t)djac & 3u) == 0,
               "%s: tsaved / jac_workspace must be 16-byte aligned, djac 4-byte aligned", who);
  SININN_CHECK(a->saved != nullptr, "%s: null saved: the gates are the value pass's hidden layers", who);
  {                                                    // the plain call's own host checks, ahead of the LDS limits: nothing is written before both
    FlowNetDev probe;
    if (int rc = fill_args(a, "flownet_backward_points", probe, nullptr, c.pl())) return rc;
    if (int rc = check_backward_buffers<4>(a, "flownet_backward_points", sininn_flownet_saved_bytes(probe.N), sininn_flownet_workspace_bytes(probe.N), probe)) return rc;
  }
  if (raise_lds(flownet_jac_chain_kernel, tile_lds(false), who)) return 1;
  if (int rc = for_jac(a, [&](auto k, auto prog) { return raise_lds(flownet_jac_wgrad_kernel<decltype(k)::value, decltype(prog)::value>, FN_WG_LDS, who); }))
    return rc;
  // the plain backward for dflows, unchanged, with its own checks in front of its launches; q: its descriptor (saved, W2^T / W3^T in its
  // workspace).  Nothing below it refuses
  FlowNetDev q;
  if (int rc = backward_launch(a, c, nullptr, st, &q)) return rc;
  const size_t lstride = (size_t)q.ntiles * FN_P * FN_HID;
  float* const dt = static_cast<float*>(jac_workspace);
  float* const part = dt + 3 * lstride;
  float* const gw1 = part + part_floats(q.ntiles);
  float* const gbx = gw1 + JAC_GW1;                    // the bias sums the shared kernels make on the way: not a gradient of anything
  float* const gw2 = gbx + FN_HID;
  float* const gw3 = gw2 + (size_t)FN_HID * FN_HID;
  float* const gw4 = gw3 + (size_t)FN_HID * FN_HID;
  q.part = part;
  const int cb = chain_blocks(q.ntiles);
  int slot = 0;
  for (int d = 0; d < FN_DOM; ++d) {
    if (!(dirs >> d & 1u)) continue;
    const float* const ts = tsaved + (size_t)slot * 3 * lstride;
    hipLaunchKernelGGL(flownet_jac_chain_kernel, dim3(cb), dim3(FN_NTHR), tile_lds(false), st, q, djac + (size_t)slot * FN_OUT * q.N, ts, dt);
    SININN_LAUNCH_CHECK("flownet_jac_chain");
    reduce_launch(q, cb, FN_OUT * FN_HID, 0, gw4, gbx, st);
    SININN_LAUNCH_CHECK("flownet_reduce");
    if (int rc = hidden_wgrad_launch(q.ntiles, dt + 2 * lstride, ts + lstride, part, gw3, gbx, st)) return rc;
    if (int rc = hidden_wgrad_launch(q.ntiles, dt + lstride, ts, part, gw2, gbx, st)) return rc;
    const int rc = for_jac(a, [&](auto k, auto prog) {
      constexpr int KIND = decltype(k)::value;
      constexpr bool PROG = decltype(prog)::value;
      using E = Enc<KIND>;
      auto kern = flownet_jac_wgrad_kernel<KIND, PROG>;
      const int nc = wgrad_chunks(q.ntiles, E::CHUNK_KF);
      const int oe = open_encoded(a);
      const int ktiles = PROG ? (oe > 0 ? (oe + FN_WT - 1) / FN_WT : 1) : E::KW / E::KT;   // the open 128-column tiles, as in the plain call
      hipLaunchKernelGGL(kern, dim3(2 * ktiles, nc), dim3(FN_NTHR), FN_WG_LDS, st, q, (const float*)dt, d);
      SININN_LAUNCH_CHECK("flownet_jac_wgrad");
      if constexpr (PROG) {
        hipLaunchKernelGGL((flownet_reduce_l1_kernel<E::KW, E::LIVE, true, FN_DOM>), dim3((FN_HID * E::width(true) + FN_HID + FN_NTHR - 1) / FN_NTHR),
                           dim3(FN_NTHR), 0, st, (const float*)part, nc, a->mask, ktiles * FN_WT, gw1, gbx);
      } else {
        reduce_launch(q, nc, FN_HID * E::LIVE, FN_HID, gw1, gbx, st);
      }
      SININN_LAUNCH_CHECK("flownet_reduce");
      return 0;
    });
    if (rc) return rc;
    const JacAdd ja = {{a->gw[0], a->gw[1], a->gw[2], a->gw[3]}, {gw1, gw2, gw3, gw4},
                       {FN_HID * a->enc_dim, FN_HID * FN_HID, FN_HID * FN_HID, FN_OUT * FN_HID}};
    const int total = ja.n[0] + ja.n[1] + ja.n[2] + ja.n[3];
    hipLaunchKernelGGL(flownet_jac_add_kernel, dim3((total + FN_NTHR - 1) / FN_NTHR), dim3(FN_NTHR), 0, st, ja);
    SININN_LAUNCH_CHECK("flownet_jac_add");
    ++slot;
  }
  return 0;
}
