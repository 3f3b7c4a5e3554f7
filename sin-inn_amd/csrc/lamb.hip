// LAMB as apex.optimizers.FusedLAMB states it (multi_tensor_lamb stages 1 and 2), the optimiser of the flow trainer
// (video-interpolation/trainer.py:134-135).  The formula block is in include/sininn.h; DESIGN 15 has the launch plan.
//
// Work is cut into CHUNKS, listed by the host once: (tensor, begin, len) with begin a multiple of 4 and no chunk crossing a tensor
// or touching padding.  One block works on one chunk at a time (float4 body, scalar tail).  Every sum -- the global gradient norm,
// the per-tensor norms of p and of the update -- is a per-chunk partial (a double) written to the workspace and then added in chunk-index order
// by a fixed thread assignment: no floating-point atomics, and the grid size never enters a result.
#include "common.h"

namespace sininn {

namespace {

constexpr int LAMB_THREADS = 256;
constexpr int LAMB_MAX_BLOCKS = 2048;

struct LambChunk { int64_t tensor, begin, len; };

// fp32 images of the double hyper-parameters; beta3, 1 - beta2 and the bias corrections are formed in double on the host first
// (1 - 0.999f in fp32 is off by 1.3e-5 relative)
struct LambHyper {
  float beta1, beta2, beta3, omb2, eps, wd, max_grad_norm, gscale, bc1, bc2;
  int adam_w_mode, always_adapt;   // always_adapt = use_nvlamb
};

static inline size_t pad4(size_t x) { return (x + 3) / 4 * 4; }

// workspace: ratio[pad4(n_tensors)] floats, then three arrays of pad2(n_chunks) doubles: gpart | ppart | upart
struct LambWs { float* ratio; double *gpart, *ppart, *upart; };
static inline size_t pad2(size_t x) { return (x + 1) / 2 * 2; }
static inline LambWs lamb_ws(void* ws, int64_t n_chunks, int n_tensors) {
  float* f = static_cast<float*>(ws);
  double* d = reinterpret_cast<double*>(f + pad4((size_t)n_tensors));
  const size_t nc = pad2((size_t)n_chunks);
  return LambWs{f, d, d + nc, d + 2 * nc};
}

// Block sums are block_sum_f64 (common.h).  Sums of squares are carried in double from the first addition on: two double FMAs per
// element are free next to five fp32 streams, and a norm is then the norm of the fp32 values themselves, whatever the tensor's size.
static_assert(LAMB_THREADS == 256, "block_sum_f64 adds four waves");

// part[lo .. hi) added in index order: thread j takes lo + j, lo + j + 256, ..., then block_sum_f64.
__device__ __forceinline__ double ordered_sum(const double* __restrict__ part, int64_t lo, int64_t hi, double* lds) {
  double acc = 0.0;
  for (int64_t c = lo + threadIdx.x; c < hi; c += LAMB_THREADS) acc += part[c];
  return block_sum_f64(acc, lds);
}

// The chunk table is device data the library cannot read on the host: a chunk that does not lie inside its tensor, inside the
// buffers, on a 16-byte boundary, is skipped by every kernel (block-uniform test), so a bad table cannot write out of bounds.
__device__ __forceinline__ bool chunk_ok(const LambChunk& c, const int64_t* __restrict__ toff, int n_tensors, int64_t n) {
  if (c.tensor < 0 || c.tensor >= n_tensors || c.len <= 0 || c.begin < 0 || (c.begin & 3)) return false;
  const int64_t lo = toff[c.tensor], hi = toff[c.tensor + 1];
  return lo >= 0 && hi <= n && c.begin >= lo && c.len <= hi - c.begin;
}

__global__ __launch_bounds__(LAMB_THREADS) void lamb_gradnorm_kernel(const float* __restrict__ g, const LambChunk* __restrict__ chunks,
                                                                     int64_t n_chunks, const int64_t* __restrict__ toff, int n_tensors,
                                                                     int64_t n, float gscale, double* __restrict__ gpart) {
  __shared__ double lds[4];
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const LambChunk ch = chunks[c];
    double acc = 0.0;
    if (chunk_ok(ch, toff, n_tensors, n)) {
      const float* gc = g + ch.begin;
      const int n4 = (int)(ch.len >> 2), len = (int)ch.len;
      for (int i = threadIdx.x; i < n4; i += LAMB_THREADS) {
        const f32x4 x = reinterpret_cast<const f32x4*>(gc)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const double s = (double)(gscale * x[k]); acc += s * s; }
      }
      for (int i = (n4 << 2) + threadIdx.x; i < len; i += LAMB_THREADS) { const double s = (double)(gscale * gc[i]); acc += s * s; }
    }
    acc = block_sum_f64(acc, lds);
    if (threadIdx.x == 0) gpart[c] = acc;
  }
}

// one block: this group's sum of squares -> its slot (rounded to fp32 once)
__global__ __launch_bounds__(LAMB_THREADS) void lamb_gradnorm_finish_kernel(const double* __restrict__ gpart, int64_t n_chunks,
                                                                            float* __restrict__ slot) {
  __shared__ double lds[4];
  const double s = ordered_sum(gpart, 0, n_chunks, lds);
  if (threadIdx.x == 0) *slot = (float)s;
}

__global__ __launch_bounds__(LAMB_THREADS) void lamb_stage1_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                                   float* __restrict__ m, float* __restrict__ v, float* __restrict__ u,
                                                                   const LambChunk* __restrict__ chunks, int64_t n_chunks,
                                                                   const int64_t* __restrict__ toff, int n_tensors, int64_t n,
                                                                   const float* __restrict__ slots, int n_groups, LambHyper h,
                                                                   double* __restrict__ ppart, double* __restrict__ upart) {
  __shared__ double lds[4];
  double total = 0.0;
  for (int k = 0; k < n_groups; ++k) total += (double)slots[k];
  const double G = sqrt(total);
  const float clip = (h.max_grad_norm > 0.f && G > (double)h.max_grad_norm) ? (float)(G / (double)h.max_grad_norm) : 1.f;
  double up2 = 0.0, uu2 = 0.0;
  // the formula block of include/sininn.h operation by operation, each rounded to fp32 once (no contraction into FMAs): the update is
  // then what an fp32 evaluation of the formulas with IEEE operations gives, bit for bit
  auto upd = [&](float pv, float gv, float& mv, float& vv) -> float {
#pragma clang fp contract(off)
    float sg = (h.gscale * gv) / clip;
    if (!h.adam_w_mode) sg = sg + h.wd * pv;
    mv = h.beta1 * mv + h.beta3 * sg;
    vv = h.beta2 * vv + (h.omb2 * sg) * sg;
    float uv = (mv / h.bc1) / (sqrtf(vv / h.bc2) + h.eps);
    if (h.adam_w_mode) uv = uv + h.wd * pv;
    up2 += (double)pv * (double)pv;
    uu2 += (double)uv * (double)uv;
    return uv;
  };
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const LambChunk ch = chunks[c];
    up2 = 0.0; uu2 = 0.0;
    if (chunk_ok(ch, toff, n_tensors, n)) {
      const float* pc = p + ch.begin; const float* gc = g + ch.begin;
      float* mc = m + ch.begin; float* vc = v + ch.begin; float* uc = u + ch.begin;
      const int n4 = (int)(ch.len >> 2), len = (int)ch.len;
      for (int i = threadIdx.x; i < n4; i += LAMB_THREADS) {
        const f32x4 pv = reinterpret_cast<const f32x4*>(pc)[i], gv = reinterpret_cast<const f32x4*>(gc)[i];
        f32x4 mv = reinterpret_cast<f32x4*>(mc)[i], vv = reinterpret_cast<f32x4*>(vc)[i], uv;
#pragma unroll
        for (int k = 0; k < 4; ++k) { float a = mv[k], b = vv[k]; uv[k] = upd(pv[k], gv[k], a, b); mv[k] = a; vv[k] = b; }
        reinterpret_cast<f32x4*>(mc)[i] = mv; reinterpret_cast<f32x4*>(vc)[i] = vv; reinterpret_cast<f32x4*>(uc)[i] = uv;
      }
      for (int i = (n4 << 2) + threadIdx.x; i < len; i += LAMB_THREADS) uc[i] = upd(pc[i], gc[i], mc[i], vc[i]);
    }
    const double sp = block_sum_f64(up2, lds), su = block_sum_f64(uu2, lds);
    if (threadIdx.x == 0) { ppart[c] = sp; upart[c] = su; }
  }
}

// first chunk whose tensor index is >= t (the table is sorted by tensor)
__device__ __forceinline__ int64_t first_chunk_of(const LambChunk* __restrict__ chunks, int64_t n_chunks, int64_t t) {
  int64_t lo = 0, hi = n_chunks;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (chunks[mid].tensor < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one block per tensor: ratio = lr * |p| / |u|, or lr
__global__ __launch_bounds__(LAMB_THREADS) void lamb_ratio_kernel(const LambChunk* __restrict__ chunks, int64_t n_chunks,
                                                                  const double* __restrict__ ppart, const double* __restrict__ upart,
                                                                  double lr, int adapt, float* __restrict__ ratio) {
  __shared__ double lds[4];
  const int64_t t = blockIdx.x;
  const int64_t lo = first_chunk_of(chunks, n_chunks, t), hi = first_chunk_of(chunks, n_chunks, t + 1);
  const double pn = sqrt(ordered_sum(ppart, lo, hi, lds)), un = sqrt(ordered_sum(upart, lo, hi, lds));
  if (threadIdx.x == 0) ratio[t] = (adapt && pn != 0.0 && un != 0.0) ? (float)(lr * (pn / un)) : (float)lr;
}

__global__ __launch_bounds__(LAMB_THREADS) void lamb_stage2_kernel(float* __restrict__ p, const float* __restrict__ u,
                                                                   const LambChunk* __restrict__ chunks, int64_t n_chunks,
                                                                   const int64_t* __restrict__ toff, int n_tensors, int64_t n,
                                                                   const float* __restrict__ ratio) {
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const LambChunk ch = chunks[c];
    if (!chunk_ok(ch, toff, n_tensors, n)) continue;
    const float r = ratio[ch.tensor];
    float* pc = p + ch.begin; const float* uc = u + ch.begin;
    const int n4 = (int)(ch.len >> 2), len = (int)ch.len;
    for (int i = threadIdx.x; i < n4; i += LAMB_THREADS) {
      f32x4 pv = reinterpret_cast<f32x4*>(pc)[i];
      const f32x4 uv = reinterpret_cast<const f32x4*>(uc)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) pv[k] = pv[k] - r * uv[k];
      reinterpret_cast<f32x4*>(pc)[i] = pv;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < len; i += LAMB_THREADS) pc[i] -= r * uc[i];
  }
}

int lamb_check(const sininn_lamb_args* a, const char* who) {
  SININN_CHECK(a != nullptr, "%s: null descriptor", who);
  SININN_CHECK(a->struct_bytes == sizeof(sininn_lamb_args), "%s: struct_bytes is %zu, this library's sininn_lamb_args has %zu", who,
               a->struct_bytes, sizeof(sininn_lamb_args));
  SININN_CHECK(a->p && a->g && a->m && a->v && a->u && a->chunks && a->tensor_offsets && a->norm_slots && a->workspace,
               "%s: null pointer in the descriptor", who);
  SININN_CHECK(aligned16(a->p) && aligned16(a->g) && aligned16(a->m) && aligned16(a->v) && aligned16(a->u) && aligned16(a->workspace),
               "%s: buffers and workspace must be 16-byte aligned", who);
  SININN_CHECK((reinterpret_cast<uintptr_t>(a->chunks) & 7u) == 0 && (reinterpret_cast<uintptr_t>(a->tensor_offsets) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(a->norm_slots) & 3u) == 0, "%s: misaligned table pointer", who);
  SININN_CHECK(a->n > 0 && a->n % 4 == 0, "%s: n must be a positive multiple of 4 (got %lld)", who, (long long)a->n);
  SININN_CHECK(a->n_tensors > 0 && a->n_chunks > 0, "%s: n_tensors and n_chunks must be positive", who);
  SININN_CHECK(a->n_chunks >= a->n_tensors && a->n_chunks <= a->n, "%s: n_chunks %lld does not fit %d tensors in %lld elements", who,
               (long long)a->n_chunks, a->n_tensors, (long long)a->n);
  SININN_CHECK(a->step >= 1, "%s: step must be >= 1 (got %d)", who, a->step);
  SININN_CHECK(a->n_groups >= 1 && a->n_groups <= 4096 && a->group >= 0 && a->group < a->n_groups,
               "%s: group index %d outside 0..%d", who, a->group, a->n_groups - 1);
  const size_t need = sininn_lamb_workspace_bytes(a->n_chunks, a->n_tensors);
  SININN_CHECK(a->workspace_bytes >= need, "%s: workspace holds %zu bytes, needs %zu", who, a->workspace_bytes, need);
  return 0;
}

static inline int lamb_grid(int64_t n_chunks) { return (int)(n_chunks < LAMB_MAX_BLOCKS ? n_chunks : LAMB_MAX_BLOCKS); }

}  // namespace

extern "C" size_t sininn_lamb_workspace_bytes(int64_t n_chunks, int n_tensors) {
  if (n_chunks <= 0 || n_tensors <= 0) return 0;
  return pad4((size_t)n_tensors) * sizeof(float) + 3 * pad2((size_t)n_chunks) * sizeof(double);
}

extern "C" int sininn_lamb_grad_norm(const sininn_lamb_args* a, void* stream) {
  hipStream_t st = ST(stream);
  if (int rc = lamb_check(a, "lamb_grad_norm")) return rc;
  const LambWs ws = lamb_ws(a->workspace, a->n_chunks, a->n_tensors);
  const LambChunk* chunks = reinterpret_cast<const LambChunk*>(a->chunks);
  hipLaunchKernelGGL(lamb_gradnorm_kernel, dim3(lamb_grid(a->n_chunks)), dim3(LAMB_THREADS), 0, st, a->g, chunks, a->n_chunks,
                     a->tensor_offsets, a->n_tensors, a->n, (float)a->grad_scale, ws.gpart);
  SININN_LAUNCH_CHECK("lamb_gradnorm");
  hipLaunchKernelGGL(lamb_gradnorm_finish_kernel, dim3(1), dim3(LAMB_THREADS), 0, st, ws.gpart, a->n_chunks, a->norm_slots + a->group);
  SININN_LAUNCH_CHECK("lamb_gradnorm_finish");
  return 0;
}

extern "C" int sininn_lamb_step(const sininn_lamb_args* a, void* stream) {
  hipStream_t st = ST(stream);
  if (int rc = lamb_check(a, "lamb_step")) return rc;
  const LambWs ws = lamb_ws(a->workspace, a->n_chunks, a->n_tensors);
  const LambChunk* chunks = reinterpret_cast<const LambChunk*>(a->chunks);
  LambHyper h;
  h.beta1 = (float)a->beta1; h.beta2 = (float)a->beta2; h.eps = (float)a->eps; h.wd = (float)a->weight_decay;
  h.beta3 = a->grad_averaging ? (float)(1.0 - a->beta1) : 1.f;
  h.omb2 = (float)(1.0 - a->beta2);
  h.max_grad_norm = (float)a->max_grad_norm; h.gscale = (float)a->grad_scale;
  h.bc1 = a->bias_correction ? (float)(1.0 - pow(a->beta1, (double)a->step)) : 1.f;
  h.bc2 = a->bias_correction ? (float)(1.0 - pow(a->beta2, (double)a->step)) : 1.f;
  h.adam_w_mode = a->adam_w_mode != 0; h.always_adapt = a->use_nvlamb != 0;
  const int grid = lamb_grid(a->n_chunks);
  hipLaunchKernelGGL(lamb_stage1_kernel, dim3(grid), dim3(LAMB_THREADS), 0, st, a->p, a->g, a->m, a->v, a->u, chunks, a->n_chunks,
                     a->tensor_offsets, a->n_tensors, a->n, a->norm_slots, a->n_groups, h, ws.ppart, ws.upart);
  SININN_LAUNCH_CHECK("lamb_stage1");
  const int adapt = h.always_adapt || h.wd != 0.f;
  hipLaunchKernelGGL(lamb_ratio_kernel, dim3(a->n_tensors), dim3(LAMB_THREADS), 0, st, chunks, a->n_chunks, ws.ppart, ws.upart, a->lr,
                     adapt, ws.ratio);
  SININN_LAUNCH_CHECK("lamb_ratio");
  hipLaunchKernelGGL(lamb_stage2_kernel, dim3(grid), dim3(LAMB_THREADS), 0, st, a->p, a->u, chunks, a->n_chunks, a->tensor_offsets,
                     a->n_tensors, a->n, ws.ratio);
  SININN_LAUNCH_CHECK("lamb_stage2");
  return 0;
}

}  // namespace sininn
