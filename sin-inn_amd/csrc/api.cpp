// What of the extern "C" surface of libsininn.so (include/sininn.h) belongs to no kernel file: the error string, version and
// struct sizes, streams and capture diagnostics, and the test hooks that switch kernels of several files at once.  Every
// other entry point is defined beside its kernels.
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

}  // namespace sininn

using namespace sininn;

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

void sininn_coupling_colmap(int Co, int tile, int* colmap_host) {
  const int w = (tile == 32) ? 32 : 16, h = w / 2;
  for (int q = 0; q < 2 * Co; ++q) {
    const int t = q / w, j = q % w;
    colmap_host[q] = (j < h) ? (t * h + j) : (Co + t * h + j - h);
  }
}

int sininn_wall_clock_khz(void) {
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return 0;
  return khz;
}

// test hook: the block executor's fused 1x1 subnet backward on / off (A/B against the pair + grouped weight-gradient path)
void sininn_sub1_bwd_test_hook(int on) { conv_sub1_bwd_enable(on); conv3_smallk_enable(on); }   // every round-4 persistent kernel on / off
// bit 0: fused 1x1 pairs on; bit 2: force the fused 3x3 subnet on, bit 1: force it off, neither: its default policy (SININN_SUB3)
void sininn_pair_k1_test_hook(int on) { conv_pair_k1_enable(on & 1); sub3_fusion_set((on & 4) ? 1 : ((on & 2) ? 0 : -1)); }

}  // extern "C"
