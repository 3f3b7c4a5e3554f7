// The error of the device expf on a list of fp32 arguments, in ulps of the result, against the double exp of the host.
//   hipcc -O3 --offload-arch=gfx950 tools/expf_ulp.hip -o tools/expf_ulp
//   python tests/flowsynth_stage_refs.py ARGS.f32 && tools/expf_ulp ARGS.f32
// Compiled like csrc/ (no fast-math), so `expf` is the function flowsynth_scatter_kernel calls.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#define CHECK(e)                                                                   \
  do {                                                                             \
    hipError_t err_ = (e);                                                         \
    if (err_ != hipSuccess) {                                                      \
      std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_));               \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

__global__ void expf_kernel(const float* __restrict__ in, float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = expf(in[i]);
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: expf_ulp ARGS.f32\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  std::vector<float> x;
  float buf[4096];
  for (size_t got; (got = std::fread(buf, sizeof(float), 4096, f)) > 0;) x.insert(x.end(), buf, buf + got);
  std::fclose(f);
  const int n = (int)x.size();
  if (n == 0) { std::fprintf(stderr, "no arguments\n"); return 2; }
  float *din = nullptr, *dout = nullptr;
  CHECK(hipMalloc(&din, n * sizeof(float)));
  CHECK(hipMalloc(&dout, n * sizeof(float)));
  CHECK(hipMemcpy(din, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(expf_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, din, dout, n);
  CHECK(hipGetLastError());
  std::vector<float> y(n);
  CHECK(hipMemcpy(y.data(), dout, n * sizeof(float), hipMemcpyDeviceToHost));
  double worst = 0, lo = x[0], hi = x[0];
  float at = x[0];
  for (int i = 0; i < n; ++i) {
    const double want = std::exp((double)x[i]);
    int e;
    std::frexp(want, &e);                                   // want = m 2^e, m in [0.5, 1): one fp32 ulp is 2^(e - 24)
    const double ulps = std::fabs((double)y[i] - want) / std::ldexp(1.0, e - 24);
    if (!(ulps <= worst)) { worst = ulps; at = x[i]; }
    lo = std::fmin(lo, x[i]); hi = std::fmax(hi, x[i]);
  }
  std::printf("expf: %d arguments in [%.6g, %.6g], worst error %.4f ulp at %.9g\n", n, lo, hi, worst, (double)at);
  CHECK(hipFree(din));
  CHECK(hipFree(dout));
  return 0;
}
