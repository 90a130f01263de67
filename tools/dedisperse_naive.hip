// The naive dedispersion the tiled kernel of csrc/bf_dedisperse.hip is measured against (tools/bench_ops.py
// --dedisperse): one thread per output element (m, d, n), n fastest, walking the K channels and reading the ring
// directly.  Same contract as step 2 of bf_dedisperse (float64 sum, channels ascending, lags clamped), no append.  A
// measurement library of its own (build/libbf_dedisperse_naive.so, `make dedisperse-naive`), never linked into the
// product.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

__global__ __launch_bounds__(256) void dedisperse_naive_kernel(const float* ring, const int32_t* lags, float* out, int K,
                                                               int M, int D, int N, int R, int head, double scale) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<long long>(M) * D * N) return;
  const int n = static_cast<int>(i % N), d = static_cast<int>(i / N % D), m = static_cast<int>(i / N / D);
  double acc = 0.0;
  for (int k = 0; k < K; ++k) {
    int lag = lags[static_cast<long long>(d) * K + k];
    lag = lag < 0 ? 0 : (lag > R - N ? R - N : lag);
    int slot = head + n - lag;
    if (slot < 0) slot += R;
    acc += static_cast<double>(ring[(static_cast<long long>(k) * R + slot) * M + m]);
  }
  out[i] = static_cast<float>(acc * scale);
}

}  // namespace

// Returns the launch's hipError_t (0 = success); refuses nothing: the caller passes a shape bf_dedisperse accepted.
extern "C" int bf_dedisperse_naive(const float* ring, const int32_t* lags, float* out, int K, int M, int D, int N, int R,
                                   int head, float scale, void* stream) {
  const long long total = static_cast<long long>(M) * D * N;
  hipLaunchKernelGGL(dedisperse_naive_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), ring, lags, out, K, M, D, N, R, head,
                     static_cast<double>(scale));
  return static_cast<int>(hipGetLastError());
}
