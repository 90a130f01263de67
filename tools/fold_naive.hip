// The naive fold the product kernel of csrc/bf_fold.hip is measured against (tools/bench_ops.py --fold): one thread per
// (f, s, k), k fastest, walking the N samples in order and updating memory directly; the thread of plane 0 also counts
// the hits.  Same contract as bf_fold (a thread owns its accumulator rows, so there are no collisions to resolve).  A
// measurement library of its own (build/libbf_fold_naive.so, `make fold-naive`), never linked into the product.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

struct NaiveTables {
  int beam[64];
  unsigned long long phase0[64], dphase[64];
};

__global__ __launch_bounds__(256) void fold_naive_kernel(const float* power, const unsigned long long* chan,
                                                         double* profile, uint32_t* hits, int B, int S, int K, int J,
                                                         int M, int F, int nbin, NaiveTables T) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<long long>(F) * S * K) return;
  const int k = static_cast<int>(i % K), s = static_cast<int>(i / K % S), f = static_cast<int>(i / K / S);
  int beam = 0;
  unsigned long long phi = 0, step = 0;
  for (int q = 0; q < F; ++q) {  // a uniform index: the tables stay in the kernel arguments
    if (q == f) {
      beam = T.beam[q];
      phi = T.phase0[q];
      step = T.dphase[q];
    }
  }
  phi -= chan[static_cast<long long>(f) * K + k];
  double* prof = profile + i * nbin;
  uint32_t* hit = hits + (static_cast<long long>(f) * K + k) * nbin;
  for (int b = 0; b < B; ++b) {
    const float* src = power + ((static_cast<long long>(b) * S + s) * K + k) * J * M + beam;
    for (int j = 0; j < J; ++j, phi += step) {
      const int bin = static_cast<int>(((phi >> 32) * static_cast<unsigned long long>(nbin)) >> 32);
      prof[bin] += static_cast<double>(src[static_cast<long long>(j) * M]);
      if (s == 0) hit[bin] += 1;
    }
  }
}

}  // namespace

// Returns the launch's hipError_t (0 = success); refuses nothing: the caller passes arguments bf_fold accepted.
extern "C" int bf_fold_naive(const float* power, const int32_t* beam, const uint64_t* phase0, const uint64_t* dphase,
                             const uint64_t* chan, double* profile, uint32_t* hits, int B, int S, int K, int J, int M,
                             int F, int nbin, void* stream) {
  NaiveTables T = {};
  for (int f = 0; f < F; ++f) {
    T.beam[f] = beam[f];
    T.phase0[f] = phase0[f];
    T.dphase[f] = dphase[f];
  }
  const long long total = static_cast<long long>(F) * S * K;
  hipLaunchKernelGGL(fold_naive_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), power, reinterpret_cast<const unsigned long long*>(chan),
                     profile, hits, B, S, K, J, M, F, nbin, T);
  return static_cast<int>(hipGetLastError());
}
