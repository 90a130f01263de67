// Timing probe (not product): read-path variants of the incoherent beam's antenna walk (csrc/bf_incoherent.hip) next
// to a plain read stream over the same bytes, at config 2/3's cube (8 x 64 antennas x 4 MiB) and config 4's (256 x
// 4 MiB).  Varies the workgroup size TH, the 16-byte loads per lane and antenna L (contiguous run per workgroup and
// antenna = L * TH * 16 bytes), the antennas per unrolled batch U, non-temporal loads and an XCD-range piece order.
// Result (profiles/incoherent_read_path_probe.txt): the contiguous run sets the rate; TH = 512, L = 2, U = 4 is the
// product's choice.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probes/incoherent_read_path.hip -o build/incoherent_read_path
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define CK(x)                                                                    \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) {                                                      \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(2);                                                                   \
    }                                                                            \
  } while (0)

// plain read stream: grid-stride, 16 B per lane
template <bool Nt>
__global__ __launch_bounds__(256) void read_stream(const u32x4* in, uint32_t* out, size_t n16) {
  uint32_t s = 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * 256;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n16; i += stride) {
    const u32x4 v = Nt ? __builtin_nontemporal_load(in + i) : in[i];
    s += v[0] ^ v[1] ^ v[2] ^ v[3];
  }
  if (s == 0x12345678u) out[0] = s;
}

// Threads per block TH, L consecutive step-loads per lane per antenna (span = L * TH * 16 bytes per antenna per
// workgroup), U antennas per unrolled batch, Nt loads, Xcd: XCD-range piece order.
template <int TH, int L, int U, bool Nt, bool Xcd>
__global__ __launch_bounds__(TH) void walk(const uint8_t* raw, uint32_t* out, size_t N, unsigned pieces, int A) {
  const int tid = threadIdx.x;
  const unsigned b = blockIdx.x / pieces;
  unsigned piece = blockIdx.x % pieces;
  if (Xcd && pieces % 8 == 0) piece = (piece & 7) * (pieces >> 3) + (piece >> 3);
  const size_t stride = N * 4;
  const uint8_t* src = raw + static_cast<size_t>(b) * A * stride + (static_cast<size_t>(piece) * L * TH + tid) * 16;
  uint32_t acc[L][4][2] = {};
  for (int a = 0; a + U <= A; a += U) {
    u32x4 v[U][L];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int l = 0; l < L; ++l) {
        const u32x4* p = reinterpret_cast<const u32x4*>(src + static_cast<size_t>(a + u) * stride + l * TH * 16);
        v[u][l] = Nt ? __builtin_nontemporal_load(p) : *p;
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[l][j][0] = __builtin_amdgcn_udot4(v[u][l][j], v[u][l][j] & 0xffffu, acc[l][j][0], false);
          acc[l][j][1] = __builtin_amdgcn_udot4(v[u][l][j], v[u][l][j] & 0xffff0000u, acc[l][j][1], false);
        }
  }
  uint32_t s = 0;
#pragma unroll
  for (int l = 0; l < L; ++l)
#pragma unroll
    for (int j = 0; j < 4; ++j) s += acc[l][j][0] + 3 * acc[l][j][1];
  out[(static_cast<size_t>(blockIdx.x) * TH + tid)] = s;
}

static float time_it(void (*fn)(void*), void* ctx, int reps) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int i = 0; i < 30; ++i) fn(ctx);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0, 0));
  for (int i = 0; i < reps; ++i) fn(ctx);
  CK(hipEventRecord(e1, 0));
  CK(hipEventSynchronize(e1));
  CK(hipGetLastError());
  float ms;
  CK(hipEventElapsedTime(&ms, e0, e1));
  return ms * 1000.f / reps;
}

struct Ctx {
  const uint8_t* raw;
  uint32_t* out;
  size_t N;
  int A, B;
  int grid;
};

template <int TH, int L, int U, bool Nt, bool Xcd>
static void run_walk(void* c) {
  Ctx* x = static_cast<Ctx*>(c);
  const unsigned pieces = static_cast<unsigned>(x->N / (static_cast<size_t>(L) * TH * 4));
  hipLaunchKernelGGL((walk<TH, L, U, Nt, Xcd>), dim3(pieces * x->B), dim3(TH), 0, 0, x->raw, x->out, x->N, pieces, x->A);
}
template <bool Nt>
static void run_stream(void* c) {
  Ctx* x = static_cast<Ctx*>(c);
  hipLaunchKernelGGL((read_stream<Nt>), dim3(x->grid), dim3(256), 0, 0, reinterpret_cast<const u32x4*>(x->raw), x->out,
                     x->N * 4 * x->A * x->B / 16);
}

#define WALK(TH, L, U, NT, XCD)                                                                      \
  do {                                                                                               \
    const float us = time_it(run_walk<TH, L, U, NT, XCD>, &c, 20);                                   \
    printf("%s walk TH=%d L=%d U=%d nt=%d xcd=%d : %.1f us  %.0f GB/s\n", name, TH, L, U, NT, XCD, us, \
           bytes / us * 1e-3);                                                                       \
    fflush(stdout);                                                                                  \
  } while (0)

int main() {
  const size_t total = 2ull << 30;
  uint8_t* raw;
  uint32_t* out;
  CK(hipMalloc(&raw, total));
  CK(hipMalloc(&out, 64ull << 20));
  CK(hipMemset(raw, 0x5a, total));
  struct {
    const char* name;
    int B, A;
    size_t N;
  } shapes[] = {{"cfg2", 8, 64, 4096ull * 256}, {"cfg4", 1, 256, 4096ull * 256}};
  for (auto& s : shapes) {
    Ctx c{raw, out, s.N, s.A, s.B, 2048};
    const char* name = s.name;
    const double bytes = 4.0 * s.N * s.A * s.B;
    for (int grid : {1024, 2048, 4096}) {
      c.grid = grid;
      printf("%s stream grid %d plain %.1f us, nt %.1f us\n", name, grid, time_it(run_stream<false>, &c, 20),
             time_it(run_stream<true>, &c, 20));
    }
    WALK(256, 1, 8, true, false);
    WALK(256, 1, 8, false, false);
    WALK(256, 1, 8, true, true);
    WALK(256, 1, 4, true, false);
    WALK(256, 1, 16, true, false);
    WALK(256, 2, 4, true, false);
    WALK(256, 2, 4, true, true);
    WALK(256, 2, 8, true, false);
    WALK(256, 4, 2, true, false);
    WALK(256, 4, 2, true, true);
    WALK(256, 4, 4, true, false);
    WALK(256, 4, 4, true, true);
    WALK(512, 1, 8, true, false);
    WALK(512, 2, 4, true, false);
    WALK(1024, 1, 8, true, false);
    WALK(1024, 1, 8, true, true);
    WALK(1024, 2, 4, true, true);
    WALK(64, 1, 8, true, false);
    WALK(64, 4, 2, true, false);
    WALK(64, 4, 4, true, true);
  }
  CK(hipDeviceSynchronize());
  printf("done\n");
  return 0;
}
