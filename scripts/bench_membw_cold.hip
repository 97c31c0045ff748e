// Cold-cache read floor for the skinny GEMM's W access pattern and grid:
// rotating buffers, > 256 MB in total, so the last-level cache never holds W.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

typedef __attribute__((ext_vector_type(4))) unsigned int uint4v;

// 16 rows per wave, 64 B per row per load; UN loads (UN*32 k) in flight.
template <int UN>
__global__ __launch_bounds__(256) void read_rows(
    const unsigned short* __restrict__ src, int k_total, int k_per_split,
    uint4v* __restrict__ sink) {
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int lq = lane % 16, la = lane / 16;
  const int row = blockIdx.x * 64 + wave * 16 + lq;
  const int kb = blockIdx.y * k_per_split;
  const int ke = min(k_total, kb + k_per_split);
  const unsigned short* p = src + (size_t)row * k_total + 8 * la;
  uint4v acc = {0, 0, 0, 0};
  int k = kb;
  for (; k + UN * 32 <= ke; k += UN * 32) {
    uint4v v[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u)
      v[u] = *reinterpret_cast<const uint4v*>(p + k + u * 32);
#pragma unroll
    for (int u = 0; u < UN; ++u) acc ^= v[u];
  }
  for (; k < ke; k += 32) acc ^= *reinterpret_cast<const uint4v*>(p + k);
  if (acc.x == 0xdeadbeef) sink[threadIdx.x] = acc;
}

int main() {
  struct Shape { int n, k, ns, kps; const char* label; };
  std::vector<Shape> shapes = {{3584, 18944, 8, 2368, "down ns8"},
                               {3584, 18944, 16, 1184, "down ns16"},
                               {3584, 18944, 9, 2112, "down ns9"},
                               {4608, 3584, 8, 448, "qkv ns8"},
                               {3584, 3584, 10, 384, "o ns10"}};
  uint4v* sink;
  if (hipMalloc(&sink, 4096) != hipSuccess) return 1;
  for (auto& s : shapes) {
    size_t bytes = (size_t)s.n * s.k * 2;
    int nbuf = (int)((640ull << 20) / bytes) + 1;
    if (nbuf < 2) nbuf = 2;
    std::vector<unsigned short*> bufs(nbuf);
    for (auto& b : bufs) {
      if (hipMalloc(&b, bytes) != hipSuccess) return 1;
      (void)hipMemset(b, 1, bytes);
    }
    dim3 grid(s.n / 64, s.ns);
    for (int un : {4, 16}) {
      auto rot = [&](int n) {
        for (int r = 0; r < n; ++r)
          for (auto b : bufs) {
            if (un == 4)
              hipLaunchKernelGGL(read_rows<4>, grid, dim3(256), 0, 0, b, s.k, s.kps, sink);
            else
              hipLaunchKernelGGL(read_rows<16>, grid, dim3(256), 0, 0, b, s.k, s.kps, sink);
          }
      };
      rot(2);
      if (hipDeviceSynchronize() != hipSuccess) return 2;
      hipEvent_t t0, t1;
      (void)hipEventCreate(&t0); (void)hipEventCreate(&t1);
      (void)hipEventRecord(t0, 0);
      rot(3);
      (void)hipEventRecord(t1, 0);
      if (hipEventSynchronize(t1) != hipSuccess) return 2;
      float ms = 0; (void)hipEventElapsedTime(&ms, t0, t1);
      double us = ms * 1000.0 / (3 * nbuf);
      printf("%-10s unroll=%2d nbuf=%2d  %7.2f us  %5.2f TB/s\n", s.label, un, nbuf, us, bytes / us / 1e6);
      fflush(stdout);
      (void)hipEventDestroy(t0); (void)hipEventDestroy(t1);
    }
    for (auto b : bufs) (void)hipFree(b);
  }
  return 0;
}
