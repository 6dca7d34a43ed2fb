// stream_sum.hip -- the yardstick of tools/bench_taxon_counts.py: a plain coalesced read-and-sum of a buffer as large as the table
// (libslk_stream_sum.so), 16 B per lane with four loads in flight, as slk_index_taxon_counts reads the cells -- what the same pass
// costs without the count.  Measurement infrastructure, not product: nothing in slacken_amd/ links or loads it.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int BLOCK = 512, UNROLL = 4;

__global__ void __launch_bounds__(BLOCK) stream_sum(const ulonglong2 *__restrict__ src, uint64_t n, unsigned long long *out) {
  unsigned long long acc = 0;
  const uint64_t tile = (uint64_t)BLOCK * UNROLL, stride = (uint64_t)gridDim.x * tile;
  for (uint64_t base = (uint64_t)blockIdx.x * tile; base < n; base += stride) {
    ulonglong2 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      const uint64_t i = base + (uint64_t)u * BLOCK + threadIdx.x;
      v[u] = i < n ? src[i] : make_ulonglong2(0, 0);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; u++) acc += v[u].x + v[u].y;
  }
  for (int d = 32; d > 0; d >>= 1) acc += ((unsigned long long)(uint32_t)__shfl_down((int)(acc >> 32), d) << 32) + (uint32_t)__shfl_down((int)acc, d);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}

}  // namespace

// d_buf: `bytes` of device memory on the current device; one warm-up launch, then the best of `reps` timed ones.  0 = ok.
extern "C" int slk_stream_sum(const void *d_buf, uint64_t bytes, int blocks, int reps, float *out_best_ms, unsigned long long *out_sum) {
  if (!d_buf || !out_best_ms || blocks < 1 || reps < 1) return -1;
  const uint64_t n = bytes / 16;
  unsigned long long *d_out = nullptr;
  hipEvent_t a = nullptr, b = nullptr;
  if (hipMalloc((void **)&d_out, 8) != hipSuccess) return -2;
  int rc = 0;
  float best = 0;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) rc = -2;
  for (int r = 0; !rc && r <= reps; r++) {   // r == 0: warm-up
    float ms = 0;
    if (hipMemsetAsync(d_out, 0, 8, 0) != hipSuccess || hipEventRecord(a, 0) != hipSuccess) { rc = -3; break; }
    hipLaunchKernelGGL(stream_sum, dim3(blocks), dim3(BLOCK), 0, 0, (const ulonglong2 *)d_buf, n, d_out);
    if (hipEventRecord(b, 0) != hipSuccess || hipEventSynchronize(b) != hipSuccess || hipGetLastError() != hipSuccess) { rc = -3; break; }
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { rc = -3; break; }
    if (r >= 1 && (r == 1 || ms < best)) best = ms;
  }
  if (!rc && out_sum && hipMemcpy(out_sum, d_out, 8, hipMemcpyDeviceToHost) != hipSuccess) rc = -3;
  if (a) (void)hipEventDestroy(a);
  if (b) (void)hipEventDestroy(b);
  (void)hipFree(d_out);
  if (rc) return rc;
  *out_best_ms = best;
  return 0;
}
