// Microbenchmark: the copy ceiling the IDA up-step (convt.hip) is held against. A plain 16-byte-per-
// lane copy of the 120x160 up-step's skip tensor at 32 frames (157 MB in, 157 MB out), 20 launches
// per grid size timed one by one with HIP events: median and minimum per launch, bytes / time.
// Build: hipcc -O3 --offload-arch=gfx950 copy_ceiling.hip -o copy_ceiling
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

__global__ __launch_bounds__(256) void copy16(const uint4* __restrict__ in, uint4* __restrict__ out, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = in[i];
}

// 4 independent 16-byte loads in flight per lane before the first store
__global__ __launch_bounds__(256) void copy16x4(const uint4* __restrict__ in, uint4* __restrict__ out, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = in[i + k * stride];
#pragma unroll
    for (int k = 0; k < 4; ++k) out[i + k * stride] = v[k];
  }
  for (; i < n; i += stride) out[i] = in[i];
}

int main() {
  const long bytes = 32L * 120 * 160 * 256;  // one 32-frame 120x160 level of 128 fp16 channels
  const long n = bytes / 16;
  uint4 *in, *out;
  if (hipMalloc(&in, bytes) != hipSuccess || hipMalloc(&out, bytes) != hipSuccess) return 1;
  if (hipMemset(in, 1, bytes) != hipSuccess || hipMemset(out, 0, bytes) != hipSuccess) return 1;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  double best = 0;
  for (int variant = 0; variant < 2; ++variant) {
    for (int grid : {1024, 2048, 4096, 8192}) {
      std::vector<float> ms(20);
      for (int r = -2; r < 20; ++r) {  // two unrecorded warm-ups
        (void)hipEventRecord(e0);
        if (variant == 0) hipLaunchKernelGGL(copy16, dim3(grid), dim3(256), 0, 0, in, out, n);
        else hipLaunchKernelGGL(copy16x4, dim3(grid), dim3(256), 0, 0, in, out, n);
        (void)hipEventRecord(e1);
        if (hipEventSynchronize(e1) != hipSuccess) return 2;
        float t;
        (void)hipEventElapsedTime(&t, e0, e1);
        if (r >= 0) ms[r] = t;
      }
      std::sort(ms.begin(), ms.end());
      const double med = 0.5 * (ms[9] + ms[10]);
      printf("{\"kernel\": \"%s\", \"grid\": %d, \"bytes_in\": %ld, \"bytes_out\": %ld, \"median_ms\": %.4f, \"min_ms\": %.4f, "
             "\"median_TBps\": %.3f, \"min_TBps\": %.3f}\n",
             variant ? "copy16x4" : "copy16", grid, bytes, bytes, med, ms[0], 2.0 * bytes / med / 1e9, 2.0 * bytes / ms[0] / 1e9);
      best = std::max(best, 2.0 * bytes / med / 1e9);
    }
  }
  printf("{\"copy_ceiling_median_TBps\": %.3f}\n", best);
  return 0;
}
