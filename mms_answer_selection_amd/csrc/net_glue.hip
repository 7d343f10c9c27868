// csrc/net_glue.hip -- the kernels that run around the layer kernels on every Net iteration: the dot product behind a
// loss top, Split's backward sum, and the empty launch that measures the launch floor.
#include "mms_internal.h"

namespace mms {
// measurement aid (include/mms.h: mms_null_launch)
__global__ __launch_bounds__(512) void null_kernel(int) {}

// x . y with the result left on the device (fixed-shape tree: deterministic); what Layer::Forward needs for a
// loss top in GPU mode (include/caffe/layer.hpp:469-481 calls caffe_gpu_dot there)
template <typename T>
__global__ __launch_bounds__(256) void dot_kernel(int n, const T* __restrict__ x, const T* __restrict__ y,
                                                  T* __restrict__ out) {
  __shared__ T red[256];
  T s = 0;
  for (int i = threadIdx.x; i < n; i += 256) s += x[i] * y[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
}
struct SplitPtrs { const float* p[8]; };
// out = ((carry? out : p0) + p1) + ... in index order
__global__ __launch_bounds__(256) void split_sum_kernel(int n, int k, SplitPtrs s, int carry, float* __restrict__ out) {
  const int stride = gridDim.x * 256;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float v = carry ? out[i] : s.p[0][i];
    for (int j = carry ? 0 : 1; j < k; ++j) v = v + s.p[j][i];
    out[i] = v;
  }
}

int null_launch(int workgroups, hipStream_t s) {
  hipLaunchKernelGGL(null_kernel, dim3(workgroups), dim3(512), 0, s, workgroups);
  return launch_status();
}
template <class T>
int dot(int n, const T* x, const T* y, T* out, hipStream_t s) {
  hipLaunchKernelGGL(dot_kernel<T>, dim3(1), dim3(256), 0, s, n, x, y, out);
  return launch_status();
}
template int dot<float>(int, const float*, const float*, float*, hipStream_t);
template int dot<double>(int, const double*, const double*, double*, hipStream_t);
// bottom_diff = the sum of ntop >= 1 top diffs of count > 0 elements, in index order (Split's backward)
int split_sum(int count, int ntop, const float* const* top_diffs, float* bottom_diff, hipStream_t s) {
  const unsigned grid = (unsigned)((count + 255) / 256 < 2048 ? (count + 255) / 256 : 2048);
  for (int first = 0; first < ntop; first += 8) {
    SplitPtrs sp{};
    const int k = ntop - first < 8 ? ntop - first : 8;
    for (int j = 0; j < k; ++j) sp.p[j] = top_diffs[first + j];
    hipLaunchKernelGGL(split_sum_kernel, dim3(grid), dim3(256), 0, s, count, k, sp, first > 0 ? 1 : 0, bottom_diff);
  }
  return launch_status();
}
}  // namespace mms
