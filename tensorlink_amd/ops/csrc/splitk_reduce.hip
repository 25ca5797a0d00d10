// The GEMM family's one split-K reduce (declared in gemm_family.hpp):
// out[i] = bf16(sum_s partial[s][i] (+ bias)), s ascending from 0.f — no
// atomics, so the sum order is fixed. The partials consumers in
// rmsnorm.hip / rope_append.hip (sum_partials8, common.hpp) reproduce
// exactly this sum.

#include "gemm_family.hpp"

namespace {

template <int HAS_BIAS>
__global__ void splitk_reduce_kernel(const float* __restrict__ partial,
                                     const bf16* __restrict__ bias,
                                     bf16* __restrict__ out, int64_t MN,
                                     int N, int n_split) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= MN) return;
  float acc = 0.f;
  for (int s = 0; s < n_split; ++s) acc += partial[s * MN + i];
  if (HAS_BIAS) acc += bf2f(bias[i % N]);
  out[i] = f2bf(acc);
}

}  // namespace

void launch_splitk_reduce(const void* partial, const void* bias, void* out,
                          int64_t M, int N, int n_split,
                          hipStream_t stream) {
  const int64_t MN = M * N;
  dim3 grid((uint32_t)((MN + 255) / 256)), block(256);
  auto kernel = bias ? splitk_reduce_kernel<1> : splitk_reduce_kernel<0>;
  hipLaunchKernelGGL(kernel, grid, block, 0, stream, (const float*)partial,
                     (const bf16*)bias, (bf16*)out, MN, N, n_split);
}
