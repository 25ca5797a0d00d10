// RMSNorm forward/backward for gfx950.
//
// Replaces the reference's per-layer HF eager RMSNorm (run inside
// tensorlink/ml/worker.py:330-335 via transformers modules) with a fused,
// bf16x8-vectorized single-pass kernel. The fused-residual variant folds the
// residual add of the decoder block into the same HBM round trip — on
// MI355X the residual stream is the memory-bound hot path (~8 TB/s HBM).
//
// Layout: x [N, H] bf16 row-major, weight [H] bf16. H % 8 == 0 required
// (all zoo models satisfy this; wrapper enforces).

#include "common.hpp"

namespace {

constexpr int BLOCK = 256;
constexpr int NW = BLOCK / WAVE_SIZE;

// Forward: one block per row, ITERS*BLOCK*8 >= H.
// RES: 0 = plain norm of x.
//      1 = fused residual add ("mode A"): f = x + residual in fp32,
//          r_out = bf16(f), the norm uses the UNROUNDED f.
//      2 = add, then plain norm ("mode B"): r_out = bf16(x + residual), the
//          norm uses the ROUNDED r_out — what a separate bf16 add kernel
//          followed by the RES=0 norm computes.
//      3 = mode B's add alone: writes r_out, no norm.
// PART: x is the fp32 split-K partial tensor [n_split, rows, H] of the GEMM
// family (split_stride = rows*H) instead of bf16 [rows, H]; the element is
// bf16(sum_s partial[s]) summed from 0 in s order — the value the GEMM's
// own reduce kernel writes.
template <int ITERS, int RES, int PART>
__global__ __launch_bounds__(BLOCK) void rmsnorm_fwd_kernel(
    const void* __restrict__ x_, const bf16* __restrict__ residual,
    const bf16* __restrict__ w, bf16* __restrict__ y, bf16* __restrict__ r_out,
    float* __restrict__ rstd_out, int H, float eps, int n_split,
    int64_t split_stride) {
  __shared__ float lds[NW];
  const int64_t row = blockIdx.x;
  const bf16* xrow = PART ? nullptr : (const bf16*)x_ + row * H;
  const float* prow = PART ? (const float*)x_ + row * H : nullptr;
  const bf16* rrow = RES ? residual + row * H : nullptr;

  // partials: sum every group this thread owns up front (idle lanes of a
  // ragged last iteration re-read column 0 and drop the result)
  constexpr int CH = ITERS <= 2 ? 8 : ITERS <= 4 ? 4 : 2;
  float psum[PART ? ITERS : 1][8];
  if constexpr (PART) {
    const float* pp[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int base = (it * BLOCK + threadIdx.x) * 8;
      pp[it] = prow + (base < H ? base : 0);
    }
    sum_partials8<ITERS, CH>(pp, split_stride, n_split, psum);
  }

  float vals[ITERS][8];
  float sumsq = 0.f;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int base = (it * BLOCK + threadIdx.x) * 8;
    if (base < H) {
      bf16x8 vx;
      if constexpr (PART) {
#pragma unroll
        for (int j = 0; j < 8; ++j) vx.v[j] = f2bf(psum[it][j]);
      } else {
        vx = *reinterpret_cast<const bf16x8*>(xrow + base);
      }
      if (RES) {
        bf16x8 vr = *reinterpret_cast<const bf16x8*>(rrow + base);
        bf16x8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = bf2f(vx.v[j]) + bf2f(vr.v[j]);
          out.v[j] = f2bf(f);
          if (RES >= 2) f = bf2f(out.v[j]);
          vals[it][j] = f;
          sumsq += f * f;
        }
        *reinterpret_cast<bf16x8*>(r_out + row * H + base) = out;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = bf2f(vx.v[j]);
          vals[it][j] = f;
          sumsq += f * f;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) vals[it][j] = 0.f;
    }
  }
  if (RES == 3) return;

  const float total = block_reduce_sum<NW>(sumsq, lds);
  const float rstd = rsqrtf(total / H + eps);
  if (threadIdx.x == 0 && rstd_out != nullptr) rstd_out[row] = rstd;

#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int base = (it * BLOCK + threadIdx.x) * 8;
    if (base < H) {
      bf16x8 vw = *reinterpret_cast<const bf16x8*>(w + base);
      bf16x8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        out.v[j] = f2bf(vals[it][j] * rstd * bf2f(vw.v[j]));
      *reinterpret_cast<bf16x8*>(y + row * H + base) = out;
    }
  }
}

// Backward: dx = (g - xhat * mean(g * xhat)) * rstd  where g = dy * w,
// xhat = x * rstd. Each block strides over rows, accumulating a private
// dw partial slab; a second kernel folds the slabs.
template <int ITERS>
__global__ __launch_bounds__(BLOCK) void rmsnorm_bwd_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ x,
    const bf16* __restrict__ w, const float* __restrict__ rstd,
    bf16* __restrict__ dx, float* __restrict__ dw_partial, int64_t N, int H) {
  __shared__ float lds[NW];
  float dw_acc[ITERS][8];
#pragma unroll
  for (int it = 0; it < ITERS; ++it)
#pragma unroll
    for (int j = 0; j < 8; ++j) dw_acc[it][j] = 0.f;

  for (int64_t row = blockIdx.x; row < N; row += gridDim.x) {
    const float rs = rstd[row];
    float xh[ITERS][8], g[ITERS][8];
    float dot = 0.f;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int base = (it * BLOCK + threadIdx.x) * 8;
      if (base < H) {
        bf16x8 vx = *reinterpret_cast<const bf16x8*>(x + row * H + base);
        bf16x8 vdy = *reinterpret_cast<const bf16x8*>(dy + row * H + base);
        bf16x8 vw = *reinterpret_cast<const bf16x8*>(w + base);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xhat = bf2f(vx.v[j]) * rs;
          float gv = bf2f(vdy.v[j]) * bf2f(vw.v[j]);
          xh[it][j] = xhat;
          g[it][j] = gv;
          dot += gv * xhat;
          dw_acc[it][j] += bf2f(vdy.v[j]) * xhat;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) { xh[it][j] = 0.f; g[it][j] = 0.f; }
      }
    }
    const float mean_dot = block_reduce_sum<NW>(dot, lds) / H;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int base = (it * BLOCK + threadIdx.x) * 8;
      if (base < H) {
        bf16x8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          out.v[j] = f2bf((g[it][j] - xh[it][j] * mean_dot) * rs);
        *reinterpret_cast<bf16x8*>(dx + row * H + base) = out;
      }
    }
    __syncthreads();  // lds reuse across row iterations
  }

  // dump private dw partials: slab layout [gridDim.x, H]
  float* slab = dw_partial + (int64_t)blockIdx.x * H;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int base = (it * BLOCK + threadIdx.x) * 8;
    if (base < H) {
#pragma unroll
      for (int j = 0; j < 8; ++j) slab[base + j] = dw_acc[it][j];
    }
  }
}

__global__ void reduce_partials_kernel(const float* __restrict__ partials,
                                       bf16* __restrict__ out, int P,
                                       int64_t H) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H) return;
  float acc = 0.f;
  for (int p = 0; p < P; ++p) acc += partials[(int64_t)p * H + i];
  out[i] = f2bf(acc);
}

template <int RES, int PART>
void launch_fwd(const void* x, const bf16* res, const bf16* w, bf16* y,
                bf16* r_out, float* rstd, int64_t N, int H, float eps,
                int n_split, hipStream_t s) {
  dim3 grid((uint32_t)N), block(BLOCK);
  const int iters = cdiv(H, BLOCK * 8);
  const int64_t split_stride = N * H;
#define CASE(I)                                                              \
  case I:                                                                    \
    hipLaunchKernelGGL((rmsnorm_fwd_kernel<I, RES, PART>), grid, block, 0,   \
                       s, x, res, w, y, r_out, rstd, H, eps, n_split,        \
                       split_stride);                                        \
    break;
  switch (iters) {
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
    default: break;
  }
#undef CASE
}

}  // namespace

extern "C" {

void tl_rmsnorm_fwd(const void* x, const void* residual, const void* w,
                    void* y, void* r_out, void* rstd, int64_t N, int H,
                    float eps, hipStream_t stream) {
  if (residual)
    launch_fwd<1, 0>(x, (const bf16*)residual, (const bf16*)w, (bf16*)y,
                     (bf16*)r_out, (float*)rstd, N, H, eps, 1, stream);
  else
    launch_fwd<0, 0>(x, nullptr, (const bf16*)w, (bf16*)y, nullptr,
                     (float*)rstd, N, H, eps, 1, stream);
}

// Residual add + norm with x as bf16 [N, H] (n_split == 0) or as the GEMM
// family's fp32 partials [n_split, N, H]. mode 1/2/3 = the kernel's RES
// (A: norm of the unrounded sum; B: norm of the rounded sum; 3: sum only,
// y and w unused).
void tl_rmsnorm_add_fwd(const void* x, const void* residual, const void* w,
                        void* y, void* r_out, int64_t N, int H, float eps,
                        int n_split, int mode, hipStream_t stream) {
#define GO(R, P)                                                          \
  launch_fwd<R, P>(x, (const bf16*)residual, (const bf16*)w, (bf16*)y,    \
                   (bf16*)r_out, nullptr, N, H, eps, n_split, stream)
  if (n_split > 0) {
    if (mode == 1) GO(1, 1);
    else if (mode == 2) GO(2, 1);
    else GO(3, 1);
  } else {
    if (mode == 1) GO(1, 0);
    else if (mode == 2) GO(2, 0);
    else GO(3, 0);
  }
#undef GO
}

// dw_partial must hold [n_blocks, H] floats; returns via dx, dw.
void tl_rmsnorm_bwd(const void* dy, const void* x, const void* w,
                    const void* rstd, void* dx, void* dw, void* dw_partial,
                    int n_blocks, int64_t N, int H, hipStream_t stream) {
  const int iters = cdiv(H, BLOCK * 8);
  dim3 grid(n_blocks), block(BLOCK);
#define CASE(I)                                                               \
  case I:                                                                     \
    hipLaunchKernelGGL((rmsnorm_bwd_kernel<I>), grid, block, 0, stream,       \
                       (const bf16*)dy, (const bf16*)x, (const bf16*)w,       \
                       (const float*)rstd, (bf16*)dx, (float*)dw_partial, N,  \
                       H);                                                    \
    break;
  switch (iters) {
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
    default: break;
  }
#undef CASE
  dim3 rgrid(cdiv(H, 256)), rblock(256);
  hipLaunchKernelGGL(reduce_partials_kernel, rgrid, rblock, 0, stream,
                     (const float*)dw_partial, (bf16*)dw, n_blocks, H);
}

}  // extern "C"
