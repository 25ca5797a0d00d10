// Fused linear cross-entropy: the training loss head without the logits.
// With logit[m, n] = sum_k x[m,k] * W[n,k] kept UNROUNDED in the f32
// accumulators,
//   MODE 0 (stats)    per 256-column panel and row: m = max logit and
//                     s = sum exp(logit - m) over the panel's real columns,
//                     plus tgt[row] = logit[row, label[row]];
//                     head_ce_combine_kernel merges the panels into
//                     lse[row] and loss_row[row] = lse - tgt;
//   MODE 1 (gradient) g[row, n] = bf16((exp(logit - lse[row])
//                     - (n == label[row])) * scale[row]).
// No [M, V] f32 tensor exists anywhere; the only scratch is one (m, s) pair
// per (panel, row) and one float per row, fully written before it is read
// (no atomics, no pre-zeroing, no host sync).
//
// The accumulators come from sq256_k_loop (gemm_family.hpp), the 256x256
// loop gemm_tiled_sq_kernel writes out and head_argmax_kernel calls, in
// both modes: a logit here has the bits the family's GEMM would round.
// MODE 0's two row passes (max, then sum of exp) are sq256_row_reduce, which fixes the order
// of the float sum.
//
// Ghosts: the clamped loads duplicate W row V - 1 into columns >= V of the
// last panel and x row M - 1 into rows >= M of the last row block. Ghost
// columns take no part in max, sum, label match or store; ghost rows are
// computed and never written. A row's bits depend on nothing but that row
// of x, W and its label: not on M, the row block, or the launch it is in.
//
// Grid: one dimension, cdiv(rows, 256) row blocks x cdiv(V, 256) panels.
// rows_fast != 0 lets the row block run fastest, so consecutive workgroups
// share a W panel; 0 lets the panel run fastest, so they share an x block
// (profiles/fused_ce.md has both timings).

#include "gemm_family.hpp"

#include <cmath>

namespace {

template <int MODE>
__global__ __launch_bounds__(512, 1) void head_ce_kernel(
    const bf16* __restrict__ x,          // [M, K]
    const bf16* __restrict__ w,          // [V, K]
    const int64_t* __restrict__ labels,  // [M]
    float2* __restrict__ ms_out,         // MODE 0: [cdiv(V, 256), M] (m, s)
    float* __restrict__ tgt,             // MODE 0: [M] label logit
    const float* __restrict__ lse,       // MODE 1: [M]
    const float* __restrict__ scale,     // MODE 1: [M]
    bf16* __restrict__ g,                // MODE 1: [M, V]
    int M, int V, int K, int rows_fast) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;          // 0..7
  const int col = lane & 15;
  const int quad = lane >> 4;
  const int wm = wave >> 2;                   // 0..1: 128-row band
  const int wn = wave & 3;                    // 0..3: 64-col band
  const int n_rb = cdiv(M, 256);
  const int n_panel = cdiv(V, 256);
  const int panel = rows_fast ? (int)blockIdx.x / n_rb
                              : (int)blockIdx.x % n_panel;
  const int rb = rows_fast ? (int)blockIdx.x % n_rb
                           : (int)blockIdx.x / n_panel;
  const int m_base = rb * 256;

  __shared__ bf16 lds[2][256 + 256][64];
  f32x4 acc[32];
  sq256_k_loop(x, w, m_base, panel * 256, M, V, K,
               family_k_slice<0>(K, 1, 0), lds, acc, lane, wave);

  // Epilogue. Lane (col, quad) holds C[mt*16 + quad*4 + r][nt*16 + col] of
  // its wave's 128 x 64 quadrant. gc0 is the global column of nt = 0; a
  // column takes part only if it is < V.
  const int gc0 = panel * 256 + wn * 64 + col;
  const int lrow0 = wm * 128 + quad * 4;      // + mt * 16 + r: row in tile

  if constexpr (MODE == 0) {
    // The freed LDS ring: red is sq256_row_reduce's [4 wn][256 rows]
    // meeting place, pmax [256] the panel's row maxima.
    float* red = reinterpret_cast<float*>(&lds[0][0][0]);
    float* pmax = red + 4 * 256;

    // 1) row max. Every panel has a real column, so it is finite for
    // finite data.
    const float pm = sq256_row_reduce(
        red, -INFINITY,
        [&](int mt, int r, int nt) {
          return gc0 + nt * 16 < V ? acc[mt * 4 + nt][r] : -INFINITY;
        },
        [](float a, float b) { return fmaxf(a, b); });
    if (threadIdx.x < 256) pmax[threadIdx.x] = pm;
    __syncthreads();

    // 2) s = sum exp(logit - panel max), in the helper's fixed order.
    const float s = sq256_row_reduce(
        red, 0.f,
        [&](int mt, int r, int nt) {
          const float e = expf(acc[mt * 4 + nt][r] - pmax[lrow0 + mt * 16 + r]);
          return gc0 + nt * 16 < V ? e : 0.f;
        },
        [](float a, float b) { return a + b; });
    if (threadIdx.x < 256 && m_base + threadIdx.x < M)
      ms_out[(int64_t)panel * M + m_base + threadIdx.x] = make_float2(pm, s);

    // The label logit, from the one lane whose column is the label.
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m_base + lrow0 + mt * 16 + r;
        const int64_t lab = labels[min(row, M - 1)];
        const int64_t d = lab - gc0;          // 0, 16, 32, 48: nt * 16
        if (row < M && d >= 0 && d < 64 && (d & 15) == 0 && lab < V) {
          const int nt = (int)d >> 4;
          const float a01 = nt == 0 ? acc[mt * 4 + 0][r] : acc[mt * 4 + 1][r];
          const float a23 = nt == 2 ? acc[mt * 4 + 2][r] : acc[mt * 4 + 3][r];
          tgt[row] = nt < 2 ? a01 : a23;
        }
      }
    }
  } else {
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m_base + lrow0 + mt * 16 + r;
        if (row < M) {
          const float l = lse[row];
          const float sc = scale[row];
          const int64_t lab = labels[row];
          bf16* grow = g + (int64_t)row * V;
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const int gc = gc0 + nt * 16;
            const float p = expf(acc[mt * 4 + nt][r] - l);
            const float v = (p - (lab == gc ? 1.f : 0.f)) * sc;
            // an ignored row (scale 0) is all-zero bits whatever p is
            if (gc < V) grow[gc] = f2bf(sc == 0.f ? 0.f : v);
          }
        }
      }
    }
  }
}

// One block per row: lse = M + log(sum_p s_p * exp(m_p - M)) with M the max
// over the panels. Thread t takes panels t, t + 256, .. in ascending order;
// the threads then meet in a fixed tree (xor butterfly, then waves 0..3).
// A panel whose m equals M contributes s_p itself, so no exp(-inf - -inf)
// is ever formed and a thread without a panel contributes 0 without one.
__global__ __launch_bounds__(256) void head_ce_combine_kernel(
    const float2* __restrict__ ms,       // [P, M]
    const float* __restrict__ tgt,       // [M]
    const int64_t* __restrict__ labels,  // [M]
    float* __restrict__ lse,             // [M]
    float* __restrict__ loss_row,        // [M]
    int M, int P, int V) {
  const int row = blockIdx.x;
  __shared__ float wred[2][4];

  float mx = -INFINITY;
  for (int p = threadIdx.x; p < P; p += 256)
    mx = fmaxf(mx, ms[(int64_t)p * M + row].x);
  mx = wave_reduce_max(mx);
  if ((threadIdx.x & 63) == 0) wred[0][threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(wred[0][0], wred[0][1]), fmaxf(wred[0][2], wred[0][3]));

  float s = 0.f;
  for (int p = threadIdx.x; p < P; p += 256) {
    const float2 v = ms[(int64_t)p * M + row];
    s += v.x == mx ? v.y : v.y * expf(v.x - mx);
  }
  s = wave_reduce_sum(s);
  if ((threadIdx.x & 63) == 0) wred[1][threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = ((wred[1][0] + wred[1][1]) + wred[1][2]) + wred[1][3];
    const float l = mx + logf(s);
    lse[row] = l;
    const int64_t lab = labels[row];
    // tgt is unwritten for a label outside [0, V): never read it then
    float loss = 0.0f;
    if (lab >= 0 && lab < V) loss = l - tgt[row];
    loss_row[row] = loss;
  }
}

}  // namespace

extern "C" {

// ms: scratch [cdiv(V, 256) * M] float2 and tgt: scratch [M] float, both
// fully written before they are read; lse, loss_row: [M] float.
void tl_head_ce_stats(const void* x, const void* w, const void* labels,
                      void* ms, void* tgt, void* lse, void* loss_row, int M,
                      int V, int K, int rows_fast, hipStream_t stream) {
  const int P = cdiv(V, 256);
  hipLaunchKernelGGL(head_ce_kernel<0>, dim3(P * cdiv(M, 256)), dim3(512), 0,
                     stream, (const bf16*)x, (const bf16*)w,
                     (const int64_t*)labels, (float2*)ms, (float*)tgt,
                     (const float*)nullptr, (const float*)nullptr,
                     (bf16*)nullptr, M, V, K, rows_fast);
  hipLaunchKernelGGL(head_ce_combine_kernel, dim3(M), dim3(256), 0, stream,
                     (const float2*)ms, (const float*)tgt,
                     (const int64_t*)labels, (float*)lse, (float*)loss_row,
                     M, P, V);
}

// g: [M, V] bf16, every element written.
void tl_head_ce_grad(const void* x, const void* w, const void* labels,
                     const void* lse, const void* scale, void* g, int M,
                     int V, int K, int rows_fast, hipStream_t stream) {
  const int P = cdiv(V, 256);
  hipLaunchKernelGGL(head_ce_kernel<1>, dim3(P * cdiv(M, 256)), dim3(512), 0,
                     stream, (const bf16*)x, (const bf16*)w,
                     (const int64_t*)labels, (float2*)nullptr,
                     (float*)nullptr, (const float*)lse, (const float*)scale,
                     (bf16*)g, M, V, K, rows_fast);
}

}  // extern "C"
