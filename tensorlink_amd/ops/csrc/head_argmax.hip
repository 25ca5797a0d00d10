// Fused greedy head: tok[m] = argmax_n bf16(sum_k x[m,k] * W[n,k]) for the
// lm_head shape (N >= TL_GEMM_WIDE_N, n_split == 1). The [M, N] logits are
// never written: the C fragments are rounded to bf16, turned into ordered
// integer keys and reduced to one winner per row, first inside a 256-column
// panel (head_argmax_kernel), then over the panels (head_combine_kernel).
//
// SAME per-row accumulation as the rest of the family (gemm_family.hpp) at
// n_split == 1: the accumulators come from sq256_k_loop, the loop that
// gemm_tiled_sq_kernel (gemm_tiled.hip) writes out, over the whole of K,
// and get ONE rounding to bf16. Every logit is one K chain, so the values
// compared here are bit for bit the ones skinny_gemm / gemm_tiled_sq would have
// stored, and the token equals torch.argmax of their output. The loop's
// clamps make the tile whole for N % 256 != 0 and for the last row block.
//
// Comparison rule (torch.argmax on bf16): the greater value wins; among
// equal values the smallest column; -0 == +0; a NaN of either sign beats
// everything and the first NaN wins. pack_key maps a bf16 to a 16-bit key
// that is monotone in that order (NaN -> 0xFFFF, else 0x8000 + magnitude
// for positive and 0x8000 - magnitude for negative values, so both zeros
// share 0x8000) and puts 255 - (column in the panel) below it, so one
// unsigned max does value and tiebreak at once. 0 is below every real
// packed value (-inf is 0x0080....) and stands for "no column": the clamped
// loads duplicate row N - 1 into columns >= N of the last panel, which must
// take no part. Ghost rows (>= M) are computed and never written.

#include "gemm_family.hpp"

namespace {

DEVINLINE unsigned pack_key(float c, int panel_col) {
  const unsigned b = __bfloat16_as_ushort(f2bf(c));
  const unsigned mag = b & 0x7FFFu;
  // selects, not branches: this runs 128 times per lane
  const unsigned ord = (b & 0x8000u) ? 0x8000u - mag : 0x8000u + mag;
  const unsigned key = mag > 0x7F80u ? 0xFFFFu : ord;
  return key << 16 | (unsigned)(255 - panel_col);
}

__global__ __launch_bounds__(512, 1) void head_argmax_kernel(
    const bf16* __restrict__ x,        // [M, K]
    const bf16* __restrict__ w,        // [N, K]
    unsigned* __restrict__ best_out,   // [cdiv(N, 256), M] packed winners
    int M, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;          // 0..7
  const int col = lane & 15;
  const int wn = wave & 3;                    // 0..3: 64-col band
  const int m_base = blockIdx.z * 256;

  __shared__ bf16 lds[2][256 + 256][64];
  f32x4 acc[32];
  sq256_k_loop(x, w, m_base, blockIdx.x * 256, M, N, K,
               family_k_slice<0>(K, 1, 0), lds, acc, lane, wave);

  // Epilogue: one unsigned max per row over the panel's packed keys, 0 for
  // the ghost columns. The meeting place is the freed LDS ring.
  const int pc0 = wn * 64 + col;              // panel column of nt = 0
  const int gc0 = blockIdx.x * 256 + pc0;
  const unsigned best = sq256_row_reduce(
      reinterpret_cast<unsigned*>(&lds[0][0][0]), 0u,
      [&](int mt, int r, int nt) {
        const unsigned p = pack_key(acc[mt * 4 + nt][r], pc0 + nt * 16);
        return gc0 + nt * 16 < N ? p : 0u;
      },
      [](unsigned a, unsigned b) { return max(a, b); });
  const int row = threadIdx.x;
  if (row < 256 && m_base + row < M)
    best_out[(int64_t)blockIdx.x * M + m_base + row] = best;
}

// One block per row: the max over the panels' winners. A panel's packed
// value becomes (key, ~global column), so the greater key wins and among
// equal keys the smaller column, whichever panel it came from.
__global__ __launch_bounds__(256) void head_combine_kernel(
    const unsigned* __restrict__ best_in,  // [P, M]
    int64_t* __restrict__ tok,             // [M]
    int M, int P) {
  const int m = blockIdx.x;
  unsigned long long best = 0ull;
  for (int p = threadIdx.x; p < P; p += 256) {
    const unsigned v = best_in[(int64_t)p * M + m];
    const unsigned gcol = (unsigned)p * 256u + (255u - (v & 0xFFu));
    const unsigned long long c =
        (unsigned long long)(v >> 16) << 32 | (0xFFFFFFFFu - gcol);
    best = c > best ? c : best;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off, WAVE_SIZE);
    best = o > best ? o : best;
  }
  __shared__ unsigned long long wbest[4];
  if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 1; q < 4; ++q) best = wbest[q] > best ? wbest[q] : best;
    tok[m] = (int64_t)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
  }
}

}  // namespace

extern "C" {

// best: scratch [cdiv(N, 256) * M] uint32, fully written by the first
// kernel (no pre-zeroing, no atomics); tok: [M] int64.
void tl_head_argmax(const void* x, const void* w, void* best, void* tok,
                    int M, int N, int K, hipStream_t stream) {
  const int P = cdiv(N, 256);
  hipLaunchKernelGGL(head_argmax_kernel, dim3(P, 1, cdiv(M, 256)), dim3(512),
                     0, stream, (const bf16*)x, (const bf16*)w,
                     (unsigned*)best, M, N, K);
  hipLaunchKernelGGL(head_combine_kernel, dim3(M), dim3(256), 0, stream,
                     (const unsigned*)best, (int64_t*)tok, M, P);
}

}  // extern "C"
