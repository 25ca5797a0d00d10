// Fused greedy head: tok[m] = argmax_n bf16(sum_k x[m,k] * W[n,k]) for the
// lm_head shape (N >= TL_GEMM_WIDE_N, n_split == 1). The [M, N] logits are
// never written: the C fragments are rounded to bf16, turned into ordered
// integer keys and reduced to one winner per row, first inside a 256-column
// panel (head_argmax_kernel), then over the panels (head_combine_kernel).
//
// SAME per-row accumulation as the rest of the family (gemm_family.hpp) at
// n_split == 1: K stepped in 64-element chunks from 0, two
// mfma_f32_16x16x32_bf16 per chunk in kk order, f32 accumulators, a 32-wide
// tail taking kk = 0 only, ONE rounding to bf16. Every logit is one K chain,
// so the values compared here are bit for bit the ones skinny_gemm /
// gemm_tiled_sq would have stored, and the token equals torch.argmax of
// their output. The K loop is gemm_tiled_sq_kernel's (gemm_tiled.hip),
// repeated as text: 256x256 tile, 8 waves as 2(M) x 4(N), 128 KB LDS in one
// object, all-glds staging, counted vmcnt, raw barriers, clamped W rows for
// N % 256 != 0 and clamped x rows for the last row block. Do not change it
// here without changing it there.
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
  const int quad = lane >> 4;
  const int wm = wave >> 2;                   // 0..1: 128-row band
  const int wn = wave & 3;                    // 0..3: 64-col band
  const int m_base = blockIdx.z * 256;

  const KSlice ks = family_k_slice<0>(K, 1, 0);

  __shared__ bf16 lds[2][256 + 256][64];

  f32x4 acc[32];
#pragma unroll
  for (int m = 0; m < 32; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int l8 = lane >> 3;

  // x: 32 pieces of 8 rows -> 4 per wave; W: 32 pieces -> 4 per wave
  auto stage = [&](int bufi, int k0) {
    if (k0 >= ks.end) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int piece = wave * 4 + g;
      const int xr = min(m_base + piece * 8 + l8, M - 1);
      stage_8x64(x + (int64_t)xr * K, lane, k0, K, &lds[bufi][piece * 8][0]);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int wpiece = wave * 4 + g;
      const int gr = min((int)blockIdx.x * 256 + wpiece * 8 + l8, N - 1);
      stage_8x64(w + (int64_t)gr * K, lane, k0, K,
                 &lds[bufi][256 + wpiece * 8][0]);
    }
  };

  stage(0, ks.begin);
  int buf = 0;
  for (int k0 = ks.begin; k0 < ks.end; k0 += 64) {
    if (k0 + 64 < ks.end) {
      stage(buf ^ 1, k0 + 64);
      waitcnt_vm<8>();                        // tile t landed; t+1 out
    } else {
      waitcnt_vm<0>();
    }
    __builtin_amdgcn_s_barrier();
    const int tile_k = min(64, ks.end - k0);
    const bf16* xt = &lds[buf][0][0];
    const bf16* wt = &lds[buf][256][0];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if (kk * 32 < tile_k) {
        bf16x8_t bfrag[4], afrag[8];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          bfrag[nt] = lds_frag(wt, wn * 64 + nt * 16 + col, kk * 4 + quad);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt)
          afrag[mt] = lds_frag(xt, wm * 128 + mt * 16 + col, kk * 4 + quad);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            acc[mt * 4 + nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag[mt], bfrag[nt], acc[mt * 4 + nt], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    buf ^= 1;
  }

  // Epilogue. Lane (col, quad) holds C[mt*16 + quad*4 + r][nt*16 + col] of
  // its wave's 128 x 64 quadrant. Per row: max over the lane's 4 nt
  // registers, then over the 16 lanes of the column group; afterwards all
  // 16 lanes hold the row's winner, and lane `col` keeps rows col and
  // col + 16 of the group's 32 (index mt*4 + r).
  const int pc0 = wn * 64 + col;              // panel column of nt = 0
  const int gc0 = blockIdx.x * 256 + pc0;
  unsigned keep[2] = {0u, 0u};
#pragma unroll
  for (int mt = 0; mt < 8; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      unsigned best = 0u;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const unsigned p = pack_key(acc[mt * 4 + nt][r], pc0 + nt * 16);
        best = max(best, gc0 + nt * 16 < N ? p : 0u);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        best = max(best, (unsigned)__shfl_xor((int)best, off, WAVE_SIZE));
      if (((mt * 4 + r) & 15) == col) keep[(mt * 4 + r) >> 4] = best;
    }
  }

  // The 4 wn waves of a row meet in LDS: the ring is free (the loop's last
  // barrier is behind every wave's last fragment read, and its vmcnt(0)
  // left no glds in flight). Image [4 wn][256 rows] of packed winners.
  unsigned* red = reinterpret_cast<unsigned*>(&lds[0][0][0]);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int idx = h * 16 + col;             // = mt * 4 + r
    const int row = wm * 128 + (idx >> 2) * 16 + quad * 4 + (idx & 3);
    red[wn * 256 + row] = keep[h];
  }
  __syncthreads();
  if (threadIdx.x < 256) {
    const int row = threadIdx.x;
    unsigned best = red[row];
#pragma unroll
    for (int q = 1; q < 4; ++q) best = max(best, red[q * 256 + row]);
    if (m_base + row < M)
      best_out[(int64_t)blockIdx.x * M + m_base + row] = best;
  }
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
