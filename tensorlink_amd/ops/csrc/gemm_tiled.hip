// Tiled serving GEMM for mid-M (65 <= M <= ~512+): out[M,N] = x[M,K] @
// W[N,K]^T (+bias). Companion to skinny_gemm.hip (M <= 64) under the
// family contract (gemm_family.hpp): a row's result is bitwise IDENTICAL
// for any M and either kernel. That property is what lets chunked prefill,
// speculative verify, batched decode and plain generate produce equal
// tokens (the serving engine's exact-greedy guarantee).
//
// Differences from skinny v5, both perf-motivated (guide §5 decode-GEMM
// notes):
//  * W panels are ALSO staged through LDS by global_load_lds, making the
//    k-loop all-glds: hipcc's counted-vmcnt scheduling survives (an
//    ordinary VGPR-destination load next to a glds forces vmcnt(0) at its
//    use — the v5 mixing trap), and the W fragment read becomes a
//    conflict-reduced b128 like the x fragments.
//  * blockIdx.z tiles M in 256-row blocks, so serving batches beyond 256
//    rows (chunked-prefill chunks, big decode batches) stay on this
//    kernel.
// Grid (N/64, n_split, ceil(M/256)); block = 4 waves; wave w owns output
// columns [blk.x*64 + w*16, +16).

#include "gemm_family.hpp"

namespace {

constexpr int BLOCK = 256;

template <int MT, int HAS_BIAS, int SPLIT>
__global__ __launch_bounds__(BLOCK, 2) void gemm_tiled_kernel(
    const bf16* __restrict__ x,     // [M, K]
    const bf16* __restrict__ w,     // [N, K]
    const bf16* __restrict__ bias,  // [N] or null
    bf16* __restrict__ out,         // [M, N]
    float* __restrict__ partial,    // [SPLITK, M, N] when SPLIT
    int M, int N, int K, int n_split) {
  constexpr int MPW = MT / 4;                 // m-tiles per wave
  static_assert(MT % 4 == 0, "quadrant layout needs MT % 4 == 0");
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int quad = lane >> 4;
  const int m_base = blockIdx.z * (MT * 16);

  const int split = SPLIT ? blockIdx.y : 0;
  const KSlice ks = family_k_slice<SPLIT>(K, n_split, split);

  // ONE shared object (a second one de-pipelines glds: guide §5 trap 4a).
  // Layout: [2 buffers][MT*16 x-rows + 64 w-rows][64 k], each part a
  // swizzled image (gemm_family.hpp).
  __shared__ bf16 lds[2][MT * 16 + 64][64];

  f32x4 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int GPW = MT / 2;                 // x glds pieces per wave
  const int l8 = lane >> 3;

  // x rows piece*8+l8 (clamped to M) and W rows wpiece*8+l8 of this
  // block's 64-column panel, 1 KB per instruction.
  auto stage = [&](int bufi, int k0) {
    if (k0 >= ks.end) return;
#pragma unroll
    for (int g = 0; g < GPW; ++g) {
      const int piece = wave * GPW + g;
      const int xr = min(m_base + piece * 8 + l8, M - 1);
      stage_8x64(x + (int64_t)xr * K, lane, k0, K, &lds[bufi][piece * 8][0]);
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int wpiece = wave * 2 + g;
      const int wr = wpiece * 8 + l8;
      stage_8x64(w + ((int64_t)blockIdx.x * 64 + wr) * K, lane, k0, K,
                 &lds[bufi][MT * 16 + wpiece * 8][0]);
    }
  };

  // Counted-vmcnt double-buffer pipeline: tile t+1's glds stay in flight
  // across the barrier (each wave issues a fixed LPT loads per tile —
  // MT/2 x-pieces + 2 W-pieces, wave-uniform for MT in {8,16} — waits
  // for its OWN tile-t loads with vmcnt(LPT), then the barrier aligns
  // the workgroup, so tile t is fully in LDS without draining t+1).
  constexpr int LPT = MT / 2 + 2;
  static_assert(MT == 8 || MT == 16, "LPT assumes wave-uniform pieces");
  stage(0, ks.begin);
  int buf = 0;
  for (int k0 = ks.begin; k0 < ks.end; k0 += 64) {
    if (k0 + 64 < ks.end) {
      stage(buf ^ 1, k0 + 64);                // in flight under compute
      waitcnt_vm<LPT>();                      // tile t landed; t+1 out
    } else {
      waitcnt_vm<0>();                        // last tile: drain
    }
    __builtin_amdgcn_s_barrier();
    const int tile_k = min(64, ks.end - k0);
    const bf16* xt = &lds[buf][0][0];
    const bf16* wt = &lds[buf][MT * 16][0];
    // 2D fragment reuse: this wave owns a (MT/4 x 4)-tile quadrant —
    // rows [wave*MPW*16, +MPW*16), all 64 panel columns — so each kk
    // reads MPW a-frags + 4 b-frags and issues 4*MPW mfmas (the 1D
    // col-strip layout read one a-frag PER mfma and was LDS-issue
    // bound at ~1.9 TB/s on wide-N shapes).
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if (kk * 32 < tile_k) {
        bf16x8_t bfrag[4], afrag[MPW];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          bfrag[nt] = lds_frag(wt, nt * 16 + col, kk * 4 + quad);
#pragma unroll
        for (int mt = 0; mt < MPW; ++mt)
          afrag[mt] = lds_frag(xt, wave * (MPW * 16) + mt * 16 + col,
                               kk * 4 + quad);
#pragma unroll
        for (int mt = 0; mt < MPW; ++mt)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            acc[mt * 4 + nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag[mt], bfrag[nt], acc[mt * 4 + nt], 0, 0, 0);
      }
    }
    // all waves done reading buf before the next iteration's glds
    // overwrite it (hipcc has already counted-waited the ds_reads into
    // the mfmas; lgkmcnt(0) makes that explicit before the raw barrier)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    buf ^= 1;
  }

#pragma unroll
  for (int mt = 0; mt < MPW; ++mt) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int oc = blockIdx.x * 64 + nt * 16 + col;
      const int row0 = m_base + wave * (MPW * 16) + mt * 16;
      if (SPLIT) {
        store_cfrag_partial(acc[mt * 4 + nt],
                            partial + (int64_t)split * M * N, row0, M, N, oc,
                            quad);
      } else {
        const float b = HAS_BIAS ? bf2f(bias[oc]) : 0.f;
        store_cfrag_bf16(acc[mt * 4 + nt] + b, out, row0, M, N, oc, quad);
      }
    }
  }
}

// Big-tile variant: 256x256 block tile, 8 waves (2M x 4N quadrants of
// 128x64), 128 KB LDS, 1 block/CU. For wide-N (gate_up, lm_head) and
// deep-K (down_proj) shapes the dominant cost in the BN=64 kernel is
// re-reading the x slab once per output panel (N/BN * M*K*2 bytes, L3-
// served at ~10 TB/s); BN=256 makes x:W traffic 1:1. Per-iteration MFMA
// work (256 mfma/block) is also long enough to hide the glds latency
// that starves the small-tile kernels. Handles N % 256 != 0 (lm_head
// 151936) with clamped W loads + guarded stores.
// The K loop below is sq256_k_loop (gemm_family.hpp), which the fused
// heads call, written out: called from here it cost this kernel 2 us in
// 350 at the lm_head shape (profiles/sq256_loop_refactor.md). The two
// texts are to be kept equal; tests/test_head_argmax_gpu.py and
// tests/test_fused_ce_gpu.py compare the heads with this kernel bit for bit.
template <int HAS_BIAS, int SPLIT>
__global__ __launch_bounds__(512, 1) void gemm_tiled_sq_kernel(
    const bf16* __restrict__ x,     // [M, K]
    const bf16* __restrict__ w,     // [N, K]
    const bf16* __restrict__ bias,  // [N] or null
    bf16* __restrict__ out,         // [M, N]
    float* __restrict__ partial,    // [SPLITK, M, N] when SPLIT
    int M, int N, int K, int n_split) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;          // 0..7
  const int col = lane & 15;
  const int quad = lane >> 4;
  const int wm = wave >> 2;                   // 0..1: 128-row band
  const int wn = wave & 3;                    // 0..3: 64-col band
  const int m_base = blockIdx.z * 256;

  const int split = SPLIT ? blockIdx.y : 0;
  const KSlice ks = family_k_slice<SPLIT>(K, n_split, split);

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

#pragma unroll
  for (int mt = 0; mt < 8; ++mt) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int oc = blockIdx.x * 256 + wn * 64 + nt * 16 + col;
      const int row0 = m_base + wm * 128 + mt * 16;
      if (oc < N) {
        if (SPLIT) {
          store_cfrag_partial(acc[mt * 4 + nt],
                              partial + (int64_t)split * M * N, row0, M, N,
                              oc, quad);
        } else {
          const float b = HAS_BIAS ? bf2f(bias[oc]) : 0.f;
          store_cfrag_bf16(acc[mt * 4 + nt] + b, out, row0, M, N, oc, quad);
        }
      }
    }
  }
}

template <int MT>
void tiled_launch_mt(const void* x, const void* w, const void* bias,
                     void* out, void* partial, int M, int N, int K,
                     int n_split, hipStream_t stream) {
  launch_variant(gemm_tiled_kernel<MT, 0, 1>, gemm_tiled_kernel<MT, 1, 0>,
                 gemm_tiled_kernel<MT, 0, 0>, n_split, bias,
                 dim3(N / 64, n_split, cdiv(M, MT * 16)), dim3(BLOCK), stream,
                 x, w, bias, out, partial, M, N, K, n_split);
}

}  // namespace

extern "C" {

// partial: scratch [n_split * M * N] floats (only used when n_split > 1).
// reduce == 0 leaves the fp32 partials for the consumer (see
// skinny_gemm.hip).
void tl_gemm_tiled(const void* x, const void* w, const void* bias, void* out,
                   void* partial, int M, int N, int K, int n_split,
                   int reduce, hipStream_t stream) {
  // very-wide-N shapes (lm_head) take the 256x256 8-wave kernel; at
  // gate_up/down widths the BN=64 kernel measures faster (see
  // profiles/gemm_family_ab.md). Dispatch is by (N, K) only -> the
  // choice is M-independent
  if (N >= TL_GEMM_WIDE_N)
    launch_variant(gemm_tiled_sq_kernel<0, 1>, gemm_tiled_sq_kernel<1, 0>,
                   gemm_tiled_sq_kernel<0, 0>, n_split, bias,
                   dim3(cdiv(N, 256), n_split, cdiv(M, 256)), dim3(512),
                   stream, x, w, bias, out, partial, M, N, K, n_split);
  else if (M <= 128)
    tiled_launch_mt<8>(x, w, bias, out, partial, M, N, K, n_split, stream);
  else
    tiled_launch_mt<16>(x, w, bias, out, partial, M, N, K, n_split, stream);
  if (n_split > 1 && reduce)
    launch_splitk_reduce(partial, bias, out, M, N, n_split, stream);
}

}  // extern "C"
