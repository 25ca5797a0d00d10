// The GEMM family's shared contract, in code. Members: skinny_gemm,
// gemm_tiled, gemm_tiled_sq, gemm_colbal, moe_gemm, and through
// mxfp4_common.hpp mxfp4_gemm and mxfp4_moe_gemm.
//
// A row's result is bitwise the same from every bf16 member, at every M,
// in every batch, because all of them
//   * step K in fixed chunks from the split's start (family_k_slice, which
//     is gemm_policy.hpp's gemm_k_slice: the splits cover [0, K) exactly,
//     a 32-wide K tail being the last chunk of the last non-empty split),
//     two mfma_f32_16x16x32_bf16 per 64-k chunk in kk order, f32
//     accumulators, a 32-wide tail taking kk = 0 only;
//   * take the split count from gemm_policy.hpp, pure in (N, K);
//   * reduce split partials in ascending split order from 0.f, then bias,
//     then ONE bf16 rounding (splitk_reduce_kernel; the partials consumers
//     in rmsnorm.hip / rope_append.hip reproduce exactly that sum).
// Change any of it here and every member changes with it — EXCEPT the
// copies that four kernels still write out themselves because a check
// failed with the helper (profiles/gemm_family_refactor.md §0):
//   skinny_gemm.hip    slice, staging piece, fragment read, epilogue
//   moe_gemm.hip       staging piece, fragment read, epilogue
//   mxfp4_gemm.hip, mxfp4_moe_gemm.hip   slice (mxfp4_k_per), epilogue,
//                      and the 128-k step body, the same text in both
// A change to the swizzle or the slice has to be made there too.
//
// The 256x256-tile K loop is sq256_k_loop below: the two fused heads
// (head_argmax.hip, head_ce.hip; three kernels) call it, and their per-row
// reduce over a panel is sq256_row_reduce. gemm_tiled_sq_kernel still
// writes the same loop out, because calling the helper made it 0.5 - 0.8 %
// slower at the lm_head shape with the loop's instructions unchanged
// (profiles/sq256_loop_refactor.md §4): a change to that loop has to be
// made in gemm_tiled.hip too, or the heads stop seeing the family's bits.
// gemm_tiled_kernel<MT> keeps a loop
// of its own, the same shape with other constants: as one template
// with this one it lost 4 VGPRs at MT = 8 and gained an s_waitcnt at MT =
// 16 (profiles/sq256_loop_refactor.md §0), and a template is not kept for
// one shape.
//
// The helpers take pointers and scalars and own no state, on purpose:
// guarded accumulator updates send acc[] to scratch, a second __shared__
// object de-pipelines global_load_lds, and an ordinary VGPR load next to a
// glds forces vmcnt(0). Kernels keep their one LDS object and their
// accumulator arrays; nothing here declares either.
#pragma once

#include "common.hpp"

// The one split-K reduce (splitk_reduce.hip): partial [n_split, M, N] fp32
// -> out [M, N] bf16, summed in ascending split order from 0.f, then bias
// ([N] or null), then one rounding.
void launch_splitk_reduce(const void* partial, const void* bias, void* out,
                          int64_t M, int N, int n_split, hipStream_t stream);

namespace {

// counted VMEM wait with a compile-time immediate — invisible to hipcc's
// waitcnt pass, so a glds pipeline is not drained at barriers (a plain
// __syncthreads with a glds in flight emits vmcnt(0))
template <int N>
DEVINLINE void waitcnt_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// global_load_lds, 16 bytes per lane (HBM -> LDS DMA, no staging
// registers). The LDS side is lane-linear: lane l lands at lds_dst + l*16,
// lds_dst wave-uniform; src is this lane's own address.
DEVINLINE void glds16(const void* src, void* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// ---------------------------------------------------------------------------
// Swizzled 64-k LDS image. A tile is rows of 64 bf16 (128 B = 8 slots of
// 16 B) with no padding, since glds writes are lane-linear. The bank
// swizzle therefore sits on the SOURCE address:
//
//     physical slot p of row r holds logical k-slot p ^ (r & 7)
//
// stage_8x64 writes by that rule and lds_frag reads by it; a mismatch is
// silent wrong data, so both live here, side by side. skinny_gemm.hip and
// moe_gemm.hip carry their own copy of the pair (see the top of this
// file): the same rule, to be kept equal. The XOR permutes within one
// row's 128 B, so the global fetch stays whole lines.
// ---------------------------------------------------------------------------

// One glds instruction: 8 rows x 64 k (1 KB) into `piece`, whose first row
// must sit at a multiple of 8 rows in its tile. Lane l fills physical slot
// l & 7 of row l >> 3 from `src_row`, that row's source (element 0 of the
// row; the caller picks and clamps it with the same l >> 3). Slots past K
// re-read the row's last 8 elements: in bounds, and never used by an MFMA.
DEVINLINE void stage_8x64(const bf16* src_row, int lane, int k0, int K,
                          bf16* piece) {
  const int l8 = lane >> 3, c8 = lane & 7;
  glds16(src_row + min(k0 + (c8 ^ l8) * 8, K - 8), piece);
}

// The 8 bf16 of logical k-slot `kslot` (k = kslot * 8 .. + 7 of the chunk)
// of row `row` of a tile staged as above: one ds_read_b128. An MFMA
// fragment of half kk takes kslot = kk * 4 + quad.
DEVINLINE bf16x8_t lds_frag(const bf16* tile, int row, int kslot) {
  return *reinterpret_cast<const bf16x8_t*>(
      tile + row * 64 + ((kslot ^ (row & 7)) * 8));
}

// ---------------------------------------------------------------------------
// Split-K slice: gemm_k_slice of gemm_policy.hpp, where the bindings and the
// tests read the same function — whole 64-k chunks, a 32-wide tail counting
// as one, ceil-divided over the splits, so the slices cover K exactly; a
// trailing split may be empty and then contributes zeros. SPLIT == 0 is the
// whole of K.
// ---------------------------------------------------------------------------
template <int SPLIT>
DEVINLINE KSlice family_k_slice(int K, int n_split, int split) {
  if (!SPLIT) return {0, K};
  return gemm_k_slice(K, n_split, split);
}

// ---------------------------------------------------------------------------
// C-fragment store: lane (col, quad) of mfma_f32_16x16x32_bf16 holds
// C[quad * 4 + r][col], r = 0..3, of a 16-row tile whose first row is row
// `row0` of `base` (row stride `ld`); `col` is this lane's column there and
// rows >= row_end are not stored. Two forms: the fp32 split partial (base =
// this split's [M, N] slab), and the bf16 output — whose caller passes
// acc + bias (0.f without one) or acc * scale, so the one rounding happens
// here.
// ---------------------------------------------------------------------------
DEVINLINE void store_cfrag_partial(f32x4 c, float* base, int row0,
                                   int row_end, int ld, int col, int quad) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + quad * 4 + r;
    if (row < row_end) base[(int64_t)row * ld + col] = c[r];
  }
}

DEVINLINE void store_cfrag_bf16(f32x4 c, bf16* base, int row0, int row_end,
                                int ld, int col, int quad) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + quad * 4 + r;
    if (row < row_end) base[(int64_t)row * ld + col] = f2bf(c[r]);
  }
}

// ---------------------------------------------------------------------------
// The 256x256-tile K loop: acc = x[m_base .. +256, ks] @ w[n_base .. +256,
// ks]^T, from zeroed accumulators. 512 threads, 8 waves as 2(M) x 4(N)
// quadrants of 128 x 64; lane (col, quad) of wave (wm, wn) ends with
//   acc[mt * 4 + nt][r] = C[wm*128 + mt*16 + quad*4 + r][wn*64 + nt*16 + col]
// `lds` is the calling kernel's one shared object, used as a double buffer
// of [256 x rows + 256 W rows][64 k] swizzled images, all staged by glds:
// each wave issues 4 x pieces and 4 W pieces per tile, waits for its own
// tile-t loads with vmcnt(8) while tile t+1's stay in flight, and the raw
// barrier aligns the workgroup. x rows are clamped to M - 1 and W rows to
// N - 1: rows >= M and columns >= N of the tile hold duplicates, for the
// caller to leave out. On return every wave is past the last fragment read
// and no glds is in flight, so the caller may reuse `lds`.
// head_argmax_kernel and head_ce_kernel are this loop plus an epilogue, and
// gemm_tiled_sq_kernel is the same text plus its store, which is why the
// fused heads see the family's bits.
// The caller passes its own `lane` (threadIdx.x & 63) and `wave`
// (threadIdx.x >> 6).
// ---------------------------------------------------------------------------
DEVINLINE void sq256_k_loop(const bf16* __restrict__ x,
                            const bf16* __restrict__ w, int m_base,
                            int n_base, int M, int N, int K, KSlice ks,
                            bf16 (&lds)[2][256 + 256][64],
                            f32x4 (&acc)[32], int lane, int wave) {
  const int col = lane & 15;
  const int quad = lane >> 4;
  const int wm = wave >> 2;                   // 0..1: 128-row band
  const int wn = wave & 3;                    // 0..3: 64-col band
  const int l8 = lane >> 3;

#pragma unroll
  for (int m = 0; m < 32; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};

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
      const int gr = min(n_base + wpiece * 8 + l8, N - 1);
      stage_8x64(w + (int64_t)gr * K, lane, k0, K,
                 &lds[bufi][256 + wpiece * 8][0]);
    }
  };

  stage(0, ks.begin);
  int buf = 0;
  for (int k0 = ks.begin; k0 < ks.end; k0 += 64) {
    if (k0 + 64 < ks.end) {
      stage(buf ^ 1, k0 + 64);                // in flight under compute
      waitcnt_vm<8>();                        // tile t landed; t+1 out
    } else {
      waitcnt_vm<0>();                        // last tile: drain
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
    // all waves done reading buf before the next iteration's glds overwrite
    // it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    buf ^= 1;
  }
}

// ---------------------------------------------------------------------------
// Row reduce over the 256 columns of a sq256_k_loop tile, for the fused
// heads. val(mt, r, nt) is the calling lane's value for accumulator element
// acc[mt * 4 + nt][r] (`init` for a column that takes no part); op combines
// two values. Fixed order per row: the lane's nt = 0..3 from `init`, then
// the 16 lanes of the column group by xor offsets 1, 2, 4, 8 — lane `col`
// keeps rows col and col + 16 of the group's 32 (index mt * 4 + r) — then
// the four wn waves meet in `red`, a [4 wn][256 rows] image in the freed
// LDS, and thread t < 256 returns ((r0 op r1) op r2) op r3 of tile row t.
// Threads >= 256 return `init`. Ends behind a __syncthreads; a second call
// on the same `red` needs one more in between.
// ---------------------------------------------------------------------------
template <typename T, typename Val, typename Op>
DEVINLINE T sq256_row_reduce(T* red, T init, Val val, Op op) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int quad = lane >> 4;
  const int wm = wave >> 2;
  const int wn = wave & 3;

  T keep[2] = {init, init};
#pragma unroll
  for (int mt = 0; mt < 8; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      T v = init;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) v = op(v, val(mt, r, nt));
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        v = op(v, __shfl_xor(v, off, WAVE_SIZE));
      if (((mt * 4 + r) & 15) == col) keep[(mt * 4 + r) >> 4] = v;
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int idx = h * 16 + col;             // = mt * 4 + r
    const int row = wm * 128 + (idx >> 2) * 16 + quad * 4 + (idx & 3);
    red[wn * 256 + row] = keep[h];
  }
  __syncthreads();
  T out = init;
  if (threadIdx.x < 256) {
    const int row = threadIdx.x;
    out = op(op(op(red[row], red[256 + row]), red[512 + row]),
             red[768 + row]);
  }
  return out;
}

// Launch the variant of a <HAS_BIAS, SPLIT> kernel that a call needs: the
// split one when n_split > 1 (bias then belongs to the reduce), else the
// bias one, else the plain one. All three take the same arguments; a
// variant ignores those its template flags switch off.
template <typename... P, typename... A>
inline void launch_variant(void (*k_split)(P...), void (*k_bias)(P...),
                           void (*k_plain)(P...), int n_split,
                           const void* bias, dim3 grid, dim3 block,
                           hipStream_t stream, A... args) {
  auto kernel = n_split > 1 ? k_split : bias ? k_bias : k_plain;
  hipLaunchKernelGGL(kernel, grid, block, 0, stream,
                     static_cast<P>(args)...);
}

}  // namespace
