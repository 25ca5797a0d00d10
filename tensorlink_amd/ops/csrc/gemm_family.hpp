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
// head_argmax.hip uses the helpers but repeats gemm_tiled_sq_kernel's K loop
// (staging order, vmcnt count, barriers) as text: a change to that loop has
// to be made in both, or the fused head stops seeing the family's bits.
// head_ce.hip (fused linear cross-entropy) holds a third copy of the same
// loop, one text for its two modes: the change goes there too.
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
