// Per-head q/k RMSNorm + RoPE + KV-cache append for gfx950 (Qwen3).
//
// One launch takes the fused-QKV projection's row — bf16, or the GEMM
// family's fp32 split-K partials (+ bias) — and does what the qk-norm models
// used to spend a split, two .contiguous(), two rmsnorm launches, a cat and
// rope_append on: normalise every q head with q_norm[D] and every k head
// with k_norm[D], rotate, write q to the contiguous [T, Hq, D] output and
// rotated k / raw v into the cache ([B, Hkv, Smax, D], or page pools
// [n_pages, Hkv, 128, D] behind block_table).
//
// Layout. A lane owns one 8-column group (16 bytes) of one head; a head is
// D/8 consecutive lanes (16 at D = 128, 8 at D = 64), so a 256-thread block
// covers 16 or 32 heads per sweep over the Hq + 2*Hkv heads of a token, and
// the grid is (T, sweeps): no block loops (grid.y = 1 makes one block walk
// all sweeps; same bits). Everything stays in registers — no LDS, no
// barrier:
//   * partials: the lane's group is one sum_partials8 group (from 0.f,
//     ascending split order, then the bias, one bf16 rounding);
//   * norm: the lane's 8 squares, then xor shuffles inside the head's lane
//     group;
//   * rotation: element d pairs with d + D/2, which lives D/16 lanes away —
//     the 8 normalised bf16 values cross as 4 packed dwords in __shfl_xor;
//   * every output leaves as one 16-byte store.
// Control flow is uniform per wave: lanes past the last head clamp their
// head index and skip only the store; q / k / v differ by select.
//
// Bit contract: every output equals the chain it replaces — the family
// reduce, rmsnorm_fwd_kernel<1,0,0> per head, rope_append_kernel. The
// arithmetic below is spelled the way those two kernels COMPILE, with
// contraction off for this file so that the compiler cannot choose again:
//   * rmsnorm: squares are rounded products (v_pk_mul_f32) added in element
//     order — not an fma chain; its wave reduce's 32/16(/8) steps and its
//     LDS sum add exact zeros for an H = D row; rsqrtf(total / D + eps);
//     (f * rstd) * w as two rounded products;
//   * rope: the lower half is fma(x1, c, -(x2 * s)), the upper half
//     fma(x1, s, x2 * c) — there the rounded product is the lane's own
//     element, the fused one its partner's; the angle is
//     __sincosf(fpos * inv_freq[d]).

#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;

union pack8 {
  bf16x8 h;
  unsigned u[4];
};

template <int D, int PAGED, int PART>
__global__ __launch_bounds__(BLOCK) void qknorm_rope_append_kernel(
    const void* __restrict__ qkv, const bf16* __restrict__ bias,
    const bf16* __restrict__ q_norm, const bf16* __restrict__ k_norm,
    bf16* __restrict__ q_out, bf16* __restrict__ k_cache,
    bf16* __restrict__ v_cache, const int* __restrict__ positions,
    const void* __restrict__ inv_freq, const int* __restrict__ block_table,
    int S, int Hq, int Hkv, int Smax, int bt_stride, int n_split,
    int64_t split_stride, int inv_bf16, float eps) {
  constexpr int LPH = D / 8;         // lanes per head
  constexpr int HPB = BLOCK / LPH;   // heads per sweep
  const int64_t token = blockIdx.x;
  const int b = token / S;
  const int pos = positions[token];
  int64_t slot;   // cache slot index (in units of D elems, per kv head 0)
  if (PAGED) {
    const int page = block_table[b * bt_stride + (pos >> 7)];
    slot = ((int64_t)page * Hkv) * 128 + (pos & 127);
  } else {
    slot = ((int64_t)b * Hkv) * Smax + pos;
  }
  const int64_t head_stride = PAGED ? 128 : Smax;
  const int NH = Hq + 2 * Hkv;
  const int64_t row_stride = (int64_t)NH * D;
  const int t = threadIdx.x % LPH;    // 8-column group inside the head
  const int hs = threadIdx.x / LPH;   // head slot inside the sweep
  const bool upper = t >= LPH / 2;

  // the lane's 8 angles d = (8t + j) mod D/2 hold for every head and sweep.
  // out = fma(a, fa, b * fb) with, in the lower half, a = mine, fa = c,
  // b = other, fb = -s; in the upper half a = other, fa = s, b = mine, fb = c
  float fa[8], fb[8];
  {
    const float fpos = (float)pos;
    const int d0 = 8 * (t % (LPH / 2));
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float fr = inv_bf16 ? bf2f(((const bf16*)inv_freq)[d0 + j])
                                : ((const float*)inv_freq)[d0 + j];
      float s, c;
      __sincosf(fpos * fr, &s, &c);
      fa[j] = upper ? s : c;
      fb[j] = upper ? c : -s;
    }
  }
  const bf16x8 wq = *reinterpret_cast<const bf16x8*>(q_norm + t * 8);
  const bf16x8 wk = *reinterpret_cast<const bf16x8*>(k_norm + t * 8);

  for (int sweep = blockIdx.y; sweep * HPB < NH; sweep += gridDim.y) {
    int head = sweep * HPB + hs;
    const bool live = head < NH;
    head = min(head, NH - 1);
    const bool is_q = head < Hq;
    const bool is_v = head >= Hq + Hkv;
    const int64_t col = (int64_t)head * D + t * 8;

    // the row's 8 values as the family's reduce would have written them
    bf16x8 x;
    if constexpr (PART) {
      const float* pp[1] = {(const float*)qkv + token * row_stride + col};
      float acc[1][8];
      sum_partials8<1, 4>(pp, split_stride, n_split, acc);
      if (bias) {
        const bf16x8 vb = *reinterpret_cast<const bf16x8*>(bias + col);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          x.v[j] = f2bf(acc[0][j] + bf2f(vb.v[j]));
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x.v[j] = f2bf(acc[0][j]);
      }
    } else {
      x = *reinterpret_cast<const bf16x8*>((const bf16*)qkv +
                                           token * row_stride + col);
    }

    // per-head RMSNorm (v lanes run it too and drop the result)
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = bf2f(x.v[j]);
    float sumsq = f[0] * f[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) sumsq = sumsq + f[j] * f[j];
    sumsq = group_reduce_sum<LPH>(sumsq);
    const float rstd = rsqrtf(sumsq / (float)D + eps);
    const bf16x8 w = is_q ? wq : wk;
    pack8 y, o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      y.h.v[j] = f2bf((f[j] * rstd) * bf2f(w.v[j]));

    // rotate: the partner half of the head sits LPH/2 lanes away
#pragma unroll
    for (int i = 0; i < 4; ++i)
      o.u[i] = __shfl_xor(y.u[i], LPH / 2, WAVE_SIZE);
    bf16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float mine = bf2f(y.h.v[j]), other = bf2f(o.h.v[j]);
      const float r = __builtin_fmaf(upper ? other : mine, fa[j],
                                     (upper ? mine : other) * fb[j]);
      out.v[j] = is_v ? x.v[j] : f2bf(r);
    }

    bf16* dst;
    if (is_q) {
      dst = q_out + (token * Hq + head) * D;
    } else {
      const int hk = head - Hq - (is_v ? Hkv : 0);
      dst = (is_v ? v_cache : k_cache) + (slot + hk * head_stride) * D;
    }
    if (live) *reinterpret_cast<bf16x8*>(dst + t * 8) = out;
  }
}

template <int D, int PART>
void launch(const void* qkv, const void* bias, const void* q_norm,
            const void* k_norm, void* q_out, void* k_cache, void* v_cache,
            const void* positions, const void* inv_freq,
            const void* block_table, int64_t T, int S, int Hq, int Hkv,
            int Smax, int bt_stride, int n_split, int inv_bf16, float eps,
            int one_block, hipStream_t stream) {
  constexpr int HPB = BLOCK / (D / 8);
  const int NH = Hq + 2 * Hkv;
  dim3 grid((uint32_t)T, one_block ? 1 : cdiv(NH, HPB)), block(BLOCK);
  const int64_t split_stride = T * (int64_t)NH * D;
#define GO(PAGED)                                                           \
  hipLaunchKernelGGL((qknorm_rope_append_kernel<D, PAGED, PART>), grid,     \
                     block, 0, stream, qkv, (const bf16*)bias,              \
                     (const bf16*)q_norm, (const bf16*)k_norm,              \
                     (bf16*)q_out, (bf16*)k_cache, (bf16*)v_cache,          \
                     (const int*)positions, inv_freq,                       \
                     (const int*)block_table, S, Hq, Hkv, Smax, bt_stride,  \
                     n_split, split_stride, inv_bf16, eps)
  if (block_table) GO(1);
  else GO(0);
#undef GO
}

}  // namespace

extern "C" {

// n_split == 0: qkv is bf16 [T, (Hq+2Hkv)*D] and bias is ignored.
// n_split  > 0: qkv is fp32 partials [n_split, T, (Hq+2Hkv)*D], bias bf16
// or null. D must be 64 or 128 (the caller checks). one_block != 0 launches
// one block per token instead of one per (token, sweep).
void tl_qknorm_rope_append(const void* qkv, const void* bias,
                           const void* q_norm, const void* k_norm,
                           void* q_out, void* k_cache, void* v_cache,
                           const void* positions, const void* inv_freq,
                           const void* block_table, int64_t T, int S, int Hq,
                           int Hkv, int D, int Smax, int bt_stride,
                           int n_split, int inv_bf16, float eps,
                           int one_block, hipStream_t stream) {
#define GO(DD, PP)                                                          \
  launch<DD, PP>(qkv, PP ? bias : nullptr, q_norm, k_norm, q_out, k_cache,  \
                 v_cache, positions, inv_freq, block_table, T, S, Hq, Hkv,  \
                 Smax, bt_stride, n_split, inv_bf16, eps, one_block, stream)
  if (D == 128) {
    if (n_split > 0) GO(128, 1);
    else GO(128, 0);
  } else {
    if (n_split > 0) GO(64, 1);
    else GO(64, 0);
  }
#undef GO
}

}  // extern "C"
