// Fused RoPE + KV-cache append for gfx950.
//
// One kernel consumes the fused-QKV GEMM output directly (strided rows:
// [T, q_size + 2*kv_size]): rotates q into a contiguous [T, Hq, D] buffer,
// rotates k and writes it into the KV cache at its position, and copies v
// into the cache — replacing a rope kernel + two cache scatters + three
// .contiguous() splits per layer per step. (The reference instead
// re-serializes the whole DynamicCache over TCP per step —
// tensorlink/ml/utils.py:210-221.)
//
// qkv [T, row_stride] bf16 (or the GEMM's fp32 split-K partials, see PART
// below) with q at offset 0, k at q_size, v at q_size+kv_size; caches
// [B, Hkv, Smax, D] with T = B*S tokens; positions [T] int32 gives both
// the RoPE angle and the cache slot.

#include "common.hpp"

namespace {

constexpr int BLOCK = 256;

// PAGED != 0: caches are page pools [n_pages, Hkv, 128, D] addressed via
// block_table [B, bt_stride].
// PART != 0: qkv is the fused-QKV GEMM's fp32 split-K partials
// [n_split, T, row_stride] (+ optional bf16 bias) instead of its bf16
// output; an element is bf16(sum_s partial[s] + bias), summed from 0 in s
// order — the value the GEMM's own reduce kernel writes — so everything
// downstream is bitwise what the bf16 input mode computes. The block first
// reduces its row into LDS (row_stride bf16 of dynamic shared memory,
// 16-byte loads, sum_partials8), then rotates out of LDS.
// inv_freq is fp32, or bf16 when inv_bf16 (widened in-register, exact).
template <int PAGED, int PART>
__global__ __launch_bounds__(BLOCK) void rope_append_kernel(
    const void* __restrict__ qkv, const bf16* __restrict__ bias,
    bf16* __restrict__ q_out, bf16* __restrict__ k_cache,
    bf16* __restrict__ v_cache, const int* __restrict__ positions,
    const void* __restrict__ inv_freq, const int* __restrict__ block_table,
    int row_stride, int S, int Hq, int Hkv, int D, int Smax, int bt_stride,
    int n_split, int64_t split_stride, int inv_bf16) {
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
  const int D2 = D / 2;
  const float fpos = (float)pos;
  extern __shared__ __align__(16) unsigned char smem[];
  const bf16* row;
  if constexpr (PART) {
    constexpr int UN = 3;   // 8-column groups per thread per sweep
    bf16* srow = reinterpret_cast<bf16*>(smem);
    const float* prow = (const float*)qkv + token * row_stride;
    const int n8 = row_stride / 8;
    for (int g0 = 0; g0 < n8; g0 += BLOCK * UN) {
      const float* pp[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u)
        pp[u] = prow + min(g0 + u * BLOCK + (int)threadIdx.x, n8 - 1) * 8;
      float acc[UN][8];
      sum_partials8<UN, 4>(pp, split_stride, n_split, acc);
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int g = g0 + u * BLOCK + threadIdx.x;
        if (g < n8) {
          bf16x8 out;
          if (bias) {
            const bf16x8 vb = *reinterpret_cast<const bf16x8*>(bias + g * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j)
              out.v[j] = f2bf(acc[u][j] + bf2f(vb.v[j]));
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) out.v[j] = f2bf(acc[u][j]);
          }
          reinterpret_cast<bf16x8*>(srow)[g] = out;
        }
      }
    }
    __syncthreads();
    row = srow;
  } else {
    row = (const bf16*)qkv + token * row_stride;
  }
  const bf16* krow = row + Hq * D;
  const bf16* vrow = krow + Hkv * D;

  // rotate q (Hq heads) -> contiguous q_out; rotate k -> cache
  const int total = (Hq + Hkv) * D2;
  auto angle = [&](int d, float& s, float& c) {
    const float fr = inv_bf16 ? bf2f(((const bf16*)inv_freq)[d])
                              : ((const float*)inv_freq)[d];
    __sincosf(fpos * fr, &s, &c);
  };
  // when D2 divides BLOCK a thread keeps the same d in every iteration:
  // one sincos per thread instead of one per (head, d) pair
  const bool fixed_d = BLOCK % D2 == 0;
  float c0 = 0.f, s0 = 0.f;
  if (fixed_d) angle(threadIdx.x % D2, s0, c0);
  for (int idx = threadIdx.x; idx < total; idx += BLOCK) {
    const int h = idx / D2;
    const int d = idx - h * D2;
    float c = c0, s = s0;
    if (!fixed_d) angle(d, s, c);
    if (h < Hq) {
      const bf16* src = row + h * D;
      const float x1 = bf2f(src[d]);
      const float x2 = bf2f(src[d + D2]);
      bf16* dst = q_out + (token * Hq + h) * D;
      dst[d] = f2bf(x1 * c - x2 * s);
      dst[d + D2] = f2bf(x2 * c + x1 * s);
    } else {
      const int hk = h - Hq;
      const bf16* src = krow + hk * D;
      const float x1 = bf2f(src[d]);
      const float x2 = bf2f(src[d + D2]);
      bf16* kc = k_cache + (slot + hk * head_stride) * D;
      kc[d] = f2bf(x1 * c - x2 * s);
      kc[d + D2] = f2bf(x2 * c + x1 * s);
    }
  }
  // copy v into cache (no rotation), vectorized
  const int vtotal = Hkv * D / 8;
  for (int idx = threadIdx.x; idx < vtotal; idx += BLOCK) {
    const int h = idx / (D / 8);
    const int d8 = idx - h * (D / 8);
    const bf16x8 val =
        *reinterpret_cast<const bf16x8*>(vrow + h * D + d8 * 8);
    reinterpret_cast<bf16x8*>(
        v_cache + (slot + h * head_stride) * D)[d8] = val;
  }
}

template <int PART>
void launch(const void* qkv, const void* bias, void* q_out, void* k_cache,
            void* v_cache, const void* positions, const void* inv_freq,
            const void* block_table, int64_t T, int row_stride, int S,
            int Hq, int Hkv, int D, int Smax, int bt_stride, int n_split,
            int inv_bf16, hipStream_t stream) {
  dim3 grid((uint32_t)T), block(BLOCK);
  const int64_t split_stride = T * row_stride;
  const size_t lds = PART ? (size_t)row_stride * sizeof(bf16) : 0;
  if (block_table)
    hipLaunchKernelGGL((rope_append_kernel<1, PART>), grid, block, lds,
                       stream, qkv, (const bf16*)bias, (bf16*)q_out,
                       (bf16*)k_cache,
                       (bf16*)v_cache, (const int*)positions, inv_freq,
                       (const int*)block_table, row_stride, S, Hq, Hkv, D,
                       Smax, bt_stride, n_split, split_stride, inv_bf16);
  else
    hipLaunchKernelGGL((rope_append_kernel<0, PART>), grid, block, lds,
                       stream, qkv, (const bf16*)bias, (bf16*)q_out,
                       (bf16*)k_cache,
                       (bf16*)v_cache, (const int*)positions, inv_freq,
                       nullptr, row_stride, S, Hq, Hkv, D, Smax, bt_stride,
                       n_split, split_stride, inv_bf16);
}

}  // namespace

extern "C" {

// n_split == 0: qkv is bf16 [T, row_stride] and bias is ignored.
// n_split  > 0: qkv is fp32 partials [n_split, T, row_stride], bias bf16
// [row_stride] or null.
void tl_rope_append(const void* qkv, const void* bias, void* q_out,
                    void* k_cache, void* v_cache, const void* positions,
                    const void* inv_freq, const void* block_table,
                    int64_t T, int row_stride, int S, int Hq, int Hkv,
                    int D, int Smax, int bt_stride, int n_split,
                    int inv_bf16, hipStream_t stream) {
  if (n_split > 0)
    launch<1>(qkv, bias, q_out, k_cache, v_cache, positions, inv_freq,
              block_table, T, row_stride, S, Hq, Hkv, D, Smax, bt_stride,
              n_split, inv_bf16, stream);
  else
    launch<0>(qkv, nullptr, q_out, k_cache, v_cache, positions, inv_freq,
              block_table, T, row_stride, S, Hq, Hkv, D, Smax, bt_stride, 0,
              inv_bf16, stream);
}

}  // extern "C"
