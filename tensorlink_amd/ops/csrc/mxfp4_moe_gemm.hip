// Grouped MXFP4 expert GEMM for MoE serving (gfx950):
//   out[p, :] = x[tok_idx[p], :] @ dequant(packed_e, exps_e)^T
// for every pair row p of segment e = [seg_off[e], seg_off[e+1]). x bf16;
// each expert's weights exactly as quantize_mxfp4 emits them (packed
// [N, K/2] uint8, exponents [N, K/32] int8), addressed through two device
// pointer tables: no stacked copy, no dequantized copy. No bias.
//
// The marriage of two family members, nothing new:
//   * moe_gemm.hip gives the outside: grid (N/64, E), segment bounds read
//     on the device, an empty segment returning before any barrier,
//     indirect x rows through tok_idx staged by global_load_lds, rows past
//     the segment end clamped to its last row, a row-chunk loop (MT*16
//     rows, 64 at MT=4) with the W panel re-read from L2.
//   * mxfp4_gemm.hip gives the inside: the 128-k step, the lane-linear
//     double-buffered [MT*16][128] slab with the XOR swizzle on the SOURCE
//     address, lane (col, quad) loading one whole 32-k group (16 B) plus
//     its exponent byte and spending it on four mfma_f32_16x16x32_bf16,
//     the byte -> float2 LDS table with one v_pk_mul_f32 by 2^e and a
//     truncation to bf16 (exact), and a next-step W prefetch that never
//     leaves the row (the last step re-reads itself).
//
// The k order of a row is fixed by the kernel alone, so a pair's row is
// bitwise the same whatever else is in the call (other segments, its
// place in its segment, MT, P), and, wherever the split counts agree,
// bitwise equal to mxfp4_gemm on the gathered rows.
//
// Split-K: third grid dimension, fp32 slabs [S, P, N], the shared
// s-ordered reduce. The split count comes from the host and depends on
// (N, K, E) only. An empty split writes zeros; the slab is never
// pre-zeroed. MT comes from P alone (segment sizes live on the device).

#include "mxfp4_common.hpp"

namespace {

constexpr int BLOCK = MX_BLOCK;
constexpr int KSTEP = MX_KSTEP;
constexpr int ROW_BYTES = MX_ROW_BYTES;
constexpr int LUT_BYTES = MX_LUT_BYTES;

using f32x2 = mx_f32x2;

template <int MT, int SPLIT>
__global__ __launch_bounds__(BLOCK, 2) void mxfp4_moe_gemm_kernel(
    const bf16* __restrict__ x,           // [T, K] (or [P, K] pair rows)
    const int* __restrict__ tok_idx,      // [P] row of x per pair, or null
    const int* __restrict__ seg_off,      // [E+1] pair segments by expert
    const uint64_t* __restrict__ p_ptrs,  // [E] -> packed [N, K/2]
    const uint64_t* __restrict__ e_ptrs,  // [E] -> exponents [N, K/32]
    bf16* __restrict__ out,               // [P, N]
    float* __restrict__ partial,          // [SPLITK, P, N] when SPLIT
    int T, int P, int N, int K, int n_split) {
  constexpr int ROWS = MT * 16;
  constexpr int SLAB_BYTES = ROWS * ROW_BYTES;

  // segment bounds, held inside [0, P]: uniform per block, and an empty
  // segment leaves before any barrier
  const int e = blockIdx.y;
  const int m0 = max(seg_off[e], 0);
  const int m_tot = min(seg_off[e + 1], P) - m0;
  if (m_tot <= 0) return;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int quad = lane >> 4;
  const int oc = blockIdx.x * 64 + wave * 16 + col;   // output column

  const int split = SPLIT ? blockIdx.z : 0;
  const int k_per = SPLIT ? mxfp4_k_per(K, n_split) : K;
  const int k_begin = split * k_per;
  const int k_end = min(K, k_begin + k_per);

  // ONE shared object: [2 buffers][ROWS][128 k] x slab, then the LUT
  __shared__ __attribute__((aligned(16))) unsigned char
      smem[2 * SLAB_BYTES + LUT_BYTES];
  unsigned char* const lut = smem + 2 * SLAB_BYTES;
  mxfp4_build_lut(lut);

  // this lane's packed row (16 B per 128-k step at dword4 index quad) and
  // exponent row (1 B per step at byte index quad) of expert e
  const uint4* wrow = reinterpret_cast<const uint4*>(
                          reinterpret_cast<const uint8_t*>(p_ptrs[e]) +
                          (int64_t)oc * (K / 2)) + quad;
  const int8_t* erow = reinterpret_cast<const int8_t*>(e_ptrs[e]) +
                       (int64_t)oc * (K / 32) + quad;

  const int l16 = lane >> 4, p16 = lane & 15;

  // chunks of ROWS pair rows of this expert's segment (W panels re-read
  // per chunk stay L2-resident: same block, back to back)
  for (int mb = 0; mb < m_tot; mb += ROWS) {
    const int mrows = min(ROWS, m_tot - mb);
    f32x4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // x glds: ROWS/4 chunks of 4 rows (1 KB each) -> MT per wave. The
    // source row is indirect and fixed for the whole k loop: rows past the
    // segment end repeat its last row, and the row index is held inside x
    const bf16* xsrc[MT];
#pragma unroll
    for (int g = 0; g < MT; ++g) {
      const int row = (wave * MT + g) * 4 + l16;
      const int p = m0 + mb + min(row, mrows - 1);
      const int xr = min(max(tok_idx ? tok_idx[p] : p, 0), T - 1);
      xsrc[g] = x + (int64_t)xr * K + (p16 ^ (row & 15)) * 8;
    }

#define MXM_GLDS_TILE(bufi, k0)                                             \
    _Pragma("unroll") for (int g = 0; g < MT; ++g) {                        \
      const int chunk = wave * MT + g;                                      \
      glds16(xsrc[g] + (k0),                                                \
             smem + (bufi) * SLAB_BYTES + chunk * 4 * ROW_BYTES);           \
    }

    if (k_begin < k_end) MXM_GLDS_TILE(0, k_begin);
    // W for the first step; an empty split clamps to a valid address
    const int s0 = min(k_begin, K - KSTEP) / KSTEP;
    uint4 wcur = wrow[s0 * 4];
    int ecur = erow[s0 * 4];
    int buf = 0;
    for (int k0 = k_begin; k0 < k_end; k0 += KSTEP) {
      __syncthreads();                      // drains this tile's glds
      if (k0 + KSTEP < k_end) MXM_GLDS_TILE(buf ^ 1, k0 + KSTEP);
      // next step's W, unconditionally (the last step re-reads itself)
      const int sn = min(k0 + KSTEP, k_end - KSTEP) / KSTEP;
      const uint4 wnext = wrow[sn * 4];
      const int enext = erow[sn * 4];

      const float scale = __int_as_float((ecur + 127) << 23);   // 2^e
      const uint32_t wd[4] = {wcur.x, wcur.y, wcur.z, wcur.w};
      const unsigned char* slab = smem + buf * SLAB_BYTES;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        union {
          uint32_t u[4];
          bf16x8_t v;
        } bfrag;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const uint32_t byte = (wd[j] >> (8 * p)) & 0xFFu;
          f32x2 v = *reinterpret_cast<const f32x2*>(lut + byte * 8);
          v = v * scale;
          // exact bf16: the upper 16 bits of each f32
          bfrag.u[p] = (__float_as_uint(v[1]) & 0xFFFF0000u) |
                       (__float_as_uint(v[0]) >> 16);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int row = m * 16 + col;
          const int slot = (quad * 4 + j) ^ col;     // row & 15 == col
          bf16x8_t afrag = *reinterpret_cast<const bf16x8_t*>(
              slab + row * ROW_BYTES + slot * 16);
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag, bfrag.v, acc[m], 0, 0, 0);
        }
      }
      wcur = wnext;
      ecur = enext;
      buf ^= 1;
    }
#undef MXM_GLDS_TILE

    // epilogue: lane holds C[row = quad*4 + r][col] per m-tile
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lrow = m * 16 + quad * 4 + r;
        if (lrow < mrows) {
          const int64_t orow = m0 + mb + lrow;
          if (SPLIT)
            partial[((int64_t)split * P + orow) * N + oc] = acc[m][r];
          else
            out[orow * N + oc] = f2bf(acc[m][r]);
        }
      }
    }
    // next row chunk restarts the glds pipeline; resync before it
    // overwrites buffer 0
    __syncthreads();
  }
}

template <int MT>
void mxfp4_moe_launch_mt(const void* x, const void* tok_idx,
                         const void* seg_off, const void* p_ptrs,
                         const void* e_ptrs, void* out, void* partial, int T,
                         int P, int E, int N, int K, int n_split,
                         hipStream_t stream) {
  // no bias: the plain kernel stands in for the bias variant
  launch_variant(mxfp4_moe_gemm_kernel<MT, 1>, mxfp4_moe_gemm_kernel<MT, 0>,
                 mxfp4_moe_gemm_kernel<MT, 0>, n_split, nullptr,
                 dim3(N / 64, E, n_split), dim3(BLOCK), stream, x, tok_idx,
                 seg_off, p_ptrs, e_ptrs, out, partial, T, P, N, K, n_split);
}

}  // namespace

extern "C" {

// partial: scratch [n_split * P * N] floats (only used when n_split > 1).
// Requires N % 64 == 0, K % 128 == 0, T >= 1, P >= 1 (checked by the
// binding). MT from P alone: P <= 16 -> 1, P <= 32 -> 2, else 4.
void tl_mxfp4_moe_gemm(const void* x, const void* tok_idx,
                       const void* seg_off, const void* p_ptrs,
                       const void* e_ptrs, void* out, void* partial, int T,
                       int P, int E, int N, int K, int n_split,
                       hipStream_t stream) {
  if (P <= 16)
    mxfp4_moe_launch_mt<1>(x, tok_idx, seg_off, p_ptrs, e_ptrs, out, partial,
                           T, P, E, N, K, n_split, stream);
  else if (P <= 32)
    mxfp4_moe_launch_mt<2>(x, tok_idx, seg_off, p_ptrs, e_ptrs, out, partial,
                           T, P, E, N, K, n_split, stream);
  else
    mxfp4_moe_launch_mt<4>(x, tok_idx, seg_off, p_ptrs, e_ptrs, out, partial,
                           T, P, E, N, K, n_split, stream);
  if (n_split > 1)
    launch_splitk_reduce(partial, nullptr, out, P, N, n_split, stream);
}

}  // extern "C"
