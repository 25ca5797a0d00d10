// Weight-only MXFP4 GEMM (gfx950): out[M,N] = x[M,K] @ W[N,K]^T (+bias),
// x bf16, W in the packed form quantize_mxfp4 emits:
//   packed    [N, K/2]  uint8  element 2i low nibble, 2i+1 high nibble;
//                              code bit 3 sign, bits 0-2 index
//                              {0,.5,1,1.5,2,3,4,6}
//   exponents [N, K/32] int8   unbiased power of two per 32-k group
//
// Streaming-GEMM family member (skinny_gemm.hip / moe_gemm.hip lineage).
// Grid (N/64, SPLITK); block = 4 waves; wave w owns 16 columns. Rows go in
// chunks of MT*16 (MT picked from M; M > 64 loops 64-row chunks, W panels
// re-read from L2). Per 128-k step:
//   * the x slab [MT*16][128] is staged by global_load_lds into a
//     double-buffered, lane-linear LDS image with the bank swizzle on the
//     SOURCE address (physical 16-B slot p of row r holds logical slot
//     p ^ (r & 15); the fragment read applies the same XOR);
//   * lane (col, quad) loads 16 B of its column's packed row = one whole
//     32-k group (group index = quad) plus that group's exponent byte,
//     and spends the four dwords on four mfma_f32_16x16x32_bf16: MFMA j
//     sums k = k0 + 32*quad + 8*j + (0..7). The A fragment is read from
//     LDS at the same k. This k order is fixed by the kernel alone, so a
//     row's result does not depend on M, MT or the chunk it falls in.
//
// Dequant is exact: a 256-entry LDS table maps a packed byte to its two
// e2m1 values as f32; one v_pk_mul_f32 by the group's 2^e (built from the
// exponent bits, e in [-120, 120] keeps every product a normal f32) and a
// truncation to the upper 16 bits give bf16. An e2m1 value times a power
// of two has <= 2 significant bits, so nothing is rounded; +-0 stays 0
// through the multiply without a special case.
//
// Split-K: fp32 partial slabs [SPLITK, M, N] and an s-ordered reduce
// kernel; the split count comes from the host and depends on (N, K) only.

#include "mxfp4_common.hpp"

namespace {

// decode, table build and split slice: mxfp4_common.hpp, shared with the
// grouped expert kernel (mxfp4_moe_gemm.hip)
constexpr int BLOCK = MX_BLOCK;
constexpr int KSTEP = MX_KSTEP;            // k per main-loop step
constexpr int ROW_BYTES = MX_ROW_BYTES;    // one slab row (bf16)
constexpr int LUT_BYTES = MX_LUT_BYTES;    // byte -> float2

using f32x2 = mx_f32x2;

template <int MT, int HAS_BIAS, int SPLIT>
__global__ __launch_bounds__(BLOCK, 2) void mxfp4_gemm_kernel(
    const bf16* __restrict__ x,          // [M, K]
    const uint8_t* __restrict__ packed,  // [N, K/2]
    const int8_t* __restrict__ exps,     // [N, K/32]
    const bf16* __restrict__ bias,       // [N] or null
    bf16* __restrict__ out,              // [M, N]
    float* __restrict__ partial,         // [SPLITK, M, N] when SPLIT
    int M, int N, int K, int n_split) {
  constexpr int ROWS = MT * 16;
  constexpr int SLAB_BYTES = ROWS * ROW_BYTES;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int quad = lane >> 4;
  const int oc = blockIdx.x * 64 + wave * 16 + col;   // output column

  const int split = SPLIT ? blockIdx.y : 0;
  const int k_per = SPLIT ? mxfp4_k_per(K, n_split) : K;
  const int k_begin = split * k_per;
  const int k_end = min(K, k_begin + k_per);

  // ONE shared object: [2 buffers][ROWS][128 k] x slab, then the LUT
  __shared__ __attribute__((aligned(16))) unsigned char
      smem[2 * SLAB_BYTES + LUT_BYTES];
  unsigned char* const lut = smem + 2 * SLAB_BYTES;
  mxfp4_build_lut(lut);

  // this lane's packed row (16 B per 128-k step at dword4 index quad) and
  // exponent row (1 B per step at byte index quad)
  const uint4* wrow = reinterpret_cast<const uint4*>(
                          packed + (int64_t)oc * (K / 2)) + quad;
  const int8_t* erow = exps + (int64_t)oc * (K / 32) + quad;

  const int l16 = lane >> 4, p16 = lane & 15;

  for (int mb = 0; mb < M; mb += ROWS) {
    const int mrows = min(ROWS, M - mb);
    f32x4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // x glds: ROWS/4 chunks of 4 rows (1 KB each) -> MT per wave
#define MX_GLDS_TILE(bufi, k0)                                              \
    _Pragma("unroll") for (int g = 0; g < MT; ++g) {                        \
      const int chunk = wave * MT + g;                                      \
      const int row = chunk * 4 + l16;                                      \
      const int xr = mb + min(row, mrows - 1);                              \
      const int kc = (k0) + (p16 ^ (row & 15)) * 8;                         \
      glds16(x + (int64_t)xr * K + kc,                                      \
             smem + (bufi) * SLAB_BYTES + chunk * 4 * ROW_BYTES);           \
    }

    if (k_begin < k_end) MX_GLDS_TILE(0, k_begin);
    // W for the first step; an empty split clamps to a valid address
    const int s0 = min(k_begin, K - KSTEP) / KSTEP;
    uint4 wcur = wrow[s0 * 4];
    int ecur = erow[s0 * 4];
    int buf = 0;
    for (int k0 = k_begin; k0 < k_end; k0 += KSTEP) {
      __syncthreads();                      // drains this tile's glds
      if (k0 + KSTEP < k_end) MX_GLDS_TILE(buf ^ 1, k0 + KSTEP);
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
#undef MX_GLDS_TILE

    // epilogue: lane holds C[row = quad*4 + r][col] per m-tile
    const float b = HAS_BIAS ? bf2f(bias[oc]) : 0.f;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lrow = m * 16 + quad * 4 + r;
        if (lrow < mrows) {
          const int64_t orow = mb + lrow;
          if (SPLIT)
            partial[((int64_t)split * M + orow) * N + oc] = acc[m][r];
          else
            out[orow * N + oc] = f2bf(acc[m][r] + b);
        }
      }
    }
    // next m-chunk restarts the glds pipeline; resync before it
    // overwrites buffer 0
    __syncthreads();
  }
}

template <int MT>
void mxfp4_launch_mt(const void* x, const void* packed, const void* exps,
                     const void* bias, void* out, void* partial, int M,
                     int N, int K, int n_split, hipStream_t stream) {
  launch_variant(mxfp4_gemm_kernel<MT, 0, 1>, mxfp4_gemm_kernel<MT, 1, 0>,
                 mxfp4_gemm_kernel<MT, 0, 0>, n_split, bias,
                 dim3(N / 64, n_split), dim3(BLOCK), stream, x, packed,
                 exps, bias, out, partial, M, N, K, n_split);
}

}  // namespace

extern "C" {

// partial: scratch [n_split * M * N] floats (only used when n_split > 1).
// Requires N % 64 == 0, K % 128 == 0, M >= 1 (checked by the binding).
void tl_mxfp4_gemm(const void* x, const void* packed, const void* exps,
                   const void* bias, void* out, void* partial, int M, int N,
                   int K, int n_split, hipStream_t stream) {
  if (M <= 16)
    mxfp4_launch_mt<1>(x, packed, exps, bias, out, partial, M, N, K, n_split,
                       stream);
  else if (M <= 32)
    mxfp4_launch_mt<2>(x, packed, exps, bias, out, partial, M, N, K, n_split,
                       stream);
  else
    mxfp4_launch_mt<4>(x, packed, exps, bias, out, partial, M, N, K, n_split,
                       stream);
  if (n_split > 1)
    launch_splitk_reduce(partial, bias, out, M, N, n_split, stream);
}

}  // extern "C"
