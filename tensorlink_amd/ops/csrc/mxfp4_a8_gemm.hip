// MXFP4 x MXFP8 GEMM on the scaled MFMA (gfx950), and the activation
// quantizer that feeds it:
//
//   out[M,N] bf16 = dequant8(xq, xs) @ dequant4(packed, exponents)^T (+bias)
//
//   xq        [M, K]    uint8  e4m3 codes           (mx_quant_act below)
//   xs        [M, K/32] uint8  e8m0, biased by 127  (one per 32-k group)
//   packed    [N, K/2]  uint8  e2m1, element 2i in the low nibble
//   exponents [N, K/32] int8   unbiased power of two per 32-k group
//
// Both operands go from memory to the matrix unit as they are stored: one
// v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz 0 = e4m3 A, blgp 4 = e2m1 B) per
// 16x16 tile and 128-k step. The two formats sit differently in the lanes
// (measured with hand-built operands, pinned by the scaled one-hot tests):
// lane l = (col = l & 15, quad = l >> 4) supplies
//   A (e4m3, 8 VGPRs): row `col`, k = k0 + 16*quad + (0..15) in VGPRs 0-3
//                      and k = k0 + 64 + 16*quad + (0..15) in VGPRs 4-7: the
//                      128 k run as two 64-k halves of 16 k per lane group
//   B (e2m1, 4 VGPRs): column `col`, k = k0 + 32*quad + (0..31), 16
//                      consecutive bytes, low nibble = even element
// and, in byte 0 of one VGPR each (op_sel 0), the e8m0 scale of 32-group
// `quad` of the step (k0 + 32*quad .. +31) of its row / column: the
// quantizer's byte for A, exponent + 127 for B. For B that is the lane's
// own data; an A group's elements sit in lane groups 2g % 4 and 2g % 4 + 1
// (half g / 2) while its scale comes from lane group g. The C fragment is
// the family's: lane holds C[quad*4 + r][col].
//
// Work split: a block owns a BM x BN output tile over the whole of K (no
// split-K), waves as WM x WN, each MT x NT 16x16 tiles. Two instantiations:
//   256 x 256, 8 waves 2(M) x 4(N), 8 x 4 tiles, 32 accumulators per lane
//   128 x 128, 4 waves 2(M) x 2(N), 4 x 4 tiles, 16 accumulators per lane
// the small one for shapes whose 256-tiles would not fill the chip. The
// choice is pure in (M, N) and no row's bits depend on it: an accumulator
// sees one MFMA per 128-k step, steps ascending from 0, in either tile.
//
// Data movement: per step a stage of LDS takes, all by global_load_lds,
//   A codes  [BM][128 B]  8-slot XOR image of gemm_family.hpp (stage_8x64 /
//                         lds_frag: a 128-B row of e4m3 is a 64-bf16 row)
//   W codes  [BN][64 B]   4 slots of 16 B, physical slot p of row r holds
//                         logical slot p ^ wswz(r)
//   A scales [BM] dwords, W exponents [BN] dwords: the row's four group
//                         bytes of this step, width-4 glds, lane = row
// Stages are double-buffered: a wave issues LOADS glds per stage, waits for
// its own stage-t loads with vmcnt(LOADS) while stage t+1 is in flight, and
// raw barriers align the block, as sq256_k_loop does. Rows past M and
// columns past N are clamped duplicates that the epilogue leaves out.
//
// Bias is added in fp32 before the one rounding to bf16.

#include "gemm_family.hpp"

// no packed fp32 arithmetic in this file's device code (bias add, quantizer
// scaling): the feature is switched off per function, the host pass does
// not know it
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x8 = __attribute__((ext_vector_type(8))) int;

// global_load_lds, 4 bytes per lane: lane l lands at lds_dst + l*4
DEVINLINE void glds4(const void* src, void* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)lds_dst, 4, 0, 0);
}

// W image swizzle: 16 consecutive rows reading one logical slot spread over
// all 16-B columns of both a 128-B and a 256-B bank window
DEVINLINE int wswz(int row) { return ((row >> 1) ^ (row >> 3)) & 3; }

template <int WM, int WN, int MT, int NT>
struct A8Tile {
  static constexpr int NW = WM * WN;
  static constexpr int BLOCK = NW * 64;
  static constexpr int BM = WM * MT * 16;
  static constexpr int BN = WN * NT * 16;
  static constexpr int A_BYTES = BM * 128;
  static constexpr int W_OFF = A_BYTES;
  static constexpr int SA_OFF = W_OFF + BN * 64;
  static constexpr int SW_OFF = SA_OFF + BM * 4;
  static constexpr int STAGE = SW_OFF + BN * 4;
  static constexpr int A_PER_WAVE = BM / 8 / NW;     // 8-row pieces
  static constexpr int W_PER_WAVE = BN / 16 / NW;    // 16-row pieces
  static constexpr int SA_WAVES = BM / 64;           // one glds4 = 64 rows
  static constexpr int LOADS = A_PER_WAVE + W_PER_WAVE + 1;
  static_assert(SA_WAVES + BN / 64 == NW, "one scale load per wave");
  static_assert(A_PER_WAVE * 8 * NW == BM && W_PER_WAVE * 16 * NW == BN, "");
  static_assert(2 * STAGE <= 160 * 1024, "LDS");
};

template <int WM, int WN, int MT, int NT, int HAS_BIAS>
__global__ __launch_bounds__(WM * WN * 64) void mxfp4_a8_gemm_kernel(
    const uint8_t* __restrict__ xq,      // [M, K]
    const uint8_t* __restrict__ xs,      // [M, K/32]
    const uint8_t* __restrict__ packed,  // [N, K/2]
    const int8_t* __restrict__ exps,     // [N, K/32]
    const bf16* __restrict__ bias,       // [N] or null
    bf16* __restrict__ out,              // [M, N]
    int M, int N, int K) {
  using T = A8Tile<WM, WN, MT, NT>;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int quad = lane >> 4;
  const int wm = wave / WN;
  const int wn = wave % WN;
  const int m_base = blockIdx.y * T::BM;
  const int n_base = blockIdx.x * T::BN;

  // ONE shared object: two stages
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * T::STAGE];

  f32x4 acc[MT * NT];
#pragma unroll
  for (int i = 0; i < MT * NT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto stage = [&](int bufi, int k0) {
    unsigned char* s = smem + bufi * T::STAGE;
#pragma unroll
    for (int g = 0; g < T::A_PER_WAVE; ++g) {
      const int piece = wave * T::A_PER_WAVE + g;
      const int xr = min(m_base + piece * 8 + (lane >> 3), M - 1);
      // the e4m3 row as 64-"bf16" chunks: k0/2 of K/2 two-byte elements
      stage_8x64(reinterpret_cast<const bf16*>(xq + (int64_t)xr * K), lane,
                 k0 >> 1, K >> 1,
                 reinterpret_cast<bf16*>(s + piece * 8 * 128));
    }
#pragma unroll
    for (int g = 0; g < T::W_PER_WAVE; ++g) {
      const int piece = wave * T::W_PER_WAVE + g;
      const int row = piece * 16 + (lane >> 2);
      const int gr = min(n_base + row, N - 1);
      const int slot = (lane & 3) ^ wswz(row);
      glds16(packed + (int64_t)gr * (K >> 1) + (k0 >> 1) + slot * 16,
             s + T::W_OFF + piece * 1024);
    }
    if (wave < T::SA_WAVES) {
      const int xr = min(m_base + wave * 64 + lane, M - 1);
      glds4(xs + (int64_t)xr * (K >> 5) + (k0 >> 5),
            s + T::SA_OFF + wave * 256);
    } else {
      const int w2 = wave - T::SA_WAVES;
      const int gr = min(n_base + w2 * 64 + lane, N - 1);
      glds4(exps + (int64_t)gr * (K >> 5) + (k0 >> 5),
            s + T::SW_OFF + w2 * 256);
    }
  };

  stage(0, 0);
  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += 128) {
    if (k0 + 128 < K) {
      stage(buf ^ 1, k0 + 128);               // in flight under compute
      waitcnt_vm<T::LOADS>();                 // stage t landed; t+1 out
    } else {
      waitcnt_vm<0>();                        // last stage: drain
    }
    __builtin_amdgcn_s_barrier();
    const unsigned char* s = smem + buf * T::STAGE;

    i32x8 bfrag[NT];
    int sb[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int row = (wn * NT + nt) * 16 + col;
      const i32x4 b = *reinterpret_cast<const i32x4*>(
          s + T::W_OFF + row * 64 + ((quad ^ wswz(row)) * 16));
      bfrag[nt] = (i32x8){b[0], b[1], b[2], b[3], 0, 0, 0, 0};
      const uint32_t e =
          *reinterpret_cast<const uint32_t*>(s + T::SW_OFF + row * 4);
      sb[nt] = (int)(((e >> (8 * quad)) + 127u) & 0xFFu);   // e + 127
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int row = (wm * MT + mt) * 16 + col;
      union {
        bf16x8_t h[2];
        i32x8 v;
      } a;
      a.h[0] = lds_frag(reinterpret_cast<const bf16*>(s), row, quad);
      a.h[1] = lds_frag(reinterpret_cast<const bf16*>(s), row, 4 + quad);
      const uint32_t e =
          *reinterpret_cast<const uint32_t*>(s + T::SA_OFF + row * 4);
      const int sa = (int)((e >> (8 * quad)) & 0xFFu);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[mt * NT + nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            a.v, bfrag[nt], acc[mt * NT + nt], 0 /* e4m3 */, 4 /* e2m1 */,
            0, sa, 0, sb[nt]);
    }
    // all waves done reading buf before the next iteration's glds overwrite
    // it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    buf ^= 1;
  }

#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int oc = n_base + (wn * NT + nt) * 16 + col;
    if (oc < N) {                             // N % 16 == 0: whole tiles
      const float b = HAS_BIAS ? bf2f(bias[oc]) : 0.f;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        f32x4 c = acc[mt * NT + nt];
#pragma unroll
        for (int r = 0; r < 4; ++r) c[r] += b;
        store_cfrag_bf16(c, out, m_base + (wm * MT + mt) * 16, M, N, oc,
                         quad);
      }
    }
  }
}

template <int WM, int WN, int MT, int NT>
void a8_launch(const void* xq, const void* xs, const void* packed,
               const void* exps, const void* bias, void* out, int M, int N,
               int K, hipStream_t stream) {
  using T = A8Tile<WM, WN, MT, NT>;
  launch_variant(mxfp4_a8_gemm_kernel<WM, WN, MT, NT, 0>,
                 mxfp4_a8_gemm_kernel<WM, WN, MT, NT, 1>,
                 mxfp4_a8_gemm_kernel<WM, WN, MT, NT, 0>, 1, bias,
                 dim3(cdiv(N, T::BN), cdiv(M, T::BM)), dim3(T::BLOCK),
                 stream, xq, xs, packed, exps, bias, out, M, N, K);
}

// ---------------------------------------------------------------------------
// Activation quantizer: bf16 [M, K] -> e4m3 codes + one e8m0 byte per
// 32-group, the bytes of ops.reference.quantize_mxfp8. A lane takes 16
// elements (two 16-B loads), two lanes a group; the group's amax meets by one
// xor shuffle, four groups' scale bytes meet in every 8th lane, which stores
// them as one dword. One pass, 16-B code stores.
// ---------------------------------------------------------------------------

// |y| <= 448 as f32 bits (sign cleared) -> e4m3 code, round to nearest even
DEVINLINE uint32_t e4m3_from_abs_bits(uint32_t u) {
  if (u < (121u << 23)) {
    // below 2^-6, the smallest normal: adding 2^14 leaves the multiple of
    // 2^-9 in the low mantissa bits, rounded by the add itself
    const uint32_t magic = 141u << 23;
    return __float_as_uint(__uint_as_float(u) + __uint_as_float(magic)) -
           magic;
  }
  const uint32_t odd = (u >> 20) & 1u;
  u += ((uint32_t)(7 - 127) << 23) + 0x7FFFFu + odd;
  return u >> 20;
}

__global__ __launch_bounds__(256) void mx_quant_act_kernel(
    const uint4* __restrict__ x,         // [M*K/8] of 8 bf16
    uint4* __restrict__ codes,           // [M*K/16]
    uint32_t* __restrict__ scales,       // [M*K/128]
    int64_t n_lanes) {                   // M*K/16, a multiple of 8
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = t < n_lanes;
  const int64_t i = live ? t : n_lanes - 1;
  const uint4 v0 = x[2 * i], v1 = x[2 * i + 1];
  const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};

  // amax over the bf16 magnitudes, as bit patterns (finite inputs)
  uint32_t amax = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    amax = max(amax, w[j] & 0x7FFFu);
    amax = max(amax, (w[j] >> 16) & 0x7FFFu);
  }
  amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, WAVE_SIZE));
  const int s = min(max((int)(amax >> 7) - 8, 0), 254);

  uint32_t c[4];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    uint32_t pair = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t bits = h ? (w[j] & 0xFFFF0000u) : (w[j] << 16);
      // x / 2^(s-127), exact; then the saturating clamp
      const float y = fminf(
          ldexpf(__uint_as_float(bits & 0x7FFFFFFFu), 127 - s), 448.f);
      const uint32_t code =
          e4m3_from_abs_bits(__float_as_uint(y)) | ((bits >> 24) & 0x80u);
      pair |= code << (8 * h);
    }
    if (j & 1)
      c[j >> 1] |= pair << 16;
    else
      c[j >> 1] = pair;
  }

  uint32_t sv = (uint32_t)s;
  sv |= (uint32_t)__shfl_down((int)sv, 2, WAVE_SIZE) << 8;
  sv |= (uint32_t)__shfl_down((int)sv, 4, WAVE_SIZE) << 16;
  if (live) {
    codes[i] = make_uint4(c[0], c[1], c[2], c[3]);
    if ((threadIdx.x & 7) == 0) scales[i >> 3] = sv;
  }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" {

// 256-tiles when they give every CU of the chip a block, else 128-tiles.
// Pure in the shape; no row's bits depend on it.
int tl_mxfp4_a8_tile(int M, int N) {
  return (int64_t)cdiv(M, 256) * cdiv(N, 256) >= 256 ? 256 : 128;
}

// Requires N % 64 == 0, K % 128 == 0, M >= 1 (checked by the binding).
// tile: 0 = tl_mxfp4_a8_tile's choice, 128 / 256 force one (tests).
void tl_mxfp4_a8_gemm(const void* xq, const void* xs, const void* packed,
                      const void* exps, const void* bias, void* out, int M,
                      int N, int K, int tile, hipStream_t stream) {
  if (tile == 0) tile = tl_mxfp4_a8_tile(M, N);
  if (tile == 256)
    a8_launch<2, 4, 8, 4>(xq, xs, packed, exps, bias, out, M, N, K, stream);
  else
    a8_launch<2, 2, 4, 4>(xq, xs, packed, exps, bias, out, M, N, K, stream);
}

// x bf16 [M*K] with K % 128 == 0 -> codes [M*K] bytes, scales [M*K/32] bytes
void tl_mx_quant_act(const void* x, void* codes, void* scales,
                     int64_t n_elems, hipStream_t stream) {
  const int64_t n_lanes = n_elems / 16;
  hipLaunchKernelGGL(mx_quant_act_kernel, dim3((unsigned)cdiv64(n_lanes, 256)),
                     dim3(256), 0, stream,
                     static_cast<const uint4*>(x),
                     static_cast<uint4*>(codes),
                     static_cast<uint32_t*>(scales), n_lanes);
}

}  // extern "C"
