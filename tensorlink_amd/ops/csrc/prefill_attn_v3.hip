// Causal GQA flash-attention forward (prefill) on gfx950 MFMA, v3.
//
// Same arithmetic per query row as prefill_attn.hip (v2), bit for bit:
// online softmax over 64-key tiles in ascending order with one tile-wide
// max, __expf, P rounded to bf16, mfma_f32_16x16x32_bf16 in the same K
// order, row sums per lane over the four sub-tiles then xor-shuffled. What
// changes is how the tiles reach the MFMAs:
//
//   * block = 256 threads (4 waves), BM = 128 query rows of one head; wave
//     w owns rows w*32..w*32+31 as TWO 16-row fragments, so every K
//     fragment and every transposed V fragment read from LDS feeds two
//     MFMAs (half the LDS bytes per FLOP of v2, half the K/V staging per
//     query row).
//   * K/V tiles are double-buffered in LDS: tile t+1 is fetched into
//     registers before tile t's compute and stored to the other buffer
//     after it; one __syncthreads per tile and no exposed global load.
//   * V fragments are fetched four at a time (one wait per 8 transposed
//     reads, not one per fragment).
//   * heavy (late) query tiles launch first; the mask compare runs only
//     on tiles that cross the diagonal or Skv.
//   * K and V carry batch / head / token strides (D contiguous), so the
//     [B,Hkv,Smax,D] cache is read in place.
//
// A wave runs exactly the key tiles v2 runs for its rows (those below
// q_off + the end of its 64-row half), so even the sign of a zero matches.
//
// LDS: 2 x (K 17,408 + V 16,640) + P 9,216 = 77,312 B -> 2 blocks per CU.

#include "common.hpp"

namespace {

constexpr int BLOCK = 256;   // 4 waves
constexpr int BM = 128;      // query rows per block (32 per wave)
constexpr int HALF = 64;     // v2's query tile: sets a wave's key range
constexpr int BN = 64;       // key cols per tile
constexpr int PPAD = 8;      // P row pad: stride 72 elems = 144 B
constexpr int PSTRIDE = 32 * 16 + 8;  // V panel stride (elems), padded

// Four consecutive V panels' B-fragments (see ds_read_tr16_frag in
// common.hpp) off one address register, one wait for all eight reads.
// Panels are PSTRIDE * 2 = 1040 bytes apart.
DEVINLINE void ds_read_tr16_frag4(unsigned addr_bytes, bf16x8_t (&f)[4]) {
  static_assert(PSTRIDE * 2 == 1040);
  unsigned long long r[8];
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8\n\t"
      "ds_read_b64_tr_b16 %1, %8 offset:128\n\t"
      "ds_read_b64_tr_b16 %2, %8 offset:1040\n\t"
      "ds_read_b64_tr_b16 %3, %8 offset:1168\n\t"
      "ds_read_b64_tr_b16 %4, %8 offset:2080\n\t"
      "ds_read_b64_tr_b16 %5, %8 offset:2208\n\t"
      "ds_read_b64_tr_b16 %6, %8 offset:3120\n\t"
      "ds_read_b64_tr_b16 %7, %8 offset:3248\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(r[4]),
        "=&v"(r[5]), "=&v"(r[6]), "=&v"(r[7])
      : "v"(addr_bytes)
      : "memory");
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    union {
      struct { unsigned long long a, b; } u;
      bf16x8_t v;
    } cvt;
    cvt.u.a = r[2 * i];
    cvt.u.b = r[2 * i + 1];
    f[i] = cvt.v;
  }
}

// One 16-row fragment's online-softmax step over a 64-key tile: v2's
// expressions in v2's order. s = raw QK^T accumulators in, P written to
// pw[16][BN + PPAD] as bf16. MASK = false only for tiles wholly below the
// diagonal and below Skv, where v2's select always takes the product.
template <bool MASK, bool PIN_FMA>
DEVINLINE void softmax_frag(f32x4 (&s)[4], float (&m_run)[4],
                            float (&l_run)[4], float (&alpha)[4], int kt0,
                            int qrow0, int Skv, int causal, float scale,
                            bf16 (*pw)[BN + PPAD], int col, int quad) {
  float row_max[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) row_max[r] = -1e30f;
#pragma unroll
  for (int ns = 0; ns < 4; ++ns) {
    const int kcol = kt0 + ns * 16 + col;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (MASK) {
        const int qrow = qrow0 + quad * 4 + r;
        const bool masked = (kcol >= Skv) || (causal && kcol > qrow);
        s[ns][r] = masked ? -1e30f : s[ns][r] * scale;
      } else {
        float sv = s[ns][r] * scale;
        // v2's product is rounded on its own (a select follows it); keep
        // this one from being contracted into the subtraction below
        asm("" : "+v"(sv));
        s[ns][r] = sv;
      }
      row_max[r] = fmaxf(row_max[r], s[ns][r]);
    }
  }
#pragma unroll
  for (int off = 1; off < 16; off <<= 1)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      row_max[r] = fmaxf(row_max[r], __shfl_xor(row_max[r], off, WAVE_SIZE));
  float psum[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float m_new = fmaxf(m_run[r], row_max[r]);
    alpha[r] = __expf(m_run[r] - m_new);
    m_run[r] = m_new;
    psum[r] = 0.f;
  }
#pragma unroll
  for (int ns = 0; ns < 4; ++ns)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = (s[ns][r] <= -1e29f)
                          ? 0.f : __expf(s[ns][r] - m_run[r]);
      pw[quad * 4 + r][ns * 16 + col] = f2bf(p);
      psum[r] += p;
    }
#pragma unroll
  for (int off = 1; off < 16; off <<= 1)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      psum[r] += __shfl_xor(psum[r], off, WAVE_SIZE);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    // the plain kernel's compile contracts this to one fma (as v2's does);
    // the carried variant's does so for some rows only, so there the fma
    // is spelled out. Spelling it out for both moves the plain kernel's
    // register allocation, which stays as it was measured.
    if constexpr (PIN_FMA)
      l_run[r] = __builtin_fmaf(l_run[r], alpha[r], psum[r]);
    else
      l_run[r] = l_run[r] * alpha[r] + psum[r];
  }
}

// Sq, Skv, q_off as in v2. k_s* / v_s* = batch, head and token strides in
// elements of the [B,Skv,Hkv,D] views (D contiguous).
//
// CARRY = 1 is the carried-state variant: the online-softmax state of a row
// (m_run, l_run and the unnormalised oacc, all f32) starts from the caller's
// buffers unless `first` and goes back to them unless `last`, so a sequence
// of calls over key chunks is one softmax over their concatenation.
//   o_state  [B,Sq,Hq,D]  unnormalised accumulator, indexed like out
//   ml_state [B,Hq,Sq,2]  (m, l) per row as one 8-byte pair
// The state is updated in place: a row's state is read in the prologue and
// written in the epilogue by the same lanes of the same workgroup, and no
// other workgroup touches that row, so there is no cross-workgroup hazard.
// Rows past Sq keep the init values and touch no address. The tile loop
// between prologue and epilogue is the same code for both variants; with
// chunk boundaries on multiples of BN and chunks in ascending order the
// carried calls run v3's tile steps in v3's order (bit-identical result).
// CARRY = 0 ignores the four trailing arguments.
template <int D, int CARRY>
__global__ __launch_bounds__(BLOCK)
__attribute__((amdgpu_waves_per_eu(2))) void prefill_attn_v3_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, bf16* __restrict__ out,
    float* __restrict__ lse, int B, int Sq, int Skv, int q_off, int Hq,
    int Hkv, float scale, int causal, int64_t k_sb, int64_t k_sh,
    int64_t k_ss, int64_t v_sb, int64_t v_sh, int64_t v_ss, float* o_state,
    float* ml_state, int first, int last) {
  static_assert(D == 64 || D == 128);
  constexpr int KCH = D / 32;      // QK^T k-chunks
  constexpr int NSUB = BN / 16;    // score col tiles = 4
  constexpr int NS_PV = D / 16;    // PV output col tiles
  constexpr int NPAN = (BN / 32) * (D / 16);  // V panels [32 keys][16 dv]
  constexpr int NLD = BN * D / 8 / BLOCK;     // 16-byte loads per thread
  constexpr int VPR = D / 8;                  // 16-byte vectors per row
  static_assert(NSUB == 4 && NS_PV % 4 == 0);

  // layouts as in v2 (K rows padded to 17 slots, V as [32][16] panels for
  // ds_read_b64_tr_b16), times two buffers
  __shared__ bf16 k_lds[2][BN][D + 8];
  __shared__ bf16 v_pan[2][NPAN * PSTRIDE];
  __shared__ bf16 p_lds[4][16][BN + PPAD];   // per wave, both fragments

  const int qt = gridDim.x - 1 - blockIdx.x;   // heavy query tiles first
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = h / (Hq / Hkv);
  const int q0 = qt * BM;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int quad = lane >> 4;
  const int r0 = wave * 32;                  // wave's first row in tile

  // ---- Q fragments in registers: rows r0 + f*16 + col ----
  bf16x8_t qfrag[2][KCH];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int qrow = q0 + r0 + f * 16 + col;
    const int safe = min(qrow, Sq - 1);
    const bf16* qp = q + (((int64_t)b * Sq + safe) * Hq + h) * D;
#pragma unroll
    for (int c = 0; c < KCH; ++c)
      qfrag[f][c] = *reinterpret_cast<const bf16x8_t*>(qp + c * 32 + quad * 8);
  }

  float m_run[2][4], l_run[2][4];
  f32x4 oacc[2][NS_PV];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { m_run[f][r] = -1e30f; l_run[f][r] = 0.f; }
#pragma unroll
    for (int n = 0; n < NS_PV; ++n) oacc[f][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  // C-fragment addressing of the state: 16 lanes cover 64 contiguous bytes
  // of an o_state row; the 16 lanes of a quad share a row's (m, l) pair
  if constexpr (CARRY) {
    if (!first) {
      const int64_t obase = ((int64_t)b * Sq) * Hq * D + (int64_t)h * D;
      const int64_t mlbase = ((int64_t)b * Hq + h) * Sq;
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qrow = q0 + r0 + f * 16 + quad * 4 + r;
          if (qrow < Sq) {
            const float2 ml = *reinterpret_cast<const float2*>(
                ml_state + (mlbase + qrow) * 2);
            m_run[f][r] = ml.x;
            l_run[f][r] = ml.y;
#pragma unroll
            for (int n = 0; n < NS_PV; ++n)
              oacc[f][n][r] =
                  o_state[obase + (int64_t)qrow * Hq * D + n * 16 + col];
          }
        }
    }
  }

  // key tiles: the block stages what its last live 64-row half needs; a
  // wave computes the tiles v2 runs for its half (none if the half starts
  // at or past Sq: those rows are never stored)
  const int halves = (min(BM, Sq - q0) + HALF - 1) / HALF;   // 1 or 2
  const int kv_end_blk =
      causal ? min(Skv, q_off + q0 + halves * HALF) : Skv;
  const int n_tiles = (kv_end_blk + BN - 1) / BN;
  const int half0 = q0 + (wave >> 1) * HALF;
  const int kv_end_w = causal ? min(Skv, q_off + half0 + HALF) : Skv;
  const int my_tiles = half0 < Sq ? (kv_end_w + BN - 1) / BN : 0;

  const bf16* kb = k + (int64_t)b * k_sb + (int64_t)hkv * k_sh;
  const bf16* vb = v + (int64_t)b * v_sb + (int64_t)hkv * v_sh;
  const int srow = threadIdx.x / VPR;          // + j * (BLOCK / VPR)
  const int sc = (threadIdx.x % VPR) * 8;

  bf16x8_t kreg[NLD], vreg[NLD];
  // keys past Skv re-read row Skv-1 (never past the tensor's last row)
  // and are zeroed on the way into LDS
  auto stage_load = [&](int kt0) {
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int key = min(kt0 + srow + j * (BLOCK / VPR), Skv - 1);
      kreg[j] = *reinterpret_cast<const bf16x8_t*>(
          kb + (int64_t)key * k_ss + sc);
      vreg[j] = *reinterpret_cast<const bf16x8_t*>(
          vb + (int64_t)key * v_ss + sc);
    }
  };
  auto stage_store = [&](int kt0, int buf) {
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int row = srow + j * (BLOCK / VPR);
      bf16x8_t kval = kreg[j], vval = vreg[j];
      if (kt0 + row >= Skv) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          kval[e] = (__bf16)0.f;
          vval[e] = (__bf16)0.f;
        }
      }
      *reinterpret_cast<bf16x8_t*>(&k_lds[buf][row][sc]) = kval;
      // panel (ks = row/32, n = c/16), row kk = row%32, col c0 = c%16
      const int pan = (row >> 5) * (D / 16) + (sc >> 4);
      *reinterpret_cast<bf16x8_t*>(
          &v_pan[buf][pan * PSTRIDE + (row & 31) * 16 + (sc & 15)]) = vval;
    }
  };

  stage_load(0);
  stage_store(0, 0);
  __syncthreads();

  for (int t = 0; t < n_tiles; ++t) {
    const int kt0 = t * BN;
    const int cur = t & 1;
    const bool more = t + 1 < n_tiles;
    if (more) stage_load(kt0 + BN);

    if (t < my_tiles) {
      // ---- QK^T: each K fragment feeds both row fragments ----
      f32x4 sacc[2][NSUB];
#pragma unroll
      for (int ns = 0; ns < NSUB; ++ns) {
        sacc[0][ns] = (f32x4){0.f, 0.f, 0.f, 0.f};
        sacc[1][ns] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
          bf16x8_t bfrag = *reinterpret_cast<const bf16x8_t*>(
              &k_lds[cur][ns * 16 + col][c * 32 + quad * 8]);
          sacc[0][ns] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              qfrag[0][c], bfrag, sacc[0][ns], 0, 0, 0);
          sacc[1][ns] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              qfrag[1][c], bfrag, sacc[1][ns], 0, 0, 0);
        }
      }

      // ---- softmax per fragment; P through the wave's LDS tile ----
      // the mask compare only where the tile crosses Skv or the wave's
      // first row's diagonal (wave-uniform: EXEC stays full for the
      // transposed reads)
      const bool need_mask =
          (kt0 + BN > Skv) || (causal && kt0 + BN - 1 > q_off + q0 + r0);
      float alpha[2][4];
      bf16x8_t pa[2][BN / 32];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        if (need_mask)
          softmax_frag<true, CARRY != 0>(
              sacc[f], m_run[f], l_run[f], alpha[f], kt0,
              q_off + q0 + r0 + f * 16, Skv, causal, scale, p_lds[wave], col,
              quad);
        else
          softmax_frag<false, CARRY != 0>(
              sacc[f], m_run[f], l_run[f], alpha[f], kt0,
              q_off + q0 + r0 + f * 16, Skv, causal, scale, p_lds[wave], col,
              quad);
#pragma unroll
        for (int ks = 0; ks < BN / 32; ++ks)
          pa[f][ks] = *reinterpret_cast<const bf16x8_t*>(
              &p_lds[wave][col][ks * 32 + quad * 8]);
      }

      // ---- O = O*alpha + P V: each V fragment feeds both ----
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int n = 0; n < NS_PV; ++n)
#pragma unroll
          for (int r = 0; r < 4; ++r) oacc[f][n][r] *= alpha[f][r];
#pragma unroll
      for (int ks = 0; ks < BN / 32; ++ks) {
#pragma unroll
        for (int n4 = 0; n4 < NS_PV; n4 += 4) {
          const unsigned pan_base = (unsigned)(uintptr_t)(
              &v_pan[cur][(ks * (D / 16) + n4) * PSTRIDE]);
          bf16x8_t vfrag[4];
          ds_read_tr16_frag4(tr16_frag_addr(pan_base, lane), vfrag);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            oacc[0][n4 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                pa[0][ks], vfrag[i], oacc[0][n4 + i], 0, 0, 0);
            oacc[1][n4 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                pa[1][ks], vfrag[i], oacc[1][n4 + i], 0, 0, 0);
          }
        }
      }
    }

    if (more) stage_store(kt0 + BN, cur ^ 1);
    __syncthreads();   // tile t+1 visible; tile t's buffer free for t+2
  }

  // ---- carried epilogue: the state goes back as it is, out untouched ----
  if constexpr (CARRY) {
    if (!last) {
      const int64_t obase = ((int64_t)b * Sq) * Hq * D + (int64_t)h * D;
      const int64_t mlbase = ((int64_t)b * Hq + h) * Sq;
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qrow = q0 + r0 + f * 16 + quad * 4 + r;
          if (qrow < Sq) {
#pragma unroll
            for (int n = 0; n < NS_PV; ++n)
              o_state[obase + (int64_t)qrow * Hq * D + n * 16 + col] =
                  oacc[f][n][r];
            if (col == 0)
              *reinterpret_cast<float2*>(ml_state + (mlbase + qrow) * 2) =
                  make_float2(m_run[f][r], l_run[f][r]);
          }
        }
      return;
    }
  }

  // ---- epilogue: divide by l, store (+ logsumexp for backward) ----
  {
    const int64_t obase = ((int64_t)b * Sq) * Hq * D + (int64_t)h * D;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + f * 16 + quad * 4 + r;
        const float linv = l_run[f][r] > 0.f ? 1.f / l_run[f][r] : 0.f;
        if (q0 + row < Sq) {
#pragma unroll
          for (int n = 0; n < NS_PV; ++n)
            out[obase + (int64_t)(q0 + row) * Hq * D + n * 16 + col] =
                f2bf(oacc[f][n][r] * linv);
          if (lse && col == 0)
            lse[((int64_t)b * Hq + h) * Sq + q0 + row] =
                l_run[f][r] > 0.f ? m_run[f][r] + __logf(l_run[f][r])
                                  : -1e30f;
        }
      }
  }
}

}  // namespace

extern "C" void tl_prefill_attn_v3(
    const void* q, const void* k, const void* v, void* out, void* lse, int B,
    int Sq, int Skv, int q_off, int Hq, int Hkv, int D, float scale,
    int causal, int64_t k_sb, int64_t k_sh, int64_t k_ss, int64_t v_sb,
    int64_t v_sh, int64_t v_ss, hipStream_t stream) {
  dim3 grid((Sq + BM - 1) / BM, Hq, B), block(BLOCK);
  if (D == 128)
    hipLaunchKernelGGL((prefill_attn_v3_kernel<128, 0>), grid, block, 0,
                       stream, (const bf16*)q, (const bf16*)k,
                       (const bf16*)v, (bf16*)out, (float*)lse, B, Sq, Skv,
                       q_off, Hq, Hkv, scale, causal, k_sb, k_sh, k_ss, v_sb,
                       v_sh, v_ss, (float*)nullptr, (float*)nullptr, 1, 1);
  else if (D == 64)
    hipLaunchKernelGGL((prefill_attn_v3_kernel<64, 0>), grid, block, 0,
                       stream, (const bf16*)q, (const bf16*)k,
                       (const bf16*)v, (bf16*)out, (float*)lse, B, Sq, Skv,
                       q_off, Hq, Hkv, scale, causal, k_sb, k_sh, k_ss, v_sb,
                       v_sh, v_ss, (float*)nullptr, (float*)nullptr, 1, 1);
}

// Carried-state entry: one key chunk of a longer softmax per call (see the
// kernel's comment). out / lse are written only when `last` (lse may be
// null); the state is read unless `first` and written unless `last`.
extern "C" void tl_prefill_attn_carry(
    const void* q, const void* k, const void* v, void* out, void* lse,
    void* o_state, void* ml_state, int B, int Sq, int Skv, int q_off, int Hq,
    int Hkv, int D, float scale, int causal, int first, int last,
    int64_t k_sb, int64_t k_sh, int64_t k_ss, int64_t v_sb, int64_t v_sh,
    int64_t v_ss, hipStream_t stream) {
  dim3 grid((Sq + BM - 1) / BM, Hq, B), block(BLOCK);
  if (D == 128)
    hipLaunchKernelGGL((prefill_attn_v3_kernel<128, 1>), grid, block, 0,
                       stream, (const bf16*)q, (const bf16*)k,
                       (const bf16*)v, (bf16*)out, (float*)lse, B, Sq, Skv,
                       q_off, Hq, Hkv, scale, causal, k_sb, k_sh, k_ss, v_sb,
                       v_sh, v_ss, (float*)o_state, (float*)ml_state, first,
                       last);
  else if (D == 64)
    hipLaunchKernelGGL((prefill_attn_v3_kernel<64, 1>), grid, block, 0,
                       stream, (const bf16*)q, (const bf16*)k,
                       (const bf16*)v, (bf16*)out, (float*)lse, B, Sq, Skv,
                       q_off, Hq, Hkv, scale, causal, k_sb, k_sh, k_ss, v_sb,
                       v_sh, v_ss, (float*)o_state, (float*)ml_state, first,
                       last);
}
