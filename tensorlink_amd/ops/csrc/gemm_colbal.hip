// Column-balanced one-pass GEMM for the wide decode projections
// (gate_up: N = 37888, K = 3584): out[M,N] = x[M,K] @ W[N,K]^T in bf16, and
// a variant that applies SwiGLU to the accumulators and writes [M, I].
//
// SAME per-row accumulation as the rest of the family (skinny_gemm.hip,
// gemm_tiled.hip) at n_split == 1: K stepped in 64-element chunks from 0,
// two mfma_f32_16x16x32_bf16 per chunk in kk order, f32 accumulators, a
// 32-wide tail taking kk = 0 only. Every output element is ONE K chain, so
// the result is bitwise equal to gemm_tiled_kernel / gemm_tiled_sq_kernel
// for the same inputs and does not depend on M, on the number of
// workgroups or on how the columns are dealt out. Do not change the loop
// order here without changing the family to match.
//
// Decomposition: one 8-wave workgroup per CU; every workgroup takes all
// rows of a 256-row M block (blockIdx.z) and a contiguous range of the
// 16-column tiles, balanced by COUNT: with T tiles and G workgroups the
// first T % G get ceil(T/G), the rest floor(T/G). gate_up has 2368 tiles:
// 9 or 10 per CU in one pass, where 256-wide tiles leave 148 tiles on 256
// CUs. A range is walked in equalised sub-ranges of at most 10 tiles
// (BN <= 160). No K split, no partials, nothing shared between workgroups.
//
// Pipeline: both operands go through LDS by global_load_lds width 16 in
// full 128-byte lines, in the family's swizzled image (gemm_family.hpp),
// fragments by ds_read_b128. A stage is (256 + 160)
// rows x 64 k = 52 KB; three stages form a ring with ONE barrier per
// chunk: each wave waits (counted vmcnt, never 0 before the last chunk) for
// its own loads of chunk t+1, the barrier makes chunk t+1 visible and
// proves chunk t is no longer read, and chunk t+3 is issued into t's
// stage, so two chunks stay in flight under the MFMAs. That barrier sits
// between the two MFMA clusters of chunk t (see the K loop).
//
// Waves are 4(M) x 2(N): 64 rows x 80 columns each, 20 accumulators, 9
// ds_read_b128 per 20 MFMAs. The tile leaves through LDS: accumulators are
// rounded to bf16 exactly as the unfused store rounds them, written to a
// [256][160] image, and read back by rows for 16-byte global stores. The
// fused variant stages gate tiles in slots 0..4 and their up tiles in
// slots 5..9, so the epilogue finds gate and up of one output element in
// the same image row and applies swiglu_bf16 (swiglu_common.hpp) to them.

#include "gemm_family.hpp"
#include "swiglu_common.hpp"

namespace {

constexpr int CB_BM = 256;               // rows per workgroup
constexpr int CB_SLOTS = 10;             // 16-column MFMA tiles per stage
constexpr int CB_ROWS = CB_BM + CB_SLOTS * 16;  // LDS rows per stage
constexpr int CB_STAGES = 3;
constexpr int CB_STAGE_ELEMS = CB_ROWS * 64;
// epilogue image row stride: 160 columns + 8 pad, so the four row groups a
// wave writes at once (rows 4 apart) fall on different banks
constexpr int CB_CPAD = 168;

template <int FUSED>
__global__ __launch_bounds__(512, 1) void gemm_colbal_kernel(
    const bf16* __restrict__ x,   // [M, K]
    const bf16* __restrict__ w,   // [NO, K], FUSED: [2*NO, K] gate | up
    bf16* __restrict__ out,       // [M, NO]
    int M, int NO, int K) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7
  const int col = lane & 15;
  const int quad = lane >> 4;
  const int wm = wave >> 1;                // 0..3: 64-row band
  const int wn = wave & 1;                 // 0..1: 5-slot band
  const int l8 = lane >> 3;
  const int m_base = blockIdx.z * CB_BM;

  // slots per column tile, tiles per sub-range
  constexpr int SPT = FUSED ? 2 : 1;
  constexpr int MAXT = CB_SLOTS / SPT;

  // this workgroup's contiguous range of the NO/16 column tiles
  const int T = NO / 16, G = gridDim.x, b = blockIdx.x;
  const int q = T / G, r = T % G;
  const int cnt = q + (b < r ? 1 : 0);
  const int start = b * q + min(b, r);
  if (cnt == 0) return;
  const int n_sub = (cnt + MAXT - 1) / MAXT;

  // ONE shared object: 3 stages of [256 x-rows + 160 w-rows][64 k], reused
  // as the [256][CB_CPAD] epilogue image
  __shared__ bf16 lds[CB_STAGES * CB_STAGE_ELEMS];

  // rows of this wave with nothing to store skip the MFMAs (wave-uniform);
  // they still stage and meet every barrier
  const bool active = m_base + wm * 64 < M;
  const int n_full = K / 64, n_chunks = (K + 63) / 64;

  for (int s = 0; s < n_sub; ++s) {
    const int sq = cnt / n_sub, sr = cnt % n_sub;
    const int t0 = start + s * sq + min(s, sr);   // first tile
    const int tc = sq + (s < sr ? 1 : 0);         // tiles here, <= MAXT

    // source rows of this lane's loads: x rows chunk*8+l8 (clamped to M),
    // W rows of slot wchunk/2; a slot past tc repeats the last tile's rows
    // so every wave issues a fixed number of loads per stage
    int64_t xoff[4], woff[3];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = (wave * 4 + g) * 8 + l8;
      xoff[g] = (int64_t)min(m_base + row, M - 1) * K;
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int wchunk = min(wave + g * 8, 19);
      const int slot = wchunk >> 1;
      const int half = FUSED ? (slot >= MAXT ? 1 : 0) : 0;
      const int tile = t0 + min(slot - half * MAXT, tc - 1);
      woff[g] = ((int64_t)half * NO + tile * 16 + (wchunk & 1) * 8 + l8) * K;
    }

    // waves 0..3 stage 4 x-chunks + 3 W-chunks, waves 4..7 4 + 2 (20 W
    // chunks over 8 waves); the count is wave-uniform
    auto stage = [&](int bufi, int k0) {
      bf16* sbase = lds + bufi * CB_STAGE_ELEMS;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        stage_8x64(x + xoff[g], lane, k0, K, sbase + (wave * 4 + g) * 8 * 64);
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        if (g == 2 && wave >= 4) break;
        stage_8x64(w + woff[g], lane, k0, K,
                   sbase + (CB_BM + (wave + g * 8) * 8) * 64);
      }
    };

    f32x4 acc[20];
#pragma unroll
    for (int i = 0; i < 20; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const bf16* sb = lds;                  // stage being computed
    bf16x8_t bfrag[2][5], afrag[2][4];
    auto read_frags = [&](int kk) {
#pragma unroll
      for (int nt = 0; nt < 5; ++nt)
        bfrag[kk][nt] = lds_frag(sb + CB_BM * 64, (wn * 5 + nt) * 16 + col,
                                 kk * 4 + quad);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        afrag[kk][mt] =
            lds_frag(sb, wm * 64 + mt * 16 + col, kk * 4 + quad);
    };
    auto mfmas = [&](int kk) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 5; ++nt)
          acc[mt * 5 + nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[kk][mt], bfrag[kk][nt], acc[mt * 5 + nt], 0, 0, 0);
    };
    // chunk t is in LDS for everyone and chunk t-1 is read by no one
    auto retire = [&](int t) {
      // own loads of chunk t landed; chunk t+1 stays in flight
      if (t + 1 < n_chunks) {
        if (wave < 4) waitcnt_vm<7>();
        else waitcnt_vm<6>();
      } else {
        waitcnt_vm<0>();
      }
      // this wave's reads of chunk t-1 are done before it passes the
      // barrier that lets others overwrite that stage
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    };

    // nine fragment reads go out between the first nine of twenty MFMAs
    // (hipcc waits lgkmcnt(0) before an MFMA cluster, so reads issued
    // ahead of a cluster would all be waited for first)
#define CB_INTERLEAVE()                                                     \
  _Pragma("unroll") for (int i = 0; i < 9; ++i) {                           \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); /* 1 MFMA */         \
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); /* 1 DS read */      \
  }                                                                         \
  __builtin_amdgcn_sched_group_barrier(0x008, 11, 0)

    // Software pipeline over half chunks: the barrier that retires chunk
    // t+1 sits between the two MFMA clusters of chunk t, so kk = 1's
    // fragments of chunk t are read under its kk = 0 MFMAs and kk = 0's
    // fragments of chunk t+1 under its kk = 1 MFMAs. Per output element the
    // MFMA order is unchanged: chunks ascending, kk = 0 then kk = 1.
    stage(0, 0);
    if (n_chunks > 1) stage(1, 64);
    retire(0);
    if (n_chunks > 2) stage(2, 128);
    int cur = 0;                           // stage of chunk t (and of t+3)
    if (active) read_frags(0);             // sb = stage 0
    // chunks that are full and have a successor
    const int n_piped = min(n_full, n_chunks - 1);
    for (int t = 0; t < n_piped; ++t) {
      if (active) {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        read_frags(1);
        mfmas(0);
        CB_INTERLEAVE();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(0);
      }
      // chunk t+1 visible; every read of chunk t has returned, so its
      // stage takes chunk t+3
      retire(t + 1);
      if (t + 3 < n_chunks) stage(cur, (t + 3) * 64);
      cur = cur == 2 ? 0 : cur + 1;
      if (active) {
        sb = lds + cur * CB_STAGE_ELEMS;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        read_frags(0);
        mfmas(1);
        CB_INTERLEAVE();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    // last chunk, its kk = 0 fragments already read: a full one has both
    // halves, the 32-wide tail kk = 0 only, as in gemm_tiled_kernel (its
    // kk = 1 fragments are read, they are in bounds, and dropped)
    if (active) {
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      read_frags(1);
      mfmas(0);
      CB_INTERLEAVE();
      __builtin_amdgcn_sched_barrier(0);
      if (n_chunks == n_full) mfmas(1);
      __builtin_amdgcn_s_setprio(0);
    }
#undef CB_INTERLEAVE

    // every stage is drained (the last wait was vmcnt(0)) and, after this
    // barrier, no longer read: the LDS becomes the output image
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    // the epilogue's addresses are derived from an opaque copy of the
    // thread id (an empty asm, no instruction), or hipcc computes them
    // all ahead of the sub-range loop and spills K-loop registers
    int etid = tid;
    asm volatile("" : "+v"(etid));
    const int ecol = etid & 15, equad = (etid >> 4) & 3;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 5; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = wm * 64 + mt * 16 + equad * 4 + i;
          const int c = (wn * 5 + nt) * 16 + ecol;
          // "+ 0.f": the family's store is f2bf(acc + bias) with bias 0.f
          lds[row * CB_CPAD + c] = f2bf(acc[mt * 5 + nt][i] + 0.f);
        }
    __syncthreads();

    // rows of the image go out in 16-byte pieces; tc*2 pieces per row are
    // real columns
    constexpr int VPR = 2 * MAXT;          // pieces per row
#pragma unroll
    for (int it = 0; it < CB_BM * VPR / 512; ++it) {
      const int v = it * 512 + etid;
      const int row = v / VPR, cv = v % VPR;
      const int orow = m_base + row;
      if (cv < tc * 2 && orow < M) {
        bf16x8 o = *reinterpret_cast<const bf16x8*>(
            &lds[row * CB_CPAD + cv * 8]);
        if (FUSED) {
          const bf16x8 u = *reinterpret_cast<const bf16x8*>(
              &lds[row * CB_CPAD + MAXT * 16 + cv * 8]);
#pragma unroll
          for (int j = 0; j < 8; ++j) o.v[j] = swiglu_bf16(o.v[j], u.v[j]);
        }
        *reinterpret_cast<bf16x8*>(
            out + (int64_t)orow * NO + t0 * 16 + cv * 8) = o;
      }
    }
    // the image is read before the next sub-range stages over it
    __syncthreads();
  }
}

}  // namespace

extern "C" {

// fused == 0: out[M, N] = x @ w[N, K]^T. fused != 0: w is [2N, K] (gate rows
// then up rows) and out[M, N] = silu(x @ gate^T) * (x @ up^T), each product
// rounded to bf16 first. n_blocks: workgroups per M block (the CU count).
void tl_gemm_colbal(const void* x, const void* w, void* out, int M, int N,
                    int K, int n_blocks, int fused, hipStream_t stream) {
  dim3 grid(n_blocks, 1, cdiv(M, CB_BM)), block(512);
  if (fused)
    hipLaunchKernelGGL((gemm_colbal_kernel<1>), grid, block, 0, stream,
                       (const bf16*)x, (const bf16*)w, (bf16*)out, M, N, K);
  else
    hipLaunchKernelGGL((gemm_colbal_kernel<0>), grid, block, 0, stream,
                       (const bf16*)x, (const bf16*)w, (bf16*)out, M, N, K);
}

}  // extern "C"
