// Column-balanced split-K GEMM for the decode projections the policy splits
// (qkv, o_proj, down_proj at 65 <= M <= 512): the fp32 partials
// [n_split, M, N] of x[M,K] @ W[N,K]^T, bitwise equal to
// gemm_tiled_kernel<., 0, 1>'s, for the same consumers (splitk_reduce.hip,
// rmsnorm.hip, rope_append.hip).
//
// SAME per-element accumulation as the family (gemm_family.hpp): for split
// s the chunks of family_k_slice<1>(K, n_split, s) ascending from its begin,
// two mfma_f32_16x16x32_bf16 per 64-k chunk in kk order, a 32-wide tail
// taking kk = 0 only, f32 accumulators from zero. Every partial element is
// ONE K chain, so it does not depend on M, on the workgroup count or on how
// the columns are dealt out. An empty trailing split writes zeros. Do not
// change the loop order here without changing the family to match.
//
// Decomposition (gemm_policy.hpp): grid (G, n_split, ceil(M / 256)), one
// 8-wave workgroup per CU when G = CUs / n_split. A workgroup takes all rows
// of its 256-row block and colbal_range(N / 16, G, blockIdx.x) of the
// 16-column tiles, walked in equalised sub-ranges of at most SLOTS tiles.
// o_proj and down_proj (224 tiles, 8 splits) get 7 tiles per workgroup, a
// 256 x 112 tile where gemm_tiled_kernel's is 256 x 64; qkv (288 tiles, 4
// splits) gets 4 or 5 and takes the SLOTS = 5 build.
//
// Pipeline: gemm_colbal.hip's. Both operands go through LDS by
// global_load_lds in the family's swizzled image; a stage is (256 + SLOTS *
// 16) rows x 64 k (46 KB at 7 slots), three stages in ONE shared object
// form a ring with ONE raw barrier per chunk and counted vmcnt, and the
// barrier sits between the two MFMA clusters of a chunk (half-chunk
// software pipeline, fragment reads interleaved into the MFMAs).
//
// Waves are 8(M) x 1(N): 32 rows x SLOTS tiles each, 2 * SLOTS accumulators,
// SLOTS + 2 ds_read_b128 per 2 * SLOTS MFMAs; any SLOTS divides evenly. The
// tile leaves through LDS: accumulators are written to a [256][SLOTS * 16]
// fp32 image and read back by rows for 16-byte global stores.

#include "gemm_family.hpp"

namespace {

constexpr int SK_BM = 256;               // rows per workgroup
constexpr int SK_STAGES = 3;

template <int SLOTS>
__global__ __launch_bounds__(512, 1) void gemm_colbal_sk_kernel(
    const bf16* __restrict__ x,     // [M, K]
    const bf16* __restrict__ w,     // [N, K]
    float* __restrict__ partial,    // [n_split, M, N]
    int M, int N, int K, int n_split) {
  constexpr int ROWS = SK_BM + SLOTS * 16;    // LDS rows per stage
  constexpr int STAGE_ELEMS = ROWS * 64;
  constexpr int NP = SLOTS * 2;               // 8-row W pieces per stage
  static_assert(NP > 8 && NP <= 16, "one or two W pieces per wave");
  // epilogue image row stride in floats: + 4, so the four row groups a wave
  // writes at once (rows 4 apart) fall on different banks
  constexpr int CPAD = SLOTS * 16 + 4;
  static_assert(SK_BM * CPAD * 4 <= SK_STAGES * STAGE_ELEMS * 2,
                "the image fits the stages");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7
  const int col = lane & 15;
  const int quad = lane >> 4;
  const int l8 = lane >> 3;
  const int m_base = blockIdx.z * SK_BM;
  const int split = blockIdx.y;

  const TileRange range = colbal_range(N / 16, gridDim.x, blockIdx.x);
  if (range.count == 0) return;
  float* const slab = partial + (int64_t)split * M * N;

  const KSlice ks = family_k_slice<1>(K, n_split, split);
  if (ks.end <= ks.begin) {
    // empty trailing split: zeros over this workgroup's rows and columns
    const int vpr = range.count * 4;          // 16-byte pieces per row
    const int rows = min(SK_BM, M - m_base);
    for (int v = tid; v < rows * vpr; v += 512) {
      const int row = v / vpr, cv = v % vpr;
      *reinterpret_cast<float4*>(slab + (int64_t)(m_base + row) * N +
                                 range.start * 16 + cv * 4) =
          make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  const int k_len = ks.end - ks.begin;
  const int n_full = k_len / 64, n_chunks = (k_len + 63) / 64;
  const int n_sub = colbal_n_sub(range.count, SLOTS);

  // ONE shared object: 3 stages of [256 x-rows + SLOTS*16 w-rows][64 k],
  // reused as the [256][CPAD] fp32 epilogue image
  __shared__ bf16 lds[SK_STAGES * STAGE_ELEMS];

  // a wave whose rows are all past M skips the MFMAs (wave-uniform); it
  // still stages and meets every barrier
  const bool active = m_base + wave * 32 < M;

  for (int s = 0; s < n_sub; ++s) {
    const TileRange sub = colbal_sub_range(range, SLOTS, s);
    const int t0 = sub.start, tc = sub.count;  // tc <= SLOTS

    // source rows of this lane's loads: x rows piece*8+l8 (clamped to M),
    // W rows of slot piece/2; a slot past tc repeats the last tile's rows so
    // every wave issues a fixed number of loads per stage
    int64_t xoff[4], woff[2];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = (wave * 4 + g) * 8 + l8;
      xoff[g] = (int64_t)min(m_base + row, M - 1) * K;
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int piece = min(wave + g * 8, NP - 1);
      const int tile = t0 + min(piece >> 1, tc - 1);
      woff[g] = (int64_t)(tile * 16 + (piece & 1) * 8 + l8) * K;
    }

    // every wave stages 4 x-pieces and W piece `wave`; waves below NP - 8
    // also W piece wave + 8. The count is wave-uniform.
    auto stage = [&](int bufi, int k0) {
      bf16* sbase = lds + bufi * STAGE_ELEMS;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        stage_8x64(x + xoff[g], lane, k0, K, sbase + (wave * 4 + g) * 8 * 64);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        if (g == 1 && wave + 8 >= NP) break;
        stage_8x64(w + woff[g], lane, k0, K,
                   sbase + (SK_BM + (wave + g * 8) * 8) * 64);
      }
    };

    f32x4 acc[2 * SLOTS];
#pragma unroll
    for (int i = 0; i < 2 * SLOTS; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const bf16* sb = lds;                  // stage being computed
    bf16x8_t bfrag[2][SLOTS], afrag[2][2];
    auto read_frags = [&](int kk) {
#pragma unroll
      for (int nt = 0; nt < SLOTS; ++nt)
        bfrag[kk][nt] = lds_frag(sb + SK_BM * 64, nt * 16 + col,
                                 kk * 4 + quad);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
        afrag[kk][mt] = lds_frag(sb, wave * 32 + mt * 16 + col, kk * 4 + quad);
    };
    auto mfmas = [&](int kk) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < SLOTS; ++nt)
          acc[mt * SLOTS + nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[kk][mt], bfrag[kk][nt], acc[mt * SLOTS + nt], 0, 0, 0);
    };
    // chunk t is in LDS for everyone and chunk t-1 is read by no one
    auto retire = [&](int t) {
      // own loads of chunk t landed; chunk t+1 stays in flight
      if (t + 1 < n_chunks) {
        if (wave + 8 < NP) waitcnt_vm<6>();
        else waitcnt_vm<5>();
      } else {
        waitcnt_vm<0>();
      }
      // this wave's reads of chunk t-1 are done before it passes the
      // barrier that lets others overwrite that stage
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    };

    // the SLOTS + 2 fragment reads go out between the first MFMAs of a
    // cluster of 2 * SLOTS (hipcc waits lgkmcnt(0) before an MFMA cluster,
    // so reads issued ahead of a cluster would all be waited for first)
#define SK_INTERLEAVE()                                                     \
  _Pragma("unroll") for (int i = 0; i < SLOTS + 2; ++i) {                   \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); /* 1 MFMA */         \
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); /* 1 DS read */      \
  }                                                                         \
  __builtin_amdgcn_sched_group_barrier(0x008, SLOTS - 2, 0)

    // Software pipeline over half chunks, as in gemm_colbal.hip: the
    // barrier that retires chunk t+1 sits between the two MFMA clusters of
    // chunk t. Per output element the MFMA order is unchanged: chunks
    // ascending, kk = 0 then kk = 1.
    const int kb = ks.begin;
    stage(0, kb);
    if (n_chunks > 1) stage(1, kb + 64);
    retire(0);
    if (n_chunks > 2) stage(2, kb + 128);
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
        SK_INTERLEAVE();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(0);
      }
      // chunk t+1 visible; every read of chunk t has returned, so its
      // stage takes chunk t+3
      retire(t + 1);
      if (t + 3 < n_chunks) stage(cur, kb + (t + 3) * 64);
      cur = cur == 2 ? 0 : cur + 1;
      if (active) {
        sb = lds + cur * STAGE_ELEMS;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        read_frags(0);
        mfmas(1);
        SK_INTERLEAVE();
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
      SK_INTERLEAVE();
      __builtin_amdgcn_sched_barrier(0);
      if (n_chunks == n_full) mfmas(1);
      __builtin_amdgcn_s_setprio(0);
    }
#undef SK_INTERLEAVE

    // every stage is drained (the last wait was vmcnt(0)) and, after this
    // barrier, no longer read: the LDS becomes the output image
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    float* img = reinterpret_cast<float*>(lds);
    // the epilogue's addresses are derived from an opaque copy of the
    // thread id (an empty asm, no instruction), or hipcc computes them all
    // ahead of the sub-range loop and spills K-loop registers
    int etid = tid;
    asm volatile("" : "+v"(etid));
    const int ecol = etid & 15, equad = (etid >> 4) & 3;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < SLOTS; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = wave * 32 + mt * 16 + equad * 4 + i;
          img[row * CPAD + nt * 16 + ecol] = acc[mt * SLOTS + nt][i];
        }
    __syncthreads();

    // rows of the image go out in 16-byte pieces; tc*4 pieces per row are
    // real columns
    constexpr int VPR = 4 * SLOTS;         // pieces per row
    static_assert(SK_BM * VPR % 512 == 0, "whole passes");
#pragma unroll
    for (int it = 0; it < SK_BM * VPR / 512; ++it) {
      const int v = it * 512 + etid;
      const int row = v / VPR, cv = v % VPR;
      const int orow = m_base + row;
      if (cv < tc * 4 && orow < M)
        *reinterpret_cast<float4*>(slab + (int64_t)orow * N + t0 * 16 +
                                   cv * 4) =
            *reinterpret_cast<const float4*>(&img[row * CPAD + cv * 4]);
    }
    // the image is read, and the stores have left the counter the next
    // sub-range's vmcnt waits count on, before it stages over the image
    waitcnt_vm<0>();
    __syncthreads();
  }
}

}  // namespace

extern "C" {

// partial [n_split, M, N] fp32 = the split-K partials of x @ w[N, K]^T, for
// n_split > 1 and N % 16 == 0. n_blocks: workgroups per split and 256-row
// block (colbal_sk_blocks; a test may pass any count >= 1). reduce != 0
// also runs the one reduce into out (bias or null), as tl_gemm_tiled does.
void tl_gemm_colbal_sk(const void* x, const void* w, const void* bias,
                       void* out, void* partial, int M, int N, int K,
                       int n_split, int n_blocks, int reduce,
                       hipStream_t stream) {
  dim3 grid(n_blocks, n_split, cdiv(M, SK_BM)), block(512);
  if (colbal_sk_slots(N / 16, n_blocks) == 5)
    hipLaunchKernelGGL((gemm_colbal_sk_kernel<5>), grid, block, 0, stream,
                       (const bf16*)x, (const bf16*)w, (float*)partial, M, N,
                       K, n_split);
  else
    hipLaunchKernelGGL((gemm_colbal_sk_kernel<7>), grid, block, 0, stream,
                       (const bf16*)x, (const bf16*)w, (float*)partial, M, N,
                       K, n_split);
  if (reduce) launch_splitk_reduce(partial, bias, out, M, N, n_split, stream);
}

}  // extern "C"
