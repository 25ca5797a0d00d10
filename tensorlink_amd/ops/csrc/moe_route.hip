// MoE routing around the two grouped expert GEMMs (moe_gemm.hip,
// mxfp4_moe_gemm.hip): the dispatch plan, the weighted combine and an
// opt-in fused router. No kernel here waits on another workgroup, uses a
// global atomic, needs a pre-zeroed buffer or syncs with the host; every
// buffer is an output or a scratch that is fully written before it is
// read, so the path replays under a captured graph.
//
// 1. Dispatch plan (moe_plan_*): a stable counting sort of the P = T * k
//    (token, slot) pairs by expert. Within an expert the pairs ascend by
//    p = t * k + s, so seg_off / pair_tok / pos equal what a stable argsort
//    of idx.view(-1), a bincount + cumsum and the inverse permutation give,
//    element for element. A block owns 1024 consecutive pairs, one per
//    thread. A pair's rank among the earlier pairs of its expert inside
//    the block is
//        (pairs of that expert in earlier waves) + (in earlier lanes),
//    the second from wave ballots over the bits of the expert id, the
//    first from per-wave per-expert counts scanned in wave order in LDS.
//    P <= 1024 (every decode shape) is ONE launch: the block also scans
//    the expert totals into seg_off. Larger P is three: an LDS histogram
//    per block, one workgroup that turns the [nblk, E] counts into each
//    block's first row per expert (in place) and writes seg_off, and the
//    rank kernel again. Expert ids are clamped into [0, E) before use.
//
// 2. Weighted combine (moe_combine_kernel):
//        out[t] = bf16( sum_s float(bf16( y[pos[t, s]] * w[t, s] )) )
//    fp32 sum from 0.f, s ascending. One thread owns 8 columns (16 bytes)
//    of one token and reads its k rows before the first add; a token's row
//    never leaves its workgroup, and a workgroup takes 256 / (H / 8) tokens
//    when H < 2048.
//
// 3. Fused router (moe_gate_topk_kernel): logits = bf16(x @ gate_w^T) on
//    mfma_f32_16x16x32_bf16 under the family's per-chain rule
//    (gemm_family.hpp: 64-k chunks from 0, two MFMAs per chunk in kk order,
//    a 32-wide tail taking kk = 0, f32 accumulators, one rounding), then
//    top-k ON THE LOGITS and the renormalised softmax of the selected, all
//    inside the block. One workgroup of four waves per 16 token rows; the
//    columns are padded to 16-wide tiles by clamping W rows to E - 1 and
//    the padding takes no part afterwards.
//      E >= 64: the waves divide the column tiles (wave w: tiles w, w + 4)
//               and each walks the whole of K: one chain per logit.
//      E <  64: every wave holds all the tiles and the waves divide the
//               64-k chunks (wave w: chunks w, w + 4, ...); the four f32
//               partials meet in LDS and are added in wave order from p0.
//    Either way a logit's summation order is a function of (H, E) only, so
//    a token's routing is bitwise the same in any batch. The fragments are
//    read straight from global memory, 16 bytes per lane: the x tile is
//    16 x H and gate_w at most 128 x H, both L2-resident and shared by all
//    blocks, and a [16 x 64] LDS image would be written once per read.
//    Top-k: 16 lanes per row, each holding 8 packed keys
//        (monotone 16-bit key of the bf16 logit) << 8 | (255 - e)
//    and k rounds of one unsigned max: the greater value wins, among equal
//    values the smaller expert; -0 == +0; a NaN orders below -inf but above
//    "no column" (0), so k distinct experts in [0, E) always come out.
//    weights[s] = expf(l_s - l_0) / sum_j expf(l_j - l_0), fp32, j ascending,
//    one rounding to bf16.

#include "gemm_family.hpp"

// no packed fp32 arithmetic in this file's device code (the combine's
// multiply-round-add, the router's partial sums)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int PLAN_BLOCK = 1024;   // pairs per block, one per thread
constexpr int PLAN_E_MAX = 128;

// ---------------------------------------------------------------------------
// 1. dispatch plan
// ---------------------------------------------------------------------------
template <typename IT>
DEVINLINE int load_expert(const IT* idx, int p, int E) {
  const long long v = (long long)idx[p];
  return v < 0 ? 0 : v > E - 1 ? E - 1 : (int)v;
}

// Exclusive prefix of v over threads 0..127 (two waves); every thread of
// the block calls it, threads >= 128 get garbage. `carry` is one LDS int.
DEVINLINE int excl_scan128(int v, int* carry) {
  const int lane = threadIdx.x & 63;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off, WAVE_SIZE);
    if (lane >= off) inc += o;
  }
  if (threadIdx.x == 63) *carry = inc;
  __syncthreads();
  if (threadIdx.x >= 64) inc += *carry;
  return inc - v;
}

template <typename IT>
__global__ __launch_bounds__(PLAN_BLOCK) void moe_plan_hist_kernel(
    const IT* __restrict__ idx,        // [P]
    int* __restrict__ blk,             // [nblk, E] counts
    int P, int E) {
  __shared__ int cnt[PLAN_E_MAX];
  const int tid = threadIdx.x;
  const int p = blockIdx.x * PLAN_BLOCK + tid;
  if (tid < E) cnt[tid] = 0;
  __syncthreads();
  if (p < P) atomicAdd(&cnt[load_expert(idx, p, E)], 1);
  __syncthreads();
  if (tid < E) blk[(int64_t)blockIdx.x * E + tid] = cnt[tid];
}

// One workgroup: thread (e, g) owns expert e over the g-th eighth of the
// blocks. blk turns, in place, from counts into
//   blk[b][e] = seg_off[e] + pairs of e in blocks < b.
__global__ __launch_bounds__(1024) void moe_plan_scan_kernel(
    int* __restrict__ blk,             // [nblk, E]
    int* __restrict__ seg_off,         // [E + 1]
    int nblk, int E) {
  __shared__ int part[8][PLAN_E_MAX];
  __shared__ int segs[PLAN_E_MAX];
  __shared__ int carry;
  const int tid = threadIdx.x;
  const int e = tid & 127, g = tid >> 7;
  const int per = cdiv(nblk, 8);
  const int b0 = min(g * per, nblk), b1 = min(b0 + per, nblk);
  int s = 0;
  if (e < E)
    for (int b = b0; b < b1; ++b) s += blk[(int64_t)b * E + e];
  part[g][e] = s;
  __syncthreads();
  int tot = 0, before = 0;
#pragma unroll
  for (int gg = 0; gg < 8; ++gg) {
    const int v = part[gg][e];
    before += gg < g ? v : 0;
    tot += v;
  }
  const int ex = excl_scan128(tot, &carry);
  if (tid < 128) {
    segs[e] = ex;
    if (e < E) seg_off[e] = ex;
    if (e == E - 1) seg_off[E] = ex + tot;
  }
  __syncthreads();
  if (e < E) {
    int run = segs[e] + before;
    for (int b = b0; b < b1; ++b) {
      const int c = blk[(int64_t)b * E + e];
      blk[(int64_t)b * E + e] = run;
      run += c;
    }
  }
}

// SINGLE: the whole plan of a P <= 1024 call, blk unused. Otherwise the
// third kernel of the split path, reading its bases from blk. blockDim is a
// multiple of 64, >= 128 (threads 0..E-1 own an expert each).
template <typename IT, bool SINGLE>
__global__ __launch_bounds__(PLAN_BLOCK) void moe_plan_rank_kernel(
    const IT* __restrict__ idx,        // [P]
    const int* __restrict__ blk,       // [nblk, E] bases
    int* __restrict__ seg_off,         // [E + 1] (written when SINGLE)
    int* __restrict__ pair_tok,        // [P]
    int* __restrict__ pos,             // [P]
    int P, int E, int k, int nbits) {
  __shared__ int wcnt[(PLAN_BLOCK / 64) * PLAN_E_MAX];
  __shared__ int base[PLAN_E_MAX];
  __shared__ int carry;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int nw = blockDim.x >> 6;
  const int p = blockIdx.x * PLAN_BLOCK + tid;
  const bool valid = p < P;
  const int e = valid ? load_expert(idx, p, E) : 0;

  for (int i = tid; i < nw * E; i += blockDim.x) wcnt[i] = 0;

  // lanes of this wave holding the same expert
  unsigned long long same = __ballot(valid);
  for (int bit = 0; bit < nbits; ++bit) {
    const bool on = (e >> bit) & 1;
    const unsigned long long b = __ballot(on);
    same &= on ? b : ~b;
  }
  const int rank_w = __popcll(same & ((1ull << lane) - 1ull));
  __syncthreads();
  if (valid && rank_w == 0) wcnt[wave * E + e] = __popcll(same);
  __syncthreads();

  // counts -> exclusive prefix over the waves, in wave order
  int tot = 0;
  if (tid < E) {
    for (int w = 0; w < nw; ++w) {
      const int c = wcnt[w * E + tid];
      wcnt[w * E + tid] = tot;
      tot += c;
    }
  }
  if (SINGLE) {
    const int ex = excl_scan128(tot, &carry);
    if (tid < E) {
      base[tid] = ex;
      seg_off[tid] = ex;
      if (tid == E - 1) seg_off[E] = ex + tot;
    }
  } else if (tid < E) {
    base[tid] = blk[(int64_t)blockIdx.x * E + tid];
  }
  __syncthreads();
  if (valid) {
    const int dst = base[e] + wcnt[wave * E + e] + rank_w;
    pair_tok[dst] = p / k;
    pos[p] = dst;
  }
}

// ---------------------------------------------------------------------------
// 2. weighted combine
// ---------------------------------------------------------------------------
constexpr int COMBINE_K_MAX = 8;

__global__ __launch_bounds__(256) void moe_combine_kernel(
    const bf16* __restrict__ y,        // [P, H] expert-sorted pair rows
    const bf16* __restrict__ w,        // [T, k] token order
    const int* __restrict__ pos,       // [T, k] sorted row of pair (t, s)
    bf16* __restrict__ out,            // [T, H]
    int T, int H, int k) {
  const int HV = H >> 3;                       // 16-byte vectors per row
  const int rpb = HV >= 256 ? 1 : 256 / HV;    // tokens per block
  const int r = threadIdx.x / HV;              // 0 when rpb == 1
  if (r >= rpb) return;
  const int t = blockIdx.x * rpb + r;
  if (t >= T) return;
  const int P = T * k;
  const int step = rpb == 1 ? 256 : HV;

  int row[COMBINE_K_MAX];
  float ws[COMBINE_K_MAX];
#pragma unroll
  for (int s = 0; s < COMBINE_K_MAX; ++s) {
    const int ss = min(s, k - 1);
    row[s] = min(max(pos[t * k + ss], 0), P - 1);
    ws[s] = bf2f(w[t * k + ss]);
  }
  for (int hv = threadIdx.x - r * HV; hv < HV; hv += step) {
    bf16x8 v[COMBINE_K_MAX];
#pragma unroll
    for (int s = 0; s < COMBINE_K_MAX; ++s)
      if (s < k)
        v[s] = *reinterpret_cast<const bf16x8*>(y + (int64_t)row[s] * H +
                                                hv * 8);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int s = 0; s < COMBINE_K_MAX; ++s)
      if (s < k) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc[j] += bf2f(f2bf(bf2f(v[s].v[j]) * ws[s]));
      }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.v[j] = f2bf(acc[j]);
    *reinterpret_cast<bf16x8*>(out + (int64_t)t * H + hv * 8) = o;
  }
}

// ---------------------------------------------------------------------------
// 3. fused router
// ---------------------------------------------------------------------------
constexpr int GATE_ROWS = 16;
constexpr int GATE_E_MAX = 128;

// bf16 bits -> 16-bit key, monotone in the router's order: NaN (either
// sign) -> 1, below -inf (0x0080); both zeros share 0x8000.
DEVINLINE unsigned gate_key(unsigned b) {
  const unsigned mag = b & 0x7FFFu;
  const unsigned ord = (b & 0x8000u) ? 0x8000u - mag : 0x8000u + mag;
  return mag > 0x7F80u ? 1u : ord;
}

DEVINLINE bf16x8_t load_frag(const bf16* p) {
  return *reinterpret_cast<const bf16x8_t*>(p);
}

// KSPLIT false: wave w holds column tiles w + 4 * j, j < NTW, whole K.
// KSPLIT true:  every wave holds tiles j < NTW, wave w the chunks w + 4 * i.
// A tile past the last real one reads row E - 1 again and is dropped.
template <bool KSPLIT, int NTW>
__global__ __launch_bounds__(256) void moe_gate_topk_kernel(
    const bf16* __restrict__ x,        // [T, H]
    const bf16* __restrict__ gw,       // [E, H]
    int* __restrict__ idx_out,         // [T, k]
    bf16* __restrict__ w_out,          // [T, k]
    bf16* __restrict__ logits,         // [T, E]
    int T, int H, int E, int k) {
  __shared__ unsigned short tile[GATE_ROWS][GATE_E_MAX];   // bf16 bits
  __shared__ float red[KSPLIT ? 4 : 1][GATE_ROWS][KSPLIT ? NTW * 16 : 1];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int m_base = blockIdx.x * GATE_ROWS;

  const bf16* xrow = x + (int64_t)min(m_base + col, T - 1) * H + quad * 8;
  const bf16* wrow[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int nt = KSPLIT ? j : wave + 4 * j;
    wrow[j] = gw + (int64_t)min(nt * 16 + col, E - 1) * H + quad * 8;
  }
  f32x4 acc[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int n_chunk = cdiv(H, 64);
  const int c_step = KSPLIT ? 4 : 1;
  // one chunk's fragments: kk = 0 and kk = 1 of x and of each tile. The
  // 32-wide tail reads kk = 0 twice and its second MFMA is skipped.
  bf16x8_t a0, a1, b0[NTW], b1[NTW];
  bf16x8_t na0, na1, nb0[NTW], nb1[NTW];
  auto fetch = [&](int c, bf16x8_t& fa0, bf16x8_t& fa1,
                   bf16x8_t (&fb0)[NTW], bf16x8_t (&fb1)[NTW]) {
    const int k0 = c * 64;
    const int k1 = k0 + 64 <= H ? k0 + 32 : k0;
    fa0 = load_frag(xrow + k0);
    fa1 = load_frag(xrow + k1);
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      fb0[j] = load_frag(wrow[j] + k0);
      fb1[j] = load_frag(wrow[j] + k1);
    }
  };
  const int c_first = KSPLIT ? wave : 0;
  if (c_first < n_chunk) fetch(c_first, na0, na1, nb0, nb1);
  for (int c = c_first; c < n_chunk; c += c_step) {
    const bool full = c * 64 + 64 <= H;        // else the 32-wide tail
    a0 = na0;
    a1 = na1;
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      b0[j] = nb0[j];
      b1[j] = nb1[j];
    }
    // the next chunk's loads fly under this chunk's MFMAs; past the end
    // the wave re-reads its last chunk (in bounds, never used)
    fetch(c + c_step < n_chunk ? c + c_step : c, na0, na1, nb0, nb1);
#pragma unroll
    for (int j = 0; j < NTW; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0[j], acc[j], 0,
                                                       0, 0);
    if (full) {
#pragma unroll
      for (int j = 0; j < NTW; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1[j], acc[j],
                                                         0, 0, 0);
    }
  }

  // accumulators -> the block's [16][E] tile of rounded logits
  if (KSPLIT) {
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        red[wave][quad * 4 + r][j * 16 + col] = acc[j][r];
    __syncthreads();
    for (int i = tid; i < GATE_ROWS * NTW * 16; i += 256) {
      const int rr = i / (NTW * 16), cc = i % (NTW * 16);
      float s = red[0][rr][cc];
      s += red[1][rr][cc];
      s += red[2][rr][cc];
      s += red[3][rr][cc];
      tile[rr][cc] = __bfloat16_as_ushort(f2bf(s));
    }
  } else {
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        tile[quad * 4 + r][(wave + 4 * j) * 16 + col] =
            __bfloat16_as_ushort(f2bf(acc[j][r]));
  }
  __syncthreads();

  unsigned short* lg = reinterpret_cast<unsigned short*>(logits);
  const int rows = min(GATE_ROWS, T - m_base);
  for (int i = tid; i < rows * E; i += 256)
    lg[(int64_t)m_base * E + i] = tile[i / E][i % E];

  // top-k: 16 lanes per row, lane c holds experts c, c + 16, ..
  const int row = tid >> 4;                    // 0..15
  unsigned key[GATE_E_MAX / 16];
#pragma unroll
  for (int j = 0; j < GATE_E_MAX / 16; ++j) {
    const int e = j * 16 + col;
    key[j] = e < E ? gate_key(tile[row][e]) << 8 | (unsigned)(255 - e) : 0u;
  }
  int my_e = 0;
  float my_l = 0.f, l_max = 0.f;
  for (int s = 0; s < k; ++s) {
    unsigned best = 0u;
#pragma unroll
    for (int j = 0; j < GATE_E_MAX / 16; ++j) best = max(best, key[j]);
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
      best = max(best, (unsigned)__shfl_xor((int)best, off, WAVE_SIZE));
    const int e = min(255 - (int)(best & 0xFFu), E - 1);   // k <= E: no-op
#pragma unroll
    for (int j = 0; j < GATE_E_MAX / 16; ++j)
      if (key[j] == best) key[j] = 0u;          // keys are distinct
    const float l =
        __uint_as_float((unsigned)tile[row][e] << 16);   // bf16 -> f32
    if (s == 0) l_max = l;
    if (col == s) {
      my_e = e;
      my_l = l;
    }
  }
  const float ex = col < k ? expf(my_l - l_max) : 0.f;
  float sum = 0.f;
  for (int s = 0; s < k; ++s)
    sum += __shfl(ex, (lane & 48) + s, WAVE_SIZE);
  if (col < k && m_base + row < T) {
    const int64_t o = (int64_t)(m_base + row) * k + col;
    idx_out[o] = my_e;
    w_out[o] = f2bf(ex / sum);
  }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" {

// idx [P] int64 (idx64 != 0) or int32; blk: scratch [cdiv(P, 1024) * E]
// int32, used (and fully written before it is read) only when P > 1024.
void tl_moe_plan(const void* idx, int idx64, void* blk, void* seg_off,
                 void* pair_tok, void* pos, int P, int E, int k,
                 hipStream_t stream) {
  int nbits = 0;
  while ((1 << nbits) < E) ++nbits;
  const int nblk = cdiv(P, PLAN_BLOCK);
  if (nblk == 1) {
    const int threads = P <= 128 ? 128 : cdiv(P, 64) * 64;
    if (idx64)
      hipLaunchKernelGGL((moe_plan_rank_kernel<int64_t, true>), dim3(1),
                         dim3(threads), 0, stream, (const int64_t*)idx,
                         (const int*)nullptr, (int*)seg_off, (int*)pair_tok,
                         (int*)pos, P, E, k, nbits);
    else
      hipLaunchKernelGGL((moe_plan_rank_kernel<int, true>), dim3(1),
                         dim3(threads), 0, stream, (const int*)idx,
                         (const int*)nullptr, (int*)seg_off, (int*)pair_tok,
                         (int*)pos, P, E, k, nbits);
    return;
  }
  if (idx64)
    hipLaunchKernelGGL(moe_plan_hist_kernel<int64_t>, dim3(nblk),
                       dim3(PLAN_BLOCK), 0, stream, (const int64_t*)idx,
                       (int*)blk, P, E);
  else
    hipLaunchKernelGGL(moe_plan_hist_kernel<int>, dim3(nblk),
                       dim3(PLAN_BLOCK), 0, stream, (const int*)idx,
                       (int*)blk, P, E);
  hipLaunchKernelGGL(moe_plan_scan_kernel, dim3(1), dim3(1024), 0, stream,
                     (int*)blk, (int*)seg_off, nblk, E);
  if (idx64)
    hipLaunchKernelGGL((moe_plan_rank_kernel<int64_t, false>), dim3(nblk),
                       dim3(PLAN_BLOCK), 0, stream, (const int64_t*)idx,
                       (const int*)blk, (int*)seg_off, (int*)pair_tok,
                       (int*)pos, P, E, k, nbits);
  else
    hipLaunchKernelGGL((moe_plan_rank_kernel<int, false>), dim3(nblk),
                       dim3(PLAN_BLOCK), 0, stream, (const int*)idx,
                       (const int*)blk, (int*)seg_off, (int*)pair_tok,
                       (int*)pos, P, E, k, nbits);
}

void tl_moe_combine(const void* y, const void* w, const void* pos, void* out,
                    int T, int H, int k, hipStream_t stream) {
  const int HV = H / 8;
  const int rpb = HV >= 256 ? 1 : 256 / HV;
  hipLaunchKernelGGL(moe_combine_kernel, dim3(cdiv(T, rpb)), dim3(256), 0,
                     stream, (const bf16*)y, (const bf16*)w, (const int*)pos,
                     (bf16*)out, T, H, k);
}

void tl_moe_gate_topk(const void* x, const void* gw, void* idx, void* w,
                      void* logits, int T, int H, int E, int k,
                      hipStream_t stream) {
  const dim3 grid(cdiv(T, GATE_ROWS)), block(256);
  const int NT = cdiv(E, 16);
#define TL_GATE_LAUNCH(KS, NTW)                                             \
  hipLaunchKernelGGL((moe_gate_topk_kernel<KS, NTW>), grid, block, 0,       \
                     stream, (const bf16*)x, (const bf16*)gw, (int*)idx,    \
                     (bf16*)w, (bf16*)logits, T, H, E, k)
  if (E >= 64) {
    if (NT <= 4) TL_GATE_LAUNCH(false, 1);
    else TL_GATE_LAUNCH(false, 2);
  } else if (NT == 1) {
    TL_GATE_LAUNCH(true, 1);
  } else if (NT == 2) {
    TL_GATE_LAUNCH(true, 2);
  } else {
    TL_GATE_LAUNCH(true, 4);
  }
#undef TL_GATE_LAUNCH
}

}  // extern "C"
