// Host/device-neutral policy of the kernel library: split counts, kernel
// class thresholds. Plain C++ (no HIP headers, only inline functions and
// constexpr values) so bindings.cpp, built by the host compiler, and the
// .hip files read the SAME definitions. Python keeps one copy of the class
// thresholds in ops/__init__.py::_gemm_class for the CPU tier.
//
// Everything here is pure in the problem shape — never M, the batch or the
// launch — which is what makes a row's accumulation identical in every
// call (the serving engine's exact-greedy guarantee).
#pragma once

#ifdef __HIPCC__
#define TL_HD __host__ __device__
#else
#define TL_HD
#endif

// Flash-decode split count for ONE row of length L. Depends only on L, so
// a sequence's attention numerics are identical whatever batch it is
// decoded in (see decode_attn_mfma.hip). Monotone in L, so a host-side
// length upper bound gives a valid launch width.
TL_HD inline int tl_split_for_len(int L) {
  int ns = 1;
  while (ns < 16 && L > 1024 * ns) ns <<= 1;
  return ns;
}

// Rows up to which the streaming kernel (skinny_gemm.hip) serves a GEMM;
// above it the tiled kernels (gemm_tiled.hip) do.
constexpr int TL_GEMM_STREAM_M = 64;
// Widths from which the 256x256-tile class (gemm_tiled_sq, lm_head) serves
// the tiled range and the split policy counts 256-column panels.
constexpr int TL_GEMM_WIDE_N = 65536;

// Split-K count SHARED by the streaming and tiled bf16 GEMM kernels, pure
// in (N, K). `target` is the block count to approach before M/z tiling.
inline int gemm_n_split_for(int N, int K, int target) {
  int n_split = 1;
  if (N >= TL_GEMM_WIDE_N) {
    // enough 256-column panels to fill the chip without splitting
    while (((N + 255) / 256) * n_split < target && n_split < 16 &&
           (K / 64) / (n_split * 2) >= 16)
      n_split <<= 1;
    return n_split;
  }
  // split K so (N/64)*n_split lands near the target block count
  while ((N / 64) * n_split < target && n_split < 8 &&
         (K / 32) / (n_split * 2) >= 2)
    n_split <<= 1;
  return n_split;
}

// Split-K slice SHARED by the streaming and tiled bf16 GEMM kernels, pure
// in (K, n_split): whole 64-k chunks, ceil-divided over the splits. The
// bindings accept K % 32 == 0, so the last chunk may be a 32-wide tail; it
// counts as a chunk ((K + 63) / 64 — a floor here left the tail in no
// split whenever n_split divided K / 64). Split s covers [begin, end):
// begins are multiples of 64, the union over s is exactly [0, K), and a
// trailing split may be empty (end <= begin), contributing zeros.
struct KSlice {
  int begin, end;
};

TL_HD inline KSlice gemm_k_slice(int K, int n_split, int split) {
  const int per = (((K + 63) / 64 + n_split - 1) / n_split) * 64;
  const int begin = split * per;
  return {begin, K < begin + per ? K : begin + per};
}

// Split-K count of the MXFP4 kernels, counted in their 128-k steps: a
// column's packed bytes are 4x fewer than bf16, so a split keeps >= 2
// steps. `blocks` is the grid before the split: N/64 for mxfp4_gemm (pure
// in (N, K)), (N/64)*E for mxfp4_moe_gemm (pure in (N, K, E), never P or
// the routing).
inline int mxfp4_split_for_blocks(int blocks, int K) {
  int n_split = 1;
  while (blocks * n_split < 256 && n_split < 8 &&
         (K / 128) / (n_split * 2) >= 2)
    n_split <<= 1;
  return n_split;
}
