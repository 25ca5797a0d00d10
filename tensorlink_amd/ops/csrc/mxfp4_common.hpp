// Shared pieces of the MXFP4 weight-only kernels (mxfp4_gemm.hip: one
// weight; mxfp4_moe_gemm.hip: grouped experts), on top of the family
// header, which brings the s-ordered reduce: the e2m1 decode, the byte ->
// float2 table build and the 128-k split slice, so the two kernels cannot
// drift apart there: wherever their split counts agree a row is bitwise
// the same from either. The 128-k step body, the three slice lines and the
// epilogue are still written out in both kernels: as a shared k loop, and
// again with only a family_k_slice at a 128-k step and store_cfrag_* in
// their place, the MT = 4 kernels measured 3-5 % slower on the gate_up and
// Mixtral down shapes (profiles/gemm_family_refactor.md).
#pragma once

#include "gemm_family.hpp"

namespace {

constexpr int MX_BLOCK = 256;
constexpr int MX_KSTEP = 128;                // k per main-loop step
constexpr int MX_ROW_BYTES = MX_KSTEP * 2;   // one slab row (bf16)
constexpr int MX_LUT_BYTES = 256 * 8;        // byte -> float2

using mx_f32x2 = __attribute__((ext_vector_type(2))) float;

// e2m1 code (4 bits) -> f32, exact
DEVINLINE float e2m1_to_f32(int c) {
  const int m = c & 7;
  const float v = m < 2 ? 0.5f * (float)m
                        : 0.25f * (float)((2 + (m & 1)) << (m >> 1));
  return (c & 8) ? -v : v;
}

// 256-entry LDS table: packed byte -> (low nibble, high nibble) as f32.
// One entry per thread of a 256-thread block; the caller's next barrier
// publishes it.
DEVINLINE void mxfp4_build_lut(unsigned char* lut) {
  const int b = threadIdx.x;                 // MX_BLOCK == 256 entries
  mx_f32x2 v;
  v[0] = e2m1_to_f32(b & 15);
  v[1] = e2m1_to_f32(b >> 4);
  *reinterpret_cast<mx_f32x2*>(lut + b * 8) = v;
}

// k range of one split: whole 128-k steps, ceil-divided over the splits
// (the bf16 family's gemm_k_slice rule in 128-k steps; see the top of this
// file for why it is not a shared call). The bindings require
// K % 128 == 0, so K / MX_KSTEP counts every step and the splits cover K.
// Split s covers [s * k_per, min(K, (s + 1) * k_per)); a trailing split
// may be empty and then contributes zeros.
DEVINLINE int mxfp4_k_per(int K, int n_split) {
  const int steps = K / MX_KSTEP;
  return ((steps + n_split - 1) / n_split) * MX_KSTEP;
}

}  // namespace
