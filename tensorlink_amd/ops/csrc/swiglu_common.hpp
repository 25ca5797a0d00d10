// The SwiGLU element expression, shared by swiglu.hip and the fused
// gate_up epilogue of gemm_colbal.hip so both produce the same bits.
#pragma once

#include "common.hpp"

DEVINLINE float silu(float x) { return x / (1.f + __expf(-x)); }

// out = silu(gate) * up on bf16 values, one bf16 rounding at the end
DEVINLINE bf16 swiglu_bf16(bf16 g, bf16 u) {
  return f2bf(silu(bf2f(g)) * bf2f(u));
}
