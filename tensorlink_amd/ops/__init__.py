"""Op dispatch: hand-written CDNA4 HIP kernels on GPU, PyTorch reference on CPU.

Policy (required by the build contract): on a GPU box the HIP extension MUST
be loadable — a missing extension raises instead of silently falling back to
eager PyTorch. On CPU-only hosts (the test tier) the fp32 reference
implementations in :mod:`tensorlink_amd.ops.reference` run instead.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from tensorlink_amd.ops import reference as ref

_C = None
_IMPORT_ERROR: Optional[BaseException] = None
try:
    from tensorlink_amd import _C  # type: ignore  # built by setup.py
except Exception as e:  # pragma: no cover - absent on CPU CI before build
    _IMPORT_ERROR = e


def extension_loaded() -> bool:
    return _C is not None


def _require_ext():
    if _C is None:
        raise RuntimeError(
            "tensorlink_amd._C HIP extension is not built but a CUDA/HIP "
            "tensor reached the op layer. Build it in-tree with "
            "`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace` "
            f"(import error: {_IMPORT_ERROR!r})")
    return _C


def _on_gpu(*tensors: torch.Tensor) -> bool:
    return any(t.is_cuda for t in tensors if isinstance(t, torch.Tensor))


# ---------------------------------------------------------------------------
# RMSNorm (autograd-aware)
# ---------------------------------------------------------------------------
class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        C = _require_ext()
        need_grad = x.requires_grad or weight.requires_grad
        outs = C.rmsnorm_fwd(x.contiguous(), None, weight.contiguous(), eps,
                             need_grad)
        y = outs[0]
        if need_grad:
            ctx.save_for_backward(x, weight, outs[1])
        return y

    @staticmethod
    def backward(ctx, dy):
        C = _require_ext()
        x, weight, rstd = ctx.saved_tensors
        dx, dw = C.rmsnorm_bwd(dy.contiguous(), x.contiguous(),
                               weight.contiguous(), rstd)
        return dx, dw, None


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6):
    if not _on_gpu(x):
        return ref.rmsnorm(x, weight, eps)
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        return _RMSNormFn.apply(x, weight, eps)
    return _require_ext().rmsnorm_fwd(x.contiguous(), None,
                                      weight.contiguous(), eps, False)[0]


def rmsnorm_residual(x: torch.Tensor, residual: torch.Tensor,
                     weight: torch.Tensor, eps: float = 1e-6):
    """Fused residual add + RMSNorm (inference path). Returns (y, r)."""
    if not _on_gpu(x):
        return ref.rmsnorm_residual(x, residual, weight, eps)
    outs = _require_ext().rmsnorm_fwd(x.contiguous(), residual.contiguous(),
                                      weight.contiguous(), eps, False)
    return outs[0], outs[1]


class Partials:
    """A projection's result before its split-K reduce: ``data`` is the
    fp32 partial tensor [n_split, ..., N] of the hand-written GEMM family
    (:func:`linear_partials`) and ``bias`` its still-unapplied bf16 bias
    (or None). The value it stands for is
    bf16(sum_s data[s] (+ bias)) summed from 0 in s order — consumers
    (:func:`rope_append_`, :func:`add_rmsnorm`, :func:`add_residual`) sum
    it in-kernel, so the reduce pass and its bf16 round trip never run."""

    __slots__ = ("data", "bias")

    def __init__(self, data: torch.Tensor, bias=None):
        self.data = data
        self.bias = bias

    @property
    def n_split(self) -> int:
        return self.data.shape[0]

    def materialize(self) -> torch.Tensor:
        """The bf16 tensor ops.linear would have returned (torch ops; for
        callers that turn out to need the plain output after all)."""
        acc = torch.zeros_like(self.data[0])
        for s in range(self.data.shape[0]):
            acc = acc + self.data[s]
        if self.bias is not None:
            acc = acc + self.bias.float()
        return acc.to(torch.bfloat16)


def add_rmsnorm(x, residual: torch.Tensor, weight: torch.Tensor,
                eps: float = 1e-6, rounded: bool = False):
    """Residual add + RMSNorm in one kernel; ``x`` is a bf16 tensor or a
    bias-free :class:`Partials`. Returns (y, r) with r = bf16(x + residual).

    rounded=False normalises the unrounded fp32 sum — exactly
    :func:`rmsnorm_residual`. rounded=True normalises r itself — exactly a
    bf16 ``x + residual`` followed by :func:`rmsnorm` (the decoder's
    layer hand-over and final norm). Off the GPU both compose the torch
    ops the CPU decoder has always run: add in the tensor dtype, norm."""
    part = isinstance(x, Partials)
    if not _on_gpu(residual):
        xt = x.materialize() if part else x
        r = residual + xt
        return ref.rmsnorm(r, weight, eps), r
    if part:
        assert x.bias is None, "add_rmsnorm takes bias-free partials"
        xt = x.data
    else:
        xt = x.contiguous()
    y, r = _require_ext().rmsnorm_add_fwd(
        xt, residual.contiguous(), weight.contiguous(), eps,
        2 if rounded else 1)
    return y, r


def add_residual(x, residual: torch.Tensor) -> torch.Tensor:
    """bf16(x + residual) with ``x`` a bf16 tensor or bias-free
    :class:`Partials` — :func:`add_rmsnorm`'s sum without the norm."""
    part = isinstance(x, Partials)
    if not _on_gpu(residual):
        return residual + (x.materialize() if part else x)
    if part:
        assert x.bias is None, "add_residual takes bias-free partials"
        xt = x.data
    else:
        xt = x.contiguous()
    return _require_ext().rmsnorm_add_fwd(xt, residual.contiguous(), None,
                                          0.0, 3)[0]


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------
def apply_rope_(q: torch.Tensor, k: torch.Tensor, positions: torch.Tensor,
                inv_freq: torch.Tensor, sign: float = 1.0) -> None:
    """In-place RoPE on q [T,Hq,D] / k [T,Hkv,D] with positions [T].

    Inference path (no autograd). sign=-1 applies the inverse rotation.
    """
    if not _on_gpu(q):
        # compute cos/sin from the PASSED inv_freq (NOT a default theta:
        # Qwen uses rope_theta=1e6, Llama-3.1 a scaled spectrum)
        freqs = positions.float()[:, None] * inv_freq.float()[None, :]
        cos, sin = freqs.cos(), freqs.sin()
        # reference expects [B,S,H,D]
        qq, kk = ref.apply_rope(q.unsqueeze(0), k.unsqueeze(0), cos,
                                sin * sign)
        q.copy_(qq[0])
        k.copy_(kk[0])
        return
    _require_ext().rope_(q, k, positions.int(), inv_freq.float(), sign)


def rope_append_(qkv, k_cache: torch.Tensor,
                 v_cache: torch.Tensor, positions: torch.Tensor,
                 inv_freq: torch.Tensor, S: int, Hq: int, Hkv: int,
                 block_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused RoPE + KV-cache append from the fused-QKV projection output.

    qkv [T, (Hq+2*Hkv)*D] with T = B*S (q | k | v per row); caches
    [B,Hkv,Smax,D] (or paged pools [n_pages,Hkv,128,D] with block_table
    [B, pages]); positions [T] gives the RoPE angle and cache slot.
    Returns the rotated q as a contiguous [T, Hq, D] tensor.

    qkv may be the projection's :class:`Partials` (reduced + biased
    in-kernel, same bits). inv_freq may be fp32 or bf16 — the kernel
    widens bf16 in-register, so no conversion kernel runs per call.
    """
    part = isinstance(qkv, Partials)
    if _on_gpu(k_cache):
        if inv_freq.dtype not in (torch.float32, torch.bfloat16):
            inv_freq = inv_freq.float()
        bt = block_table.int() if block_table is not None else None
        if part:
            return _require_ext().rope_append_(
                qkv.data, k_cache, v_cache, positions.int(),
                inv_freq.contiguous(), S, Hq, Hkv, bt, qkv.bias)
        return _require_ext().rope_append_(
            qkv.contiguous(), k_cache, v_cache, positions.int(),
            inv_freq.contiguous(), S, Hq, Hkv, bt, None)
    if part:
        qkv = qkv.materialize()
    D = k_cache.shape[-1]
    T = qkv.numel() // qkv.shape[-1]
    q = qkv[..., :Hq * D].reshape(T, Hq, D).contiguous()
    k = qkv[..., Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D).contiguous()
    v = qkv[..., (Hq + Hkv) * D:].reshape(T, Hkv, D).contiguous()
    apply_rope_(q, k, positions, inv_freq)
    B = T // S
    pos = positions.view(B, S).long()
    kB = k.view(B, S, Hkv, D)
    vB = v.view(B, S, Hkv, D)
    if block_table is None:
        for b in range(B):
            k_cache[b, :, pos[b]] = kB[b].transpose(0, 1)
            v_cache[b, :, pos[b]] = vB[b].transpose(0, 1)
    else:
        for b in range(B):
            for s_i in range(S):
                p = int(pos[b, s_i])
                page = int(block_table[b, p // 128])
                k_cache[page, :, p % 128] = kB[b, s_i]
                v_cache[page, :, p % 128] = vB[b, s_i]
    return q


class _RopeFn(torch.autograd.Function):
    """Autograd RoPE for the training path (operates out-of-place)."""

    @staticmethod
    def forward(ctx, q, k, positions, inv_freq):
        q2, k2 = q.contiguous().clone(), k.contiguous().clone()
        apply_rope_(q2, k2, positions, inv_freq, 1.0)
        ctx.save_for_backward(positions, inv_freq)
        return q2, k2

    @staticmethod
    def backward(ctx, dq, dk):
        positions, inv_freq = ctx.saved_tensors
        dq2, dk2 = dq.contiguous().clone(), dk.contiguous().clone()
        apply_rope_(dq2, dk2, positions, inv_freq, -1.0)
        return dq2, dk2, None, None


def apply_rope(q, k, positions, inv_freq):
    return _RopeFn.apply(q, k, positions, inv_freq)


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------
class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):
        C = _require_ext()
        ctx.save_for_backward(gate, up)
        return C.swiglu_fwd(gate.contiguous(), up.contiguous())

    @staticmethod
    def backward(ctx, dout):
        C = _require_ext()
        gate, up = ctx.saved_tensors
        dg, du = C.swiglu_bwd(dout.contiguous(), gate.contiguous(),
                              up.contiguous())
        return dg, du


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    if not _on_gpu(gate):
        return ref.swiglu(gate, up)
    if torch.is_grad_enabled() and (gate.requires_grad or up.requires_grad):
        return _SwiGLUFn.apply(gate, up)
    return _require_ext().swiglu_fwd(gate.contiguous(), up.contiguous())


def swiglu_fused(gate_up: torch.Tensor) -> torch.Tensor:
    """silu(gu[..., :I]) * gu[..., I:] on the fused gate_up GEMM output
    (inference path — avoids two .contiguous() splits)."""
    if not _on_gpu(gate_up):
        I = gate_up.shape[-1] // 2
        return ref.swiglu(gate_up[..., :I], gate_up[..., I:])
    return _require_ext().swiglu_fused(gate_up.contiguous())


# ---------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------
def attention_prefill(q, k, v, causal: bool = True,
                      scale: Optional[float] = None,
                      q_off: int = 0) -> torch.Tensor:
    """q [B,Sq,Hq,D], k/v [B,Skv,Hkv,D] -> [B,Sq,Hq,D]. Inference path.
    q_off: query row i is at global position q_off+i (chunked prefill).
    k/v may be views with any batch/token/head strides (D contiguous)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    if not _on_gpu(q):
        return ref.attention_prefill(q, k, v, causal, scale, q_off)
    if (q.shape[1] >= 4096 and q_off == 0 and causal
            and q.shape[1] == k.shape[1]):
        # long-context full prefill: ROCm flash SDPA measured faster
        # than the hand-written kernel at S >= 4k (376 vs 259 TF,
        # profiles/ r1); chunked/q_off windows stay on the HIP kernel
        out = torch.nn.functional.scaled_dot_product_attention(
            q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
            is_causal=True, scale=scale, enable_gqa=True)
        return out.transpose(1, 2)
    # k/v go in as strided views when their last dim is contiguous (the
    # permuted KV cache): the kernel reads them in place. TL_NO_PREFILL_V3=1
    # (read per call, in the binding) runs the v2 kernel on copies.
    if k.stride(-1) != 1:
        k = k.contiguous()
    if v.stride(-1) != 1:
        v = v.contiguous()
    return _require_ext().prefill_attn(q.contiguous(), k, v, scale, causal,
                                       q_off)


# incremented whenever the carried-state kernel handles a chunk (same
# purpose as gemm_dispatch_count: a silent fallback to torch math cannot
# pass as kernel coverage)
attn_carry_dispatch_count = 0


class AttnCarry:
    """The online-softmax state :func:`attention_prefill_carry` carries
    between key chunks, fp32, updated in place: ``o`` [B,Sq,Hq,D] is the
    unnormalised accumulator, ``ml`` [B,Hq,Sq,2] the (max, sum) pair per
    row."""

    __slots__ = ("o", "ml")

    def __init__(self, o: torch.Tensor, ml: torch.Tensor):
        self.o = o
        self.ml = ml

    @classmethod
    def empty(cls, q: torch.Tensor) -> "AttnCarry":
        """Uninitialised state for q [B,Sq,Hq,D]; the ``first`` call does
        not read it."""
        B, Sq, Hq, D = q.shape
        return cls(torch.empty(B, Sq, Hq, D, dtype=torch.float32,
                               device=q.device),
                   torch.empty(B, Hq, Sq, 2, dtype=torch.float32,
                               device=q.device))


def attention_prefill_carry(q, k, v, carry: AttnCarry, *, causal: bool,
                            q_off: int = 0, scale: Optional[float] = None,
                            first: bool, last: bool):
    """Attention of q [B,Sq,Hq,D] over ONE key chunk k/v [B,Skv,Hkv,D] of a
    longer key sequence, with the online-softmax state in ``carry``. The
    state is not read when ``first`` and is updated in place unless
    ``last``; the ``last`` call returns the normalised [B,Sq,Hq,D] output,
    the others None. With ``causal``, key j of this chunk is visible to
    query row i when j <= q_off + i. Chunks may come in any order; in
    ascending order with boundaries on multiples of 64 keys the result is
    bit-identical to one prefill kernel call over the concatenation.
    GPU bf16 at head dim 64 / 128 runs the carried-state prefill kernel,
    everything else the fp32 reference."""
    global attn_carry_dispatch_count
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    if (q.is_cuda and q.dtype == torch.bfloat16
            and q.shape[-1] in (64, 128)):
        C = _require_ext()        # a missing kernel is an error, not a
        if k.stride(-1) != 1:     # reason to run torch math on the GPU
            k = k.contiguous()
        if v.stride(-1) != 1:
            v = v.contiguous()
        attn_carry_dispatch_count += 1
        return C.prefill_attn_carry(q.contiguous(), k, v, carry.o, carry.ml,
                                    scale, causal, q_off, first, last)
    return ref.attention_prefill_carry(q, k, v, carry.o, carry.ml, causal,
                                       scale, q_off, first, last)


class _FlashAttnFn(torch.autograd.Function):
    """Hand-written flash attention for training (gfx950): forward =
    prefill kernel saving the logsumexp; backward = the two MFMA kernels
    in ops/csrc/flash_bwd.hip (dKV over key tiles, dQ over query tiles)
    with Delta = rowsum(dO*O) precomputed in fp32."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale):
        C = _require_ext()
        out, lse = C.prefill_attn_lse(q.contiguous(), k.contiguous(),
                                      v.contiguous(), scale, causal)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.causal = causal
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        C = _require_ext()
        q, k, v, out, lse = ctx.saved_tensors
        delta = (dout.float() * out.float()).sum(-1)          # [B,S,Hq]
        delta = delta.permute(0, 2, 1).contiguous()           # [B,Hq,S]
        dq, dk, dv = C.attn_bwd(q.contiguous(), k.contiguous(),
                                v.contiguous(), dout.contiguous(), lse,
                                delta, ctx.scale, ctx.causal)
        return dq, dk, dv, None, None


def attention_train(q, k, v, causal: bool = True,
                    scale: Optional[float] = None) -> torch.Tensor:
    """Training attention with autograd. GPU bf16 runs the hand-written
    flash forward+backward kernels; CPU (and unsupported head dims)
    composes torch SDPA."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if (q.is_cuda and q.dtype == torch.bfloat16 and _C is not None
            and D in (64, 128) and k.shape[1] == S):
        return _FlashAttnFn.apply(q, k, v, causal, scale)
    qt = q.transpose(1, 2)
    kt = k.transpose(1, 2)
    vt = v.transpose(1, 2)
    try:
        out = torch.nn.functional.scaled_dot_product_attention(
            qt, kt, vt, is_causal=causal, scale=scale, enable_gqa=True)
    except (TypeError, RuntimeError):
        # older torch / unsupported backend: materialize repeated heads
        rep = Hq // Hkv
        out = torch.nn.functional.scaled_dot_product_attention(
            qt, kt.repeat_interleave(rep, dim=1),
            vt.repeat_interleave(rep, dim=1), is_causal=causal, scale=scale)
    return out.transpose(1, 2)


def attention_decode(q, k_cache, v_cache, seq_lens,
                     scale: Optional[float] = None, n_split: int = 0,
                     block_table: Optional[torch.Tensor] = None,
                     len_add: int = 0) -> torch.Tensor:
    """q [B,1,Hq,D] or [B,Hq,D]; caches [B,Hkv,Smax,D] (or paged pools +
    block_table); seq_lens [B]. n_split: flash-decode splits (0 = auto).
    Row b attends to its first seq_lens[b] + len_add keys; len_add is
    added in-kernel, sparing the caller a per-layer tensor add."""
    squeeze = q.dim() == 4
    if squeeze:
        q3 = q.squeeze(1)
    else:
        q3 = q
    scale = scale if scale is not None else 1.0 / math.sqrt(q3.shape[-1])
    if not _on_gpu(q3):
        if len_add:
            seq_lens = seq_lens + len_add
        if block_table is not None:
            # gather pages -> contiguous [B, L, Hkv, D] for the reference
            B = q3.shape[0]
            L = int(seq_lens.max())
            np_ = (L + 127) // 128
            idx = block_table[:, :np_].long()
            kc = k_cache[idx].permute(0, 1, 3, 2, 4)
            vc = v_cache[idx].permute(0, 1, 3, 2, 4)
            kc = kc.reshape(B, np_ * 128, *kc.shape[3:])[:, :L]
            vc = vc.reshape(B, np_ * 128, *vc.shape[3:])[:, :L]
            out = ref.attention_decode(q3.unsqueeze(1), kc, vc, seq_lens,
                                       scale)
        else:
            out = ref.attention_decode(q3.unsqueeze(1),
                                       k_cache.permute(0, 2, 1, 3),
                                       v_cache.permute(0, 2, 1, 3),
                                       seq_lens, scale)
        return out if squeeze else out.squeeze(1)
    out = _require_ext().decode_attn(
        q3.contiguous(), k_cache, v_cache, seq_lens.int(), scale, n_split,
        block_table.int() if block_table is not None else None, len_add)
    return out.unsqueeze(1) if squeeze else out


# ---------------------------------------------------------------------------
# Linear (hand-written serving GEMM family)
# ---------------------------------------------------------------------------
import os as _os

# Inference GEMMs at M <= this route to the deterministic MFMA family
# (streaming kernel at M<=64, tiled all-glds kernel above). The family
# guarantees bitwise M-INDEPENDENT per-row results (same K chunk order,
# same (N,K)-only split policy), which is what makes chunked prefill /
# speculative verify / ragged batch decode / plain generate emit
# identical greedy tokens. Above the threshold (large prefill) hipBLASLt
# wins on throughput and exact cross-path equality is not claimed.
GEMM_M_MAX = int(_os.environ.get("TL_GEMM_M_MAX", "512"))

# incremented whenever the hand-written family handles a linear — GPU
# tests assert on it so a silent hipBLASLt fallback cannot pass as
# kernel coverage
gemm_dispatch_count = 0


# (N,K)-pure shape classes; TL_GEMM_LIB_CLASSES routes whole classes to
# hipBLASLt for in-pipeline A/B (a class flips for ALL M at once, so the
# bitwise M-independence guarantee is preserved per process).
# default: empty — every class runs the hand-written family. The gateup
# class (16k <= N < 64k), where the BN=64/256 structures lost ~40 us to
# the library (profiles/gemm_family_ab.md), takes the column-balanced
# one-pass kernel (gemm_colbal.hip) at 65 <= M <= GEMM_M_MAX: one
# workgroup per CU, 9-10 column tiles each, same K chain as the family and
# so the same bits as skinny_gemm at every M (profiles/gemm_colbal.md).
# TL_GEMM_LIB_CLASSES=gateup restores the library route.
_LIB_CLASSES = frozenset(
    c for c in _os.environ.get("TL_GEMM_LIB_CLASSES", "").split(",") if c)


def _gemm_class(N: int, K: int) -> str:
    # "wide" is TL_GEMM_WIDE_N in ops/csrc/gemm_policy.hpp: keep them equal
    if N >= 65536:
        return "wide"
    if N >= 16384:
        return "gateup"
    if K >= 8192:
        return "deepk"
    return "narrow"


def _use_tl_gemm(M: int, N: int, K: int) -> bool:
    return (K % 32 == 0 and N % 64 == 0 and M <= GEMM_M_MAX
            and _gemm_class(N, K) not in _LIB_CLASSES)


_n_split_cache = {}


def _use_colbal(M: int, N: int, K: int) -> bool:
    """The column-balanced kernel's domain: the gateup class at 65 <= M <=
    GEMM_M_MAX where the family's policy does not split K (always, at the
    default split target). TL_NO_COLBAL=1 keeps the class on skinny_gemm
    (same bits) for A/B runs and tests; read per call."""
    if not (65 <= M and _use_tl_gemm(M, N, K)
            and _gemm_class(N, K) == "gateup"
            and not _os.environ.get("TL_NO_COLBAL")):
        return False
    ns = _n_split_cache.get((N, K))
    if ns is None:
        ns = _n_split_cache[(N, K)] = _require_ext().gemm_n_split(N, K)
    return ns == 1


def _family_input(x: torch.Tensor) -> bool:
    return (x.is_cuda and not torch.is_grad_enabled()
            and x.dtype == torch.bfloat16
            and not _os.environ.get("TL_NO_SKINNY"))


def linear(x: torch.Tensor, weight: torch.Tensor,
           bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x @ W^T + bias. Serving-M shapes route to the hand-written MFMA
    family (skinny_gemm.hip / gemm_tiled.hip / gemm_colbal.hip); large
    prefill M and training go to torch/hipBLASLt."""
    global gemm_dispatch_count
    if _family_input(x):
        K = x.shape[-1]
        M = x.numel() // K
        N = weight.shape[0]
        if bias is None and _use_colbal(M, N, K):
            gemm_dispatch_count += 1
            return _require_ext().gemm_colbal(x.contiguous(), weight)
        if _use_tl_gemm(M, N, K):
            gemm_dispatch_count += 1
            return _require_ext().skinny_gemm(
                x.contiguous(), weight,
                bias.to(torch.bfloat16) if bias is not None else None)
    return torch.nn.functional.linear(x, weight, bias)


def gate_up_swiglu(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """swiglu_fused(linear(x, weight)) for a fused gate_up weight [2I, K]
    (gate rows, then up rows), [.., I]. In the column-balanced kernel's
    domain the activation is applied to the accumulators (gemm_colbal.hip,
    fused variant): no [M, 2I] round trip, no second kernel, same bits.
    TL_NO_GATEUP_FUSION=1 keeps the two-kernel chain (read per call)."""
    global gemm_dispatch_count
    if _family_input(x) and not _os.environ.get("TL_NO_GATEUP_FUSION"):
        K = x.shape[-1]
        M = x.numel() // K
        if _use_colbal(M, weight.shape[0], K):
            gemm_dispatch_count += 1
            return _require_ext().gemm_colbal_swiglu(x.contiguous(), weight)
    return swiglu_fused(linear(x, weight))


# incremented whenever head_argmax.hip picks the tokens (same purpose as
# gemm_dispatch_count: a silent fallback cannot pass as kernel coverage)
head_argmax_dispatch_count = 0

# Rows from which the fused head is routed. Below, the fallback's GEMM is
# the streaming kernel, which does not pay for a 256-row tile and beats the
# fused pair at M <= 32 (329 vs 256-323 us); M = 48 is a tie within the
# spread, M = 64 the first measured win (profiles/head_argmax.md).
HEAD_ARGMAX_M_MIN = 64


def _use_head_argmax(M: int, N: int, K: int) -> bool:
    """The fused greedy head's domain: the wide class, in the family's M
    range from HEAD_ARGMAX_M_MIN up, where the policy does not split K
    (always, at the default split target). TL_NO_HEAD_FUSION=1 keeps the
    GEMM + argmax pair (same tokens) for A/B runs and tests; read per
    call."""
    if not (HEAD_ARGMAX_M_MIN <= M and _use_tl_gemm(M, N, K)
            and _gemm_class(N, K) == "wide"
            and not _os.environ.get("TL_NO_HEAD_FUSION")):
        return False
    ns = _n_split_cache.get((N, K))
    if ns is None:
        ns = _n_split_cache[(N, K)] = _require_ext().gemm_n_split(N, K)
    return ns == 1


def linear_argmax(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """linear(x, weight).argmax(-1), int64 [..]: the greedy head. In the
    fused kernel's domain (head_argmax.hip) the [.., N] logits are never
    written and the tokens are the same, because every logit there is one
    K chain with the family's bits. Everything else — CPU, other dtypes,
    grad enabled, other widths, M outside the routed range — takes the
    two-step form."""
    global head_argmax_dispatch_count
    if _family_input(x):
        K = x.shape[-1]
        M = x.numel() // K
        if _use_head_argmax(M, weight.shape[0], K):
            head_argmax_dispatch_count += 1
            return _require_ext().lm_head_argmax(x.contiguous(), weight)
    return linear(x, weight).argmax(-1)


def decode_fusion_enabled() -> bool:
    """False under TL_NO_DECODE_FUSION=1: the decoder then runs the
    unfused chain (every GEMM reduces its own partials, the residual adds
    are separate kernels) — same bits, kept for A/B runs and tests. Read
    per call so a test can flip it."""
    return not _os.environ.get("TL_NO_DECODE_FUSION")


def linear_partials(x: torch.Tensor, weight: torch.Tensor,
                    bias: Optional[torch.Tensor] = None):
    """:func:`linear` for a caller whose next kernel can consume split-K
    partials: where the hand-written family would split K, returns
    :class:`Partials` and skips the reduce pass; everywhere else (other
    devices/dtypes, M above GEMM_M_MAX, library-routed classes, n_split
    == 1) returns :func:`linear`'s tensor."""
    global gemm_dispatch_count
    if _family_input(x):
        K = x.shape[-1]
        M = x.numel() // K
        N = weight.shape[0]
        if _use_tl_gemm(M, N, K):
            gemm_dispatch_count += 1
            b = bias.to(torch.bfloat16) if bias is not None else None
            out = _require_ext().skinny_gemm_partials(x.contiguous(),
                                                      weight, b)
            if out.dtype == torch.float32:
                return Partials(out, b)
            return out
    return linear(x, weight, bias)


# ---------------------------------------------------------------------------
# MXFP4 weight-only linear
# ---------------------------------------------------------------------------
# incremented whenever mxfp4_gemm.hip handles a linear (same purpose as
# gemm_dispatch_count: a silent fallback cannot pass as kernel coverage)
mxfp4_dispatch_count = 0


def _use_mxfp4_gemm(M: int, N: int, K: int) -> bool:
    # 512 is the binding's own row limit: a raised TL_GEMM_M_MAX must
    # not turn into an error there
    return (N > 0 and N % 64 == 0 and K > 0 and K % 128 == 0
            and 1 <= M <= min(GEMM_M_MAX, 512))


def mxfp4_linear(x: torch.Tensor, packed: torch.Tensor,
                 exponents: torch.Tensor,
                 bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x @ dequant(packed, exponents)^T + bias for MXFP4 weights as
    models.quant.quantize_mxfp4 emits them (packed [N, K/2] uint8,
    exponents [N, K/32] int8). GPU bf16 rows at serving M run the
    hand-written weight-only kernel (ops/csrc/mxfp4_gemm.hip): bitwise
    M-independent rows, hipGraph-capturable, no dequantized copy. Other
    GPU inputs dequantize once to bf16 (exact) and use F.linear; CPU runs
    the fp32 reference."""
    global mxfp4_dispatch_count
    if not _on_gpu(x):
        return ref.mxfp4_linear(x, packed, exponents, bias)
    K = x.shape[-1]
    M = x.numel() // K if K else 0
    N = packed.shape[0]
    if (x.dtype == torch.bfloat16 and _C is not None
            and _use_mxfp4_gemm(M, N, K)):
        mxfp4_dispatch_count += 1
        return _C.mxfp4_gemm(
            x.contiguous(), packed.contiguous(), exponents.contiguous(),
            bias.to(torch.bfloat16).contiguous()
            if bias is not None else None)
    w = ref.dequantize_mxfp4(packed, exponents, dtype=torch.bfloat16)
    return torch.nn.functional.linear(
        x, w.to(x.dtype), bias.to(x.dtype) if bias is not None else None)


# incremented whenever mxfp4_moe_gemm.hip handles a grouped expert GEMM
# (same purpose as mxfp4_dispatch_count)
mxfp4_moe_dispatch_count = 0


def mxfp4_moe_gemm(x: torch.Tensor, tok_idx: Optional[torch.Tensor],
                   seg_off: torch.Tensor, p_ptrs: torch.Tensor,
                   e_ptrs: torch.Tensor, N: int) -> torch.Tensor:
    """Grouped MXFP4 expert GEMM (ops/csrc/mxfp4_moe_gemm.hip), GPU only:
    out[p] = x[tok_idx[p]] @ dequant(packed_e, exponents_e)^T for the pair
    rows p of segment e = [seg_off[e], seg_off[e+1]). x bf16 [T, K] (or
    [P, K] with tok_idx None); tok_idx [P] and seg_off [E+1] int32;
    p_ptrs / e_ptrs [E] int64 device addresses of each expert's packed
    [N, K/2] uint8 and exponents [N, K/32] int8, 16-byte aligned and
    contiguous. Needs N % 64 == 0 and K % 128 == 0. One launch, no host
    sync, hipGraph-capturable; a pair's row is bitwise independent of the
    rest of the call. The CPU contract is
    ops.reference.mxfp4_moe_grouped."""
    global mxfp4_moe_dispatch_count
    out = _require_ext().mxfp4_moe_gemm(x, tok_idx, seg_off, p_ptrs, e_ptrs,
                                        N)
    mxfp4_moe_dispatch_count += 1
    return out


# ---------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------
def adamw_(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor,
           exp_avg_sq: torch.Tensor, *, lr: float, beta1: float = 0.9,
           beta2: float = 0.999, eps: float = 1e-8,
           weight_decay: float = 0.0, step: int = 1) -> None:
    if not _on_gpu(param):
        ref.adamw_step(param, grad, exp_avg, exp_avg_sq, lr=lr, beta1=beta1,
                       beta2=beta2, eps=eps, weight_decay=weight_decay,
                       step=step)
        return
    _require_ext().adamw_(param, grad.contiguous(), exp_avg, exp_avg_sq, lr,
                          beta1, beta2, eps, weight_decay, step)


# ---------------------------------------------------------------------------
# Sampling
# ---------------------------------------------------------------------------
def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    return x ^ (x >> 31)


def request_seed(seed: int, step: int) -> int:
    """Per-draw seed for a seeded request: depends only on (seed, step),
    so a request's samples are reproducible wherever it is batched.
    Returned as a signed 63-bit value (torch.long seeds tensor)."""
    return _splitmix64((seed & (2 ** 63 - 1)) ^ (step * 0xA24BAED4963EE407)) \
        & (2 ** 63 - 1)


def sample_tokens(logits: torch.Tensor, *, temps, top_ps, top_ks, pres,
                  freqs, counts: Optional[torch.Tensor] = None,
                  seeds: Optional[torch.Tensor] = None,
                  counter: Optional[torch.Tensor] = None,
                  seed_base: int = 0) -> torch.Tensor:
    """Batched fused sampling (ops/csrc/sampling.hip): penalties +
    temperature + top-k + top-p + draw, one kernel, graph-capture-safe.
    logits [B, V] bf16 on GPU; per-row param tensors; counts [B, V] i32
    is read for penalties and the chosen token's count is incremented."""
    C = _require_ext()
    return C.sample_tokens(logits.contiguous(), temps, top_ps, top_ks,
                           pres, freqs, counts, seeds, counter, seed_base)


def sample_token(logits, *, temperature=1.0, top_p=1.0, top_k=0,
                 generator=None, token_counts=None,
                 presence_penalty=0.0, frequency_penalty=0.0):
    """Single-request sampling with the reference (torch) semantics.
    The serving engine's hot path uses :func:`sample_tokens`; this stays
    torch-composed for API parity (dict token_counts, torch.Generator)
    and for greedy argmax."""
    return ref.sample_token(logits, temperature=temperature, top_p=top_p,
                            top_k=top_k, generator=generator,
                            token_counts=token_counts,
                            presence_penalty=presence_penalty,
                            frequency_penalty=frequency_penalty)


moe_topk_router = ref.moe_topk_router
causal_lm_loss = ref.causal_lm_loss
rope_cos_sin = ref.rope_cos_sin


# ---------------------------------------------------------------------------
# Fused linear cross-entropy (training loss head, ops/csrc/head_ce.hip)
# ---------------------------------------------------------------------------
# incremented whenever head_ce.hip computes a training loss (same purpose as
# gemm_dispatch_count: a silent fallback cannot pass as kernel coverage)
fused_ce_dispatch_count = 0


class _LinearCEFn(torch.autograd.Function):
    """Mean cross-entropy of hidden @ weight^T against labels without the
    logits. Forward is one pass of the stats kernel over all rows (bf16
    MFMA, f32 accumulators used unrounded) and a torch sum; nothing syncs
    the host. Backward walks the rows in chunks: the gradient kernel
    recomputes a chunk's logits and writes g = dloss/dlogits in bf16, two
    bf16 library GEMMs turn it into dh and the chunk's share of dW.

    Peak extra memory in backward: one g chunk (chunk * V * 2 B, 1.25 GB at
    4096 x 152064), dh (N * H * 2 B), and with more than one chunk the fp32
    dW accumulator plus one chunk's fp32 share (2 * V * H * 4 B, 4.4 GB at
    the Qwen2.5-7B head); with a single chunk dW comes straight out of the
    GEMM in the weight's dtype. Forward holds the stats scratch (39 MB at
    that vocabulary) and two fp32 vectors of N."""

    @staticmethod
    def forward(ctx, hidden, weight, labels, chunk):
        C = _require_ext()
        hidden = hidden.contiguous()
        weight = weight.contiguous()
        lse, loss_row = C.head_ce_stats(hidden, weight, labels)
        valid = (labels >= 0) & (labels < weight.shape[0])
        ctx.save_for_backward(hidden, weight, labels, lse)
        ctx.chunk = chunk
        return loss_row.sum() / valid.sum().clamp(min=1)

    @staticmethod
    def backward(ctx, dloss):
        C = _require_ext()
        hidden, weight, labels, lse = ctx.saved_tensors
        N = hidden.shape[0]
        chunk = ctx.chunk
        valid = (labels >= 0) & (labels < weight.shape[0])
        # exact +0 for ignored rows: the kernel turns it into zero bits
        scale = torch.where(valid, dloss.float() / valid.sum().clamp(min=1),
                            0.0)
        need_dh, need_dw = ctx.needs_input_grad[:2]
        dh = torch.empty_like(hidden) if need_dh else None
        dw = None
        single = N <= chunk
        for s in range(0, N, chunk):
            e = min(s + chunk, N)
            g = C.head_ce_grad(hidden[s:e], weight, labels[s:e], lse[s:e],
                               scale[s:e])
            if need_dh:
                torch.mm(g, weight, out=dh[s:e])
            if not need_dw:
                continue
            if single:
                dw = torch.mm(g.t(), hidden[s:e])
            elif dw is None:
                dw = torch.mm(g.t(), hidden[s:e], out_dtype=torch.float32)
            else:
                dw += torch.mm(g.t(), hidden[s:e], out_dtype=torch.float32)
        if dw is not None:
            dw = dw.to(weight.dtype)
        return dh, dw, None, None


def linear_cross_entropy(hidden: torch.Tensor, weight: torch.Tensor,
                         labels: torch.Tensor, ignore_index: int = -100,
                         chunk: int = 4096) -> torch.Tensor:
    """Mean over valid rows of cross_entropy(hidden @ weight^T, labels) as
    a scalar fp32, on the fused kernels (see :class:`_LinearCEFn`): hidden
    [N, H] and weight [V, H] bf16 on the GPU with H % 32 == 0, labels [N]
    int64. A row whose label equals ``ignore_index`` or lies outside
    [0, V) is ignored; with no valid row the loss is 0. ``chunk`` is the
    number of rows per backward step. No host sync, so the forward can be
    captured in a graph."""
    labels = labels.long()
    if ignore_index >= 0:
        labels = torch.where(labels == ignore_index, -100, labels)
    return _LinearCEFn.apply(hidden, weight, labels.contiguous(), chunk)


def _use_fused_ce(hidden: torch.Tensor, weight: torch.Tensor) -> bool:
    """The fused loss head's domain: bf16 operands on the GPU, H % 32 == 0,
    extension loaded. TL_NO_FUSED_CE=1 keeps the torch route for A/B runs
    and tests; read per call."""
    return (hidden.is_cuda and weight.is_cuda
            and hidden.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16 and _C is not None
            and hidden.shape[-1] % 32 == 0
            and not _os.environ.get("TL_NO_FUSED_CE"))


def chunked_causal_lm_loss(hidden: torch.Tensor, head_weight: torch.Tensor,
                           labels: torch.Tensor, chunk: int = 1024,
                           ignore_index: int = -100) -> torch.Tensor:
    """Shifted CE loss from the pre-head hidden states, hidden [B,S,H],
    labels [B,S]: the mean over the valid shifted positions. In the fused
    kernels' domain (:func:`_use_fused_ce`) it is
    :func:`linear_cross_entropy` over all B*S rows, each sequence's last
    position carrying -100, which spares the copy a slice of hidden would
    make; ``chunk`` then has no part (the fused backward uses its own
    default). Everything else is ops.reference.chunked_causal_lm_loss,
    unchanged."""
    global fused_ce_dispatch_count
    if not _use_fused_ce(hidden, head_weight):
        return ref.chunked_causal_lm_loss(hidden, head_weight, labels, chunk,
                                          ignore_index)
    fused_ce_dispatch_count += 1
    B, S, H = hidden.shape
    lb = torch.full_like(labels, -100)
    lb[:, :-1] = labels[:, 1:]
    return linear_cross_entropy(hidden.reshape(B * S, H), head_weight,
                                lb.reshape(-1), ignore_index)
