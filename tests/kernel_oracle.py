"""float64 oracles, the error metric and the input builders of the kernel
conformance suite (docs/TESTING.md, "Kernel conformance").

A plain module, torch only: it runs on CPU and, in float64, on cuda. The
CPU tier (tests/test_kernel_oracle.py) checks the oracles themselves and
shows that deliberately wrong variants ("mutants") are rejected; the GPU
tier (tests/test_ops_conformance_gpu.py) runs the HIP kernels through the
same metric, inputs and tolerance.

Conventions
-----------
* Every oracle takes tensors of any float dtype and computes in
  ``dtype`` (float64 by default). ``dtype=torch.float32`` gives the fp32
  twin used for the bf16-faithful emulation.
* ``nme(out, ref64)`` is the one error metric, ``tolerance(E0)`` the one
  tolerance rule: ``tol = MARGIN * E0`` with E0 the nme of the emulation
  of the same op on the same inputs. Nothing in it comes from the code
  under test.
"""

from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

MARGIN = 4.0          # accumulation order, split recombination, fast exp
LSE_MARGIN = 16.0     # fp32 floor is tiny; fast log/exp cost a few ulps
PAGE = 128
F64 = torch.float64


# --------------------------------------------------------------------------
# metric and tolerance
# --------------------------------------------------------------------------
def nme(out: torch.Tensor, ref64: torch.Tensor,
        floor: Optional[float] = None) -> float:
    """max over rows of max|out - ref| / rms(ref row); a row is the
    last-dim vector.

    A reference row can be identically zero by construction (dq of the
    first causal query: one key, softmax gradient 0); the ratio is then
    undefined, and any nonzero output there counts as infinite error.
    Where that is not wanted the caller passes ``floor``, an rms below
    which rows are normalised by the floor instead (the backward test
    uses the rms of the whole gradient, its natural scale)."""
    r = ref64.to(F64)
    o = out.to(F64).to(r.device)
    assert o.shape == r.shape, (o.shape, r.shape)
    if not torch.isfinite(o).all():
        return float("inf")
    err = (o - r).abs().amax(-1)
    rms = r.pow(2).mean(-1).sqrt()
    den = rms.clamp_min(floor) if floor else rms
    ratio = torch.where(err == 0, torch.zeros_like(err), err / den)
    return float(ratio.max())


def tolerance(e0: float, margin: float = MARGIN) -> float:
    return margin * e0


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


# --------------------------------------------------------------------------
# attention
# --------------------------------------------------------------------------
def attention_masked(q, k, v, allowed, scale=None, dtype=F64,
                     round_p: bool = False):
    """GQA attention under an explicit mask.

    q [B,Sq,Hq,D], k/v [B,Skv,Hkv,D], allowed bool broadcastable to
    [B,1,Sq,Skv] (True = attend). Returns (out [B,Sq,Hq,D],
    lse [B,Hq,Sq]) in ``dtype``; lse is the natural-log logsumexp of the
    scaled scores. Masked keys get probability exactly 0, so poisoned
    (large finite) cache slots contribute 0 * V = 0.

    round_p: round the unnormalised probabilities exp(s - max) to bf16
    before P @ V and normalise by the unrounded row sum — the kernels
    pass P through LDS as bf16 and keep the row sum in fp32."""
    B, Sq, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    qf = q.to(dtype).transpose(1, 2)
    kf = k.to(dtype).transpose(1, 2).repeat_interleave(rep, dim=1)
    vf = v.to(dtype).transpose(1, 2).repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale       # [B,Hq,Sq,Skv]
    s = s.masked_fill(~allowed, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    e = torch.where(allowed.expand_as(e), e, torch.zeros_like(e))
    l = e.sum(-1, keepdim=True)
    if round_p:
        e = bf16_round(e)
    out = torch.matmul(e, vf) / l
    lse = (m + l.log()).squeeze(-1)
    return out.transpose(1, 2), lse


def prefill_mask(Sq: int, Skv: int, q_off: int = 0, causal: bool = True,
                 device=None) -> torch.Tensor:
    """[1,1,Sq,Skv]: query row i sits at global position q_off + i and
    attends keys <= its position; non-causal attends every key."""
    if not causal:
        return torch.ones(1, 1, Sq, Skv, dtype=torch.bool, device=device)
    rows = torch.arange(Sq, device=device).unsqueeze(1) + q_off
    cols = torch.arange(Skv, device=device).unsqueeze(0)
    return (cols <= rows).view(1, 1, Sq, Skv)


def attention_prefill(q, k, v, causal=True, scale=None, q_off=0, dtype=F64,
                      round_p=False):
    """(out, lse). Cache slack (Skv > q_off + Sq) is masked by causality."""
    mask = prefill_mask(q.shape[1], k.shape[1], q_off, causal, q.device)
    return attention_masked(q, k, v, mask, scale, dtype, round_p)


def decode_mask(lens: torch.Tensor, Smax: int) -> torch.Tensor:
    """[B,1,1,Smax]: key j of row b is attended iff j < lens[b]."""
    cols = torch.arange(Smax, device=lens.device)
    return (cols[None, :] < lens.long()[:, None]).view(-1, 1, 1, Smax)


def attention_decode(q, k_cache, v_cache, lens, scale=None, dtype=F64,
                     round_p=False, mask=None):
    """q [B,Hq,D]; caches [B,Hkv,Smax,D]; lens [B] -> out [B,Hq,D]."""
    if mask is None:
        mask = decode_mask(lens, k_cache.shape[2])
    out, _ = attention_masked(q.unsqueeze(1), k_cache.transpose(1, 2),
                              v_cache.transpose(1, 2), mask, scale, dtype,
                              round_p)
    return out[:, 0]


def gather_pages(pool: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """pool [n_pages,Hkv,PAGE,D], table [B,W] -> contiguous
    [B,Hkv,W*PAGE,D] (position p lives in page table[b, p // PAGE])."""
    B, W = table.shape
    g = pool[table.long()]                       # [B,W,Hkv,PAGE,D]
    g = g.permute(0, 2, 1, 3, 4)
    return g.reshape(B, pool.shape[1], W * PAGE, pool.shape[3]).contiguous()


def attention_backward(q, k, v, dout, causal=True, scale=None):
    """fp64 (out, dq, dk, dv) by autograd through attention_prefill."""
    q64 = q.detach().to(F64).requires_grad_(True)
    k64 = k.detach().to(F64).requires_grad_(True)
    v64 = v.detach().to(F64).requires_grad_(True)
    out, _ = attention_prefill(q64, k64, v64, causal, scale)
    out.backward(dout.to(F64))
    return out.detach(), q64.grad, k64.grad, v64.grad


def grad_floor(dq64: torch.Tensor, dk64: torch.Tensor) -> float:
    """nme floor for dq: the rms of the whole gradient, or of dk (same
    natural scale) where dq is identically zero (S = 1)."""
    r = float(dq64.pow(2).mean().sqrt())
    return r if r > 0 else float(dk64.pow(2).mean().sqrt())


def split_ranges(L: int, n_split: int) -> List[Tuple[int, int]]:
    """Key range of each flash-decode split: ceil(L / n_split) keys per
    split, later splits possibly empty."""
    per = (L + n_split - 1) // n_split
    return [(s * per, min(L, s * per + per)) for s in range(n_split)]


def auto_split(L: int) -> int:
    """Per-row automatic split count: doubles past every 1024 keys."""
    ns = 1
    while ns < 16 and L > 1024 * ns:
        ns <<= 1
    return ns


def boundary_keys(L: int, n_split: int = 1, paged: bool = False
                  ) -> List[int]:
    """Keys a decode/prefill kernel can get wrong at length L: tile edges,
    the last key, each split's first key and the one before it, each
    page's first and last slot — whichever exist."""
    ks = {0, 15, 16, 63, 64, 127, 128, L - 1}
    for b, e in split_ranges(L, n_split):
        if 0 < b < L:
            ks.update((b, b - 1))
    if paged:
        for p in range(0, L, PAGE):
            ks.update((p, min(p + PAGE, L) - 1))
    return sorted(x for x in ks if 0 <= x < L)


def weighted_attention_inputs(B, Sq, Skv, Hq, Hkv, D, chosen, n_other,
                              poison=None, share=0.02, gen=None,
                              dtype=torch.bfloat16):
    """Boundary-weighted q/k/v: randn plus a score boost on the chosen
    keys, so each of them holds a guaranteed share of the softmax mass.

    chosen: bool [B,Skv]; n_other [B]: the most unboosted keys any query
    of that batch row attends (sets the boost). Per (batch, kv head) a
    unit direction d: every query carries sqrt(D) along d, ordinary keys
    carry nothing along d (their scores stay ~N(0,1)), chosen keys carry
    t along d and a quarter of the usual randn, so their scaled score is
    t + N(0,1/16) for every head of the group. V rows at chosen keys get
    distinct O(1) offsets. The caller asserts the mass condition on the
    fp64 reference (min_key_mass).

    poison: bool [B,Skv] of slots no kernel may read. They get K = 50 x a
    boosted key (its score would swamp the row) and V = 1e4: finite, so
    a legitimate 0 * V stays 0."""
    G = Hq // Hkv
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    d = rn(B, Hkv, D)
    d = d / d.norm(dim=-1, keepdim=True)
    perp = lambda x, dd: x - (x * dd).sum(-1, keepdim=True) * dd
    n_ch = chosen.sum(-1).to(F64)                                # [B]
    assert float((share * 2 * n_ch).max()) < 0.9, "too many chosen keys"
    # ordinary keys weigh E[exp(N(0,1))] = e^0.5 each; a chosen key needs
    # e^t >= share * (n e^t + R). Twice that share, then e^(3/4) for the
    # N(0,1/16) spread over a few dozen keys and heads.
    R = n_other.to(F64).clamp_min(1.0) * math.exp(0.5)
    t = torch.log((2 * share * R / (1 - 2 * share * n_ch)).clamp_min(1.0))
    t = t + 0.75
    dq = d.repeat_interleave(G, dim=1)[:, None]                  # [B,1,Hq,D]
    q = perp(rn(B, Sq, Hq, D), dq) + math.sqrt(D) * dq
    dk = d[:, None]                                              # [B,1,Hkv,D]
    k_plain = perp(rn(B, Skv, Hkv, D), dk)
    k_boost = 0.25 * perp(rn(B, Skv, Hkv, D), dk) + t.view(B, 1, 1, 1) * dk
    ch = chosen.view(B, Skv, 1, 1)
    k = torch.where(ch, k_boost, k_plain)
    v = rn(B, Skv, Hkv, D)
    rank = (chosen.cumsum(-1) - 1).to(F64)
    offs = torch.where(chosen, -2.0 + 4.0 * rank /
                       (n_ch.view(B, 1) - 1).clamp_min(1.0),
                       torch.zeros_like(rank))
    v = v + offs.view(B, Skv, 1, 1)
    if poison is not None:
        po = poison.view(B, Skv, 1, 1)
        k = torch.where(po, 50.0 * k_boost, k)
        v = torch.where(po, torch.full_like(v, 1e4), v)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def min_key_mass(q, k, v, allowed, chosen, scale=None) -> float:
    """Smallest softmax mass any chosen key holds over the heads and
    queries that attend it (fp64). chosen bool [B,Skv]."""
    B, Sq, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    qf = q.to(F64).transpose(1, 2)
    kf = k.to(F64).transpose(1, 2).repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    s = s.masked_fill(~allowed, float("-inf"))
    p = s.softmax(-1)                                   # [B,Hq,Sq,Skv]
    sel = chosen.view(B, 1, 1, -1) & allowed.expand_as(p)
    return float(p[sel].min()) if bool(sel.any()) else 1.0


# --------------------------------------------------------------------------
# RoPE and RoPE + cache append
# --------------------------------------------------------------------------
def rope(x, positions, inv_freq, sign: float = 1.0, dtype=F64,
         pairing: str = "half"):
    """x [T,H,D], positions [T], inv_freq [D/2] fp32. The angle is
    pos * float64(inv_freq_fp32): the fp32 spectrum is the operator's
    definition, everything after it is exact. dtype=float32 computes the
    angle the way fp32 torch does (fp32 product, fp32 cos/sin).
    pairing "half" rotates (d, d + D/2); "adjacent" is the wrong one."""
    ang = positions.to(dtype)[:, None] * inv_freq.to(torch.float32).to(dtype)
    c = ang.cos()[:, None, :]
    s = ang.sin()[:, None, :] * sign
    xf = x.to(dtype)
    if pairing == "half":
        d2 = x.shape[-1] // 2
        x1, x2 = xf[..., :d2], xf[..., d2:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    x1, x2 = xf[..., 0::2], xf[..., 1::2]
    return torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], -1).flatten(-2)


def rope_append(qkv, positions, inv_freq, S, Hq, Hkv, D,
                block_table=None, dtype=F64):
    """Reference of the fused rope + cache append.

    qkv [T,(Hq+2Hkv)*D] with T = B*S (q | k | v per row). Returns
    (q_rot [T,Hq,D], k_rot [T,Hkv,D], v [T,Hkv,D], rows [T], slots [T]):
    token t's rotated k and its v belong at cache[rows[t], :, slots[t]]
    — contiguous caches [B,Hkv,Smax,D]: row = batch, slot = position;
    page pools [n_pages,Hkv,PAGE,D] with block_table [B,W]: row =
    table[batch, pos // PAGE], slot = pos % PAGE. No other slot may
    change."""
    T = qkv.shape[0]
    q = qkv[:, :Hq * D].reshape(T, Hq, D)
    k = qkv[:, Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D)
    v = qkv[:, (Hq + Hkv) * D:].reshape(T, Hkv, D)
    pos = positions.long()
    batch = torch.arange(T, device=pos.device) // S
    if block_table is None:
        rows, slots = batch, pos
    else:
        rows = block_table.long()[batch, pos // PAGE]
        slots = pos % PAGE
    return (rope(q, positions, inv_freq, dtype=dtype),
            rope(k, positions, inv_freq, dtype=dtype), v.to(dtype), rows,
            slots)


# --------------------------------------------------------------------------
# RMSNorm, SwiGLU
# --------------------------------------------------------------------------
def rmsnorm(x, w, eps, dtype=F64, eps_outside: bool = False):
    xf = x.to(dtype)
    var = xf.pow(2).mean(-1, keepdim=True)
    r = 1.0 / (var.sqrt() + eps) if eps_outside else torch.rsqrt(var + eps)
    return xf * r * w.to(dtype)


def rmsnorm_residual(x, residual, w, eps, dtype=F64):
    """(y, r): r = x + residual is itself rounded to the storage dtype
    by the op, y is computed from the unrounded sum."""
    r = x.to(dtype) + residual.to(dtype)
    return rmsnorm(r, w, eps, dtype), r


def rmsnorm_backward(dy, x, w, eps):
    """fp64 (dx, dw) by autograd."""
    x64 = x.detach().to(F64).requires_grad_(True)
    w64 = w.detach().to(F64).requires_grad_(True)
    rmsnorm(x64, w64, eps).backward(dy.to(F64))
    return x64.grad, w64.grad


def swiglu(gate, up, dtype=F64):
    g = gate.to(dtype)
    return g * torch.sigmoid(g) * up.to(dtype)


def swiglu_backward(dout, gate, up):
    g = gate.detach().to(F64).requires_grad_(True)
    u = up.detach().to(F64).requires_grad_(True)
    swiglu(g, u).backward(dout.to(F64))
    return g.grad, u.grad


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------
def adamw_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step,
               use_wd: bool = True, bc2_under_sqrt: bool = True):
    """One AdamW step in float64, bias corrections in double. Returns
    new (param, m, v); inputs are not modified. The two flags produce
    the mutants."""
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    m = m * beta1 + (1 - beta1) * g
    v = v * beta2 + (1 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = ((v / bc2).sqrt() if bc2_under_sqrt else v.sqrt() / bc2) + eps
    wd = weight_decay if use_wd else 0.0
    p = p * (1 - lr * wd) - lr * (m / bc1) / denom
    return p, m, v


# --------------------------------------------------------------------------
# linear, grouped MoE
# --------------------------------------------------------------------------
def linear(x, w, bias=None, dtype=F64):
    y = x.to(dtype) @ w.to(dtype).t()
    return y + bias.to(dtype) if bias is not None else y


def moe_grouped(x, pair_tok, seg, weights: Sequence[torch.Tensor],
                scales: Optional[Sequence[torch.Tensor]] = None, dtype=F64,
                last_row_next_expert: bool = False):
    """out[p] = x[pair_tok[p]] @ W[e]^T (* scale[e]) for the pairs p in
    segment e = [seg[e], seg[e+1]). last_row_next_expert is the mutant."""
    E = len(weights)
    P = pair_tok.shape[0]
    N = weights[0].shape[0]
    out = torch.zeros(P, N, dtype=dtype, device=x.device)
    def rows_of(lo, hi, ew):
        y = x[pair_tok[lo:hi].long()].to(dtype) @ weights[ew].to(dtype).t()
        return y * scales[ew].to(dtype) if scales is not None else y

    for e in range(E):
        a, b = int(seg[e]), int(seg[e + 1])
        if b <= a:
            continue
        out[a:b] = rows_of(a, b, e)
        if last_row_next_expert:
            out[b - 1:b] = rows_of(b - 1, b, (e + 1) % E)
    return out


def e4m3_codes() -> torch.Tensor:
    """The 254 non-NaN fp8 e4m3fn byte codes."""
    c = torch.arange(256, dtype=torch.int32)
    return c[(c & 0x7F) != 0x7F].to(torch.uint8)


# --------------------------------------------------------------------------
# sampler
# --------------------------------------------------------------------------
_M64 = 2 ** 64 - 1


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def sampler_uniform(seeds: Sequence[int]) -> torch.Tensor:
    """u = float32((splitmix64(seed) >> 11) * 2^-53) per row, as fp64."""
    u = [(splitmix64(int(s) & _M64) >> 11) * 2.0 ** -53 for s in seeds]
    return torch.tensor(u, dtype=F64).to(torch.float32).to(F64)


def sampler_kept(z: torch.Tensor, T: torch.Tensor, top_k: torch.Tensor,
                 top_p: torch.Tensor, p_of_total: bool = False
                 ) -> torch.Tensor:
    """Kept set [B,V] with ops.reference.sample_token's semantics: mask
    to the top k first (value ties kept), then top-p over the
    renormalised survivors: a token stays while the mass strictly above
    it is <= p. Value ties at the p cut are kept together.
    p_of_total takes the p mass over all tokens instead (the mutant)."""
    B, V = z.shape
    z = z.to(F64)
    kept = torch.ones_like(z, dtype=torch.bool)
    k = top_k.long().view(B, 1)
    use_k = (k > 0) & (k < V)
    srt = z.sort(-1, descending=True).values
    kth = srt.gather(1, (k.clamp(1, V) - 1))
    kept = torch.where(use_k, z >= kth, kept)
    p = top_p.to(F64).view(B, 1)
    use_p = p < 1.0
    zt = z / T.to(F64).view(B, 1).clamp_min(1e-30)
    w = torch.exp(zt - zt.amax(-1, keepdim=True))
    base = w if p_of_total else torch.where(kept, w, torch.zeros_like(w))
    wk = torch.where(kept, w, torch.zeros_like(w))
    order = z.argsort(dim=-1, descending=True, stable=True)
    ws = wk.gather(1, order)
    zs = z.gather(1, order)
    excl = ws.cumsum(-1) - ws
    ok = excl <= p * base.sum(-1, keepdim=True)
    ok = ok & (ws > 0)
    # lowest kept value; ties with it stay
    thr = torch.where(ok, zs, torch.full_like(zs, float("inf"))).amin(
        -1, keepdim=True)
    kept = torch.where(use_p, kept & (z >= thr), kept)
    return kept


def penalized_logits(logits, counts, pres, freqs) -> torch.Tensor:
    """fp32, as the kernel forms them: z - (pres + freqs * count) where
    count > 0."""
    z = logits.to(torch.float32)
    if counts is None:
        return z
    c = counts.to(torch.float32)
    pen = pres.to(torch.float32).view(-1, 1) \
        + freqs.to(torch.float32).view(-1, 1) * c
    return torch.where(counts > 0, z - pen, z)


def sample_oracle(logits, temps, top_ks, top_ps, seeds, counts=None,
                  pres=None, freqs=None, edge: float = 1e-5,
                  p_of_total: bool = False):
    """Expected tokens [B] of the fused sampler and an ``excluded`` bool
    [B] of rows whose draw lies within edge*S of an interval edge (the
    fp32 scan of the kernel may legitimately land on the neighbour).

    Greedy (T <= 0): first-index argmax. Sampled: fp64 weights
    exp((z - max)/T) over the kept set in index order; the token is the
    first kept index whose inclusive cumulative weight is >= u*S."""
    logits = logits.detach().cpu()
    B, V = logits.shape
    cpu = lambda t: None if t is None else t.detach().cpu()
    temps, top_ks, top_ps = cpu(temps), cpu(top_ks), cpu(top_ps)
    z32 = penalized_logits(logits, cpu(counts),
                           cpu(pres) if pres is not None else None,
                           cpu(freqs) if freqs is not None else None)
    z = z32.to(F64)
    greedy = temps <= 0
    Tsafe = torch.where(greedy, torch.ones_like(temps), temps)
    kept = sampler_kept(z, Tsafe, top_ks, top_ps, p_of_total)
    zt = z / Tsafe.to(F64).view(B, 1)
    w = torch.exp(zt - zt.amax(-1, keepdim=True))
    w = torch.where(kept, w, torch.zeros_like(w))
    cum = w.cumsum(-1)
    S = cum[:, -1:]
    u = sampler_uniform([int(s) for s in cpu(seeds)]).view(B, 1)
    target = u * S
    hit = (cum >= target) & (w > 0)
    first = torch.where(hit, torch.arange(V).expand(B, V),
                        torch.full((B, V), V)).amin(-1)
    last_kept = torch.where(w > 0, torch.arange(V).expand(B, V),
                            torch.full((B, V), -1)).amax(-1)
    tok = torch.where(first < V, first, last_kept)
    hi = cum.gather(1, tok.view(B, 1))
    lo = hi - w.gather(1, tok.view(B, 1))
    near = ((target - lo).abs() <= edge * S) | ((hi - target).abs() <= edge * S)
    tok = torch.where(greedy, z32.argmax(-1), tok)
    excluded = near.view(B) & ~greedy
    return tok, excluded


def distinct_bf16_logits(B: int, V: int, gen: torch.Generator,
                         std: float = 3.0) -> torch.Tensor:
    """[B,V] bf16 ~ N(0, std^2) with no two equal values in a row, so a
    top-k / top-p cut never falls inside a tie."""
    rows = []
    for _ in range(B):
        cand = (torch.randn(16 * V, generator=gen) * std).to(torch.bfloat16)
        uniq = torch.unique(cand.float())
        assert uniq.numel() >= V, (uniq.numel(), V)
        pick = uniq[torch.randperm(uniq.numel(), generator=gen)[:V]]
        rows.append(pick.to(torch.bfloat16))
    return torch.stack(rows)


def midpoint_top_p(logits, temps, top_ks, target: float = 0.8):
    """Per row, p halfway between two adjacent sorted cumulative
    probabilities (over the top-k survivors) nearest ``target``, so the
    cut is unambiguous. Returns (p [B] fp32, half_gap [B] fp64, Zn [B]):
    half_gap is the distance from p to either neighbour, Zn the survivors'
    mean weight in units of the largest weight."""
    B, V = logits.shape
    z = logits.detach().cpu().to(F64)
    T = temps.detach().cpu().to(F64).view(B, 1)
    kept = sampler_kept(z, T.view(B), top_ks.detach().cpu(),
                        torch.ones(B))
    zt = z / T
    w = torch.exp(zt - zt.amax(-1, keepdim=True))
    w = torch.where(kept, w, torch.zeros_like(w))
    Z = w.sum(-1)
    cum = (w.sort(-1, descending=True).values / Z.view(B, 1)).cumsum(-1)
    nk = kept.sum(-1)
    mid = (cum[:, :-1] + cum[:, 1:]) / 2
    valid = torch.arange(V - 1).expand(B, V - 1) < (nk.view(B, 1) - 1)
    dist = torch.where(valid, (mid - target).abs(),
                       torch.full_like(mid, float("inf")))
    j = dist.argmin(-1, keepdim=True)
    p = mid.gather(1, j).view(B)
    half = ((cum[:, 1:] - cum[:, :-1]) / 2).gather(1, j).view(B)
    return p.to(torch.float32), half, Z / nk.to(F64)


def attention_backward_emulated(q, k, v, dout, causal=True, scale=None):
    """bf16-faithful emulation of a flash backward: fp32 math, P and dS
    rounded to bf16 before the matrix products (they feed the matrix
    cores as bf16), gradients rounded to bf16. Returns (dq, dk, dv)."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    G = Hq // Hkv
    f32 = torch.float32
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    out, lse = attention_prefill(q, k, v, causal, scale, dtype=f32,
                                 round_p=True)
    out = bf16_round(out)
    mask = prefill_mask(S, S, 0, causal, q.device)
    qf = q.to(f32).transpose(1, 2)                              # [B,Hq,S,D]
    kf = k.to(f32).transpose(1, 2).repeat_interleave(G, dim=1)
    vf = v.to(f32).transpose(1, 2).repeat_interleave(G, dim=1)
    do = dout.to(f32).transpose(1, 2)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    p = torch.exp(s - lse.unsqueeze(-1))
    p = torch.where(mask.expand_as(p), p, torch.zeros_like(p))
    delta = (do * out.transpose(1, 2)).sum(-1, keepdim=True)
    dp = torch.matmul(do, vf.transpose(-1, -2))
    ds = bf16_round(p * (dp - delta))
    pb = bf16_round(p)
    dq = torch.matmul(ds, kf) * scale
    dk = torch.matmul(ds.transpose(-1, -2), qf) * scale
    dv = torch.matmul(pb.transpose(-1, -2), do)
    fold = lambda t: t.view(B, Hkv, G, S, D).sum(2)
    tr = lambda t: bf16_round(t.transpose(1, 2))
    return tr(dq), tr(fold(dk)), tr(fold(dv))


# --------------------------------------------------------------------------
# shared cases: the CPU mutants and the GPU kernels see the same inputs
# --------------------------------------------------------------------------
def decode_case(lens: Sequence[int], Smax: int, Hq: int, Hkv: int, D: int,
                splits: Optional[Sequence[int]] = None, paged: bool = False,
                seed: int = 0):
    """Boundary-weighted, poisoned decode inputs. splits: the split count
    whose boundaries get weight, per row (default: the automatic one).
    Returns q [B,Hq,D], kc/vc [B,Hkv,Smax,D], lens i32, chosen [B,Smax]."""
    gen = torch.Generator().manual_seed(seed)
    B = len(lens)
    splits = splits or [auto_split(L) for L in lens]
    chosen = torch.zeros(B, Smax, dtype=torch.bool)
    for b, L in enumerate(lens):
        chosen[b, boundary_keys(L, splits[b], paged)] = True
    lt = torch.tensor(list(lens))
    poison = torch.arange(Smax)[None, :] >= lt[:, None]
    q, k, v = weighted_attention_inputs(
        B, 1, Smax, Hq, Hkv, D, chosen, lt - chosen.sum(-1), poison=poison,
        gen=gen)
    return dict(q=q[:, 0].contiguous(), kc=k.transpose(1, 2).contiguous(),
                vc=v.transpose(1, 2).contiguous(),
                lens=lt.to(torch.int32), chosen=chosen)


def check_mass(q, k, v, allowed, chosen, share=0.02):
    """The input condition of the boundary-weighted cases."""
    got = min_key_mass(q, k, v, allowed, chosen)
    assert got >= share, f"a chosen key holds only {got:.4f} of the mass"


def check_decode_mass(case):
    check_mass(case["q"].unsqueeze(1), case["kc"].transpose(1, 2),
               case["vc"].transpose(1, 2),
               decode_mask(case["lens"], case["kc"].shape[2]),
               case["chosen"])


def decode_reference(case, mask=None):
    """(ref64, E0, tol) of a decode case."""
    ref = attention_decode(case["q"], case["kc"], case["vc"], case["lens"],
                           mask=mask)
    emu = bf16_round(attention_decode(case["q"], case["kc"], case["vc"],
                                      case["lens"], dtype=torch.float32,
                                      round_p=True))
    e0 = nme(emu, ref)
    return ref, e0, tolerance(e0)


def paged_case(lens: Sequence[int], width: int, n_pages: int, Hq: int,
               Hkv: int, D: int, seed: int = 0):
    """decode_case scattered into a page pool through a shuffled table.
    Unused table entries and unlisted pool pages are valid, fully
    poisoned pages. Adds pool_k/pool_v [n_pages,Hkv,PAGE,D], table [B,W],
    free_page (poisoned, in no row's live range)."""
    c = decode_case(lens, width * PAGE, Hq, Hkv, D, paged=True, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    B = len(lens)
    used = [(b, w) for b, L in enumerate(lens)
            for w in range((L + PAGE - 1) // PAGE)]
    assert len(used) < n_pages
    perm = torch.randperm(n_pages, generator=gen).tolist()
    free = perm[len(used):]
    table = torch.full((B, width), free[0], dtype=torch.int32)
    pk = torch.empty(n_pages, Hkv, PAGE, D, dtype=c["kc"].dtype)
    pv = torch.empty_like(pk)
    # a poisoned slab: any slot past a row's length
    b_p = min(range(B), key=lambda b: lens[b])
    w_p = width - 1
    assert lens[b_p] <= w_p * PAGE
    for pg in free:
        pk[pg] = c["kc"][b_p, :, w_p * PAGE:(w_p + 1) * PAGE]
        pv[pg] = c["vc"][b_p, :, w_p * PAGE:(w_p + 1) * PAGE]
    for (b, w), pg in zip(used, perm):
        table[b, w] = pg
        pk[pg] = c["kc"][b, :, w * PAGE:(w + 1) * PAGE]
        pv[pg] = c["vc"][b, :, w * PAGE:(w + 1) * PAGE]
    c.update(pool_k=pk, pool_v=pv, table=table, free_page=free[0])
    return c


def prefill_case(Sq: int, q_off: int, Skv: int, Hq: int, Hkv: int, D: int,
                 causal: bool = True, B: int = 1, seed: int = 0):
    """Boundary-weighted prefill inputs; keys past q_off + Sq (cache
    slack) are poisoned when causal. q [B,Sq,Hq,D], k/v [B,Skv,Hkv,D]."""
    gen = torch.Generator().manual_seed(seed)
    L = q_off + Sq if causal else Skv
    chosen = torch.zeros(B, Skv, dtype=torch.bool)
    chosen[:, boundary_keys(L)] = True
    poison = (torch.arange(Skv) >= L).expand(B, Skv)
    n_other = torch.full((B,), L) - chosen.sum(-1)
    q, k, v = weighted_attention_inputs(B, Sq, Skv, Hq, Hkv, D, chosen,
                                        n_other, poison=poison, gen=gen)
    return dict(q=q, k=k, v=v, q_off=q_off, causal=causal, chosen=chosen,
                mask=prefill_mask(Sq, Skv, q_off, causal))


def prefill_reference(case, mask=None):
    """(out64, lse64, E0_out, E0_lse) of a prefill case. ``mask``
    replaces the case's own mask in out64/lse64 (the mutants); E0 always
    belongs to the true operator."""
    true_out, true_lse = attention_masked(case["q"], case["k"], case["v"],
                                          case["mask"])
    emu, lse32 = attention_masked(case["q"], case["k"], case["v"],
                                  case["mask"], dtype=torch.float32,
                                  round_p=True)
    e0, e0_lse = nme(bf16_round(emu), true_out), nme(lse32, true_lse)
    if mask is None:
        return true_out, true_lse, e0, e0_lse
    out, lse = attention_masked(case["q"], case["k"], case["v"], mask)
    return out, lse, e0, e0_lse


def rope_case(D: int, theta: float, Hq: int = 4, Hkv: int = 2, seed: int = 0,
              positions: Sequence[int] = (0, 1, 4095, 32767, 131071)):
    gen = torch.Generator().manual_seed(seed)
    T = len(positions)
    q = torch.randn(T, Hq, D, generator=gen).to(torch.bfloat16)
    k = torch.randn(T, Hkv, D, generator=gen).to(torch.bfloat16)
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    return dict(q=q, k=k, pos=torch.tensor(list(positions),
                                           dtype=torch.int32), inv=inv)


def rope_reference(x, pos, inv):
    """(ref64, E0): E0 from the fp32 torch rope rounded to bf16."""
    ref = rope(x, pos, inv)
    e0 = nme(bf16_round(rope(x, pos, inv, dtype=torch.float32)), ref)
    return ref, e0


SAMPLER_CASES = ("T0.5", "T1.0", "T1.7", "topk", "topp", "topk_topp",
                 "penalties")


def sampler_case(name: str, V: int, B: int = 512, seed: int = 0):
    """Inputs of one fused-sampler conformance case (CPU tensors).
    Tie-free bf16 logits ~ N(0, 9); seeds b*7919+1."""
    gen = torch.Generator().manual_seed(seed * 1000 + V)
    logits = distinct_bf16_logits(B, V, gen)
    # top-k + top-p at T=1.7: the top 20 then hold well under the whole
    # mass, so taking p over all tokens instead of over the survivors
    # changes the drawn token in a third of the rows
    T = {"T0.5": 0.5, "T1.7": 1.7, "topk_topp": 1.7}.get(name, 1.0)
    c = dict(logits=logits, temps=torch.full((B,), T),
             top_ps=torch.ones(B), top_ks=torch.zeros(B, dtype=torch.int32),
             pres=torch.zeros(B), freqs=torch.zeros(B), counts=None,
             seeds=torch.arange(B, dtype=torch.int64) * 7919 + 1)
    if name in ("topk", "topk_topp"):
        c["top_ks"] = torch.full((B,), 20, dtype=torch.int32)
    if name in ("topp", "topk_topp"):
        p, half, Z = midpoint_top_p(logits, c["temps"], c["top_ks"])
        c.update(top_ps=p, half_gap=half, Zn=Z)
    if name == "penalties":
        cnt = torch.randint(0, 4, (B, V), generator=gen, dtype=torch.int32)
        cnt = cnt * (torch.rand(B, V, generator=gen) < 0.1)
        c.update(counts=cnt.to(torch.int32), pres=torch.full((B,), 0.8),
                 freqs=torch.full((B,), 0.5))
    return c


def check_top_p_cut(case, V: int):
    """Input condition of the top-p cases: the cut is unambiguous — p is
    further from both neighbouring cumulative probabilities than the
    kernel's 2^-20 fixed-point weights (one truncation per surviving
    token, relative to their sum) and the fp32 p can move it."""
    if "half_gap" not in case:
        return
    slack = 4 * (2.0 ** -20 / case["Zn"] + 2.0 ** -23)
    assert bool((case["half_gap"] >= slack).all()), \
        float((case["half_gap"] / slack).min())


def sampler_expected(case, **kw):
    return sample_oracle(case["logits"], case["temps"], case["top_ks"],
                         case["top_ps"], case["seeds"], case["counts"],
                         case["pres"], case["freqs"], **kw)


def rmsnorm_case(N: int, H: int, seed: int = 0):
    """bf16 rows, alternately scaled x100 and x1e-3 (the second makes
    mean(x^2) comparable to eps = 1e-5)."""
    gen = torch.Generator().manual_seed(seed + H)
    x = torch.randn(N, H, generator=gen)
    sc = torch.where(torch.arange(N) % 2 == 0, 100.0, 1e-3).view(N, 1)
    w = 1.0 + 0.5 * torch.randn(H, generator=gen)
    dy = torch.randn(N, H, generator=gen)
    return dict(x=(x * sc).to(torch.bfloat16), w=w.to(torch.bfloat16),
                dy=dy.to(torch.bfloat16), eps=1e-5)


ADAMW_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1)


def adamw_case(n: int, steps: int, seed: int = 0):
    gen = torch.Generator().manual_seed(seed + n)
    return dict(p=torch.randn(n, generator=gen),
                g=torch.randn(steps, n, generator=gen))


def adamw_run(case, steps: int, **flags):
    """fp64 oracle trajectory from zero moments: (p, m, v) after steps."""
    p = case["p"].to(F64)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    for s in range(1, steps + 1):
        p, m, v = adamw_step(p, case["g"][s - 1], m, v, step=s, **ADAMW_HP,
                             **flags)
    return p, m, v


def adamw_torch_fp32(case, steps: int):
    """torch.optim.AdamW on fp32 parameters: the E0 of the fp32 kernel."""
    p = case["p"].clone().float().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=ADAMW_HP["lr"],
                            betas=(ADAMW_HP["beta1"], ADAMW_HP["beta2"]),
                            eps=ADAMW_HP["eps"],
                            weight_decay=ADAMW_HP["weight_decay"])
    for s in range(steps):
        p.grad = case["g"][s].clone().float()
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


def gemm_case(M: int, N: int, K: int, bias: bool, seed: int = 0):
    gen = torch.Generator().manual_seed(seed + N + K)
    x = torch.randn(M, K, generator=gen).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=gen) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=gen).to(torch.bfloat16) if bias else None
    return dict(x=x, w=w, b=b)


def gemm_reference(case):
    ref = linear(case["x"], case["w"], case["b"])
    e0 = nme(bf16_round(linear(case["x"], case["w"], case["b"],
                               dtype=torch.float32)), ref)
    return ref, e0


MOE_SEGMENTS = (130, 64, 0, 6)


def moe_case(K: int, N: int = 128, T: int = 48, seed: int = 0):
    """Forced routing: expert-sorted pairs with segment sizes
    MOE_SEGMENTS (two 64-row chunks + tail, exactly one chunk, empty,
    short). weights are bf16 [N,K] per expert."""
    gen = torch.Generator().manual_seed(seed + K)
    E = len(MOE_SEGMENTS)
    P = sum(MOE_SEGMENTS)
    seg = torch.zeros(E + 1, dtype=torch.int32)
    seg[1:] = torch.tensor(MOE_SEGMENTS).cumsum(0)
    x = torch.randn(T, K, generator=gen).to(torch.bfloat16)
    ws = [(torch.randn(N, K, generator=gen) / K ** 0.5).to(torch.bfloat16)
          for _ in range(E)]
    tok = torch.randint(0, T, (P,), generator=gen, dtype=torch.int32)
    return dict(x=x, ws=ws, seg=seg, tok=tok, N=N)


def moe_reference(case, ws=None, scales=None):
    ws = ws if ws is not None else case["ws"]
    ref = moe_grouped(case["x"], case["tok"], case["seg"], ws, scales)
    e0 = nme(bf16_round(moe_grouped(case["x"], case["tok"], case["seg"], ws,
                                    scales, dtype=torch.float32)), ref)
    return ref, e0
