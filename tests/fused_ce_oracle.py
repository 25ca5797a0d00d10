"""Oracles, emulations and input builders for the fused linear
cross-entropy (ops/csrc/head_ce.hip; docs/TESTING.md, "Fused
cross-entropy"). Torch only: the CPU tier (tests/test_fused_ce_cpu.py)
checks the oracles and shows that wrong variants are rejected, the GPU tier
(tests/test_fused_ce_gpu.py) runs the kernels through the same inputs,
metric and tolerance (kernel_oracle.nme / kernel_oracle.tolerance).

The operation: logits = x @ W^T (x [M, K], W [V, K] bf16), labels [M]
int64, a row being ignored when its label lies outside [0, V);
    lse[i]      = logsumexp(logits[i])
    loss_row[i] = lse[i] - logits[i, label_i]          (0 if ignored)
    loss        = sum(loss_row) / max(n_valid, 1)
    g[i, c]     = (softmax(logits[i])[c] - (c == label_i)) * dloss / n_valid
                  (0 if ignored)
    dh = g @ W,  dW = g^T @ x
"""

from __future__ import annotations

import functools
from typing import Dict, Optional

import torch

import kernel_oracle as ko

F64 = torch.float64
BF16 = torch.bfloat16

VS = (16, 256, 272, 777)     # one partial panel; one full; 16 real + 240
                             # ghosts in a second; no multiple of 16
KS = (32, 96, 160, 256)      # tail alone; after one chunk; after two; none
MS = (1, 255, 256, 257, 300)  # one row block .. two blocks

# row roles, by index (a role a case is too short for is simply absent)
ZERO_ROW = 2                 # x row all zero: lse = log V
BIG_POS, BIG_NEG = 3, 6      # logits near +80 / -80
HUGE_POS, HUGE_NEG = 10, 11  # logits near +100 / -100: past fp32 exp range
DOMINANT_SHARE = 0.30        # least softmax mass of column V-1, dominant rows
LOGIT_STD = 1.5              # "a spread of a few units"

MUTANTS = ("ghost_columns", "k_tail_dropped", "label_off_by_one",
           "no_max_subtraction", "merge_without_rescale", "ignored_row_counts",
           "scale_by_all_rows")


def boundary_columns(V: int):
    return sorted({c for c in (0, 63, 64, 255, 256, V - 1) if 0 <= c < V})


def is_ignored(i: int, M: int) -> bool:
    return i % 4 == 1 or i == M - 1


def is_dominant(i: int, M: int) -> bool:
    return i >= 4 and i % 4 == 0 and not is_ignored(i, M)


@functools.lru_cache(maxsize=None)
def ce_case(V: int, K: int, M: int) -> Dict[str, torch.Tensor]:
    """bf16 inputs with every edge in them (docs/TESTING.md, "Fused
    cross-entropy": boundary labels, ignored rows, dominant last column,
    large logits of both signs, an all-zero row). W column 0 is 1 for
    every class, so x[i, 0] shifts all of row i's logits at once (0 for
    ordinary rows). Callers must not modify the tensors."""
    gen = torch.Generator().manual_seed(1000003 * V + 1009 * K + M)
    w = torch.randn(V, K, generator=gen) * (LOGIT_STD / K ** 0.5)
    w[:, 0] = 1.0
    w = w.to(BF16)
    x = torch.randn(M, K, generator=gen)
    x[:, 0] = 0.0
    wl = w[V - 1].float().clone()
    wl[0] = 0.0
    labels = torch.randint(0, V, (M,), generator=gen)
    cols = boundary_columns(V)
    n_lab = 0
    for i in range(M):
        if is_dominant(i, M):
            # aligned with W row V-1: that logit leads by about 10
            x[i] = 0.5 * x[i] + wl * (10.0 / float(wl.pow(2).sum()))
        if is_ignored(i, M):
            labels[i] = -100
        elif n_lab < 2 * len(cols):
            labels[i] = cols[n_lab % len(cols)]
            n_lab += 1
    if M > ZERO_ROW:
        x[ZERO_ROW] = 0.0
    for row, shift in ((BIG_POS, 80.0), (BIG_NEG, -80.0),
                       (HUGE_POS, 100.0), (HUGE_NEG, -100.0)):
        if M > row:
            x[row, 0] = shift
    return {"x": x.to(BF16), "w": w, "labels": labels, "V": V, "K": K,
            "M": M}


def _valid(labels: torch.Tensor, V: int) -> torch.Tensor:
    return (labels >= 0) & (labels < V)


def reference(c, dtype=F64, faithful: bool = False,
              dloss: float = 1.0) -> Dict[str, torch.Tensor]:
    """The operation in ``dtype``. float64: the oracle. float32: the torch
    route's math. float32 with ``faithful``: the bf16-faithful emulation
    (g rounded to bf16 before the two GEMMs, dh and dW rounded to bf16)."""
    x, w, labels = c["x"].to(dtype), c["w"].to(dtype), c["labels"]
    M, V = x.shape[0], w.shape[0]
    logits = x @ w.t()
    lse = torch.logsumexp(logits, -1)
    valid = _valid(labels, V)
    safe = labels.clamp(0, V - 1)
    tgt = logits.gather(1, safe[:, None])[:, 0]
    loss_row = torch.where(valid, lse - tgt, torch.zeros_like(lse))
    n_valid = max(int(valid.sum()), 1)
    p = (logits - lse[:, None]).exp()
    p[torch.arange(M), safe] -= valid.to(dtype)
    g = p * (valid.to(dtype) * (dloss / n_valid))[:, None]
    if faithful:
        g = ko.bf16_round(g)
    dh, dw = g @ w, g.t() @ x
    if faithful:
        dh, dw = ko.bf16_round(dh), ko.bf16_round(dw)
    return {"lse": lse, "loss_row": loss_row, "loss": loss_row.sum() / n_valid,
            "g": g, "dh": dh, "dW": dw}


def panel_emulation(c, mutant: Optional[str] = None,
                    dloss: float = 1.0) -> Dict[str, torch.Tensor]:
    """The kernels' contract in torch: fp32 logits from the bf16 operands,
    per 256-column panel (m, s) over the real columns, the panels merged in
    ascending order against the global max, g rounded to bf16 once, dh and
    dW from bf16 GEMMs. ``mutant`` names one deliberate error (MUTANTS)."""
    assert mutant is None or mutant in MUTANTS, mutant
    x, w, labels = c["x"].float(), c["w"].float(), c["labels"]
    M, V, K = x.shape[0], w.shape[0], x.shape[1]
    if mutant == "k_tail_dropped":
        logits = x[:, :K - 32] @ w[:, :K - 32].t()
    else:
        logits = x @ w.t()
    ms, ss = [], []
    for p0 in range(0, V, 256):
        lp = logits[:, p0:min(p0 + 256, V)]
        if mutant == "ghost_columns" and lp.shape[1] < 256:
            # the clamped loads' duplicates of row V-1, counted
            lp = torch.cat([lp, lp[:, -1:].expand(M, 256 - lp.shape[1])], 1)
        m = lp.amax(-1)
        if mutant == "no_max_subtraction":
            m = torch.zeros_like(m)
        ms.append(m)
        ss.append((lp - m[:, None]).exp().sum(-1))
    top = torch.stack(ms).amax(0)
    s = torch.zeros_like(top)
    for m, sp in zip(ms, ss):
        if mutant == "merge_without_rescale":
            s = s + sp
        else:
            s = s + torch.where(m == top, sp, sp * (m - top).exp())
    lse = top + s.log()

    valid = _valid(labels, V)
    lab = labels
    if mutant == "ignored_row_counts":
        valid = torch.ones_like(valid)
    if mutant == "label_off_by_one":
        lab = torch.where(valid, (labels + 1) % V, labels)
    safe = lab.clamp(0, V - 1)
    tgt = logits.gather(1, safe[:, None])[:, 0]
    loss_row = torch.where(valid, lse - tgt, torch.zeros_like(lse))
    n = M if mutant == "scale_by_all_rows" else max(int(valid.sum()), 1)
    scale = valid.float() * (dloss / n)
    p = (logits - lse[:, None]).exp()
    p[torch.arange(M), safe] -= valid.float()
    g = p * scale[:, None]
    g = torch.where(scale[:, None] == 0, torch.zeros_like(g), g)
    g = ko.bf16_round(g)
    return {"lse": lse, "loss_row": loss_row,
            "loss": loss_row.sum() / max(int(valid.sum()), 1), "g": g,
            "dh": ko.bf16_round(g @ w), "dW": ko.bf16_round(g.t() @ x)}


@functools.lru_cache(maxsize=None)
def references(V: int, K: int, M: int):
    """(ref64, E0) of ce_case(V, K, M), computed once and shared. E0 per
    output, by the rule of docs/TESTING.md: lse and loss_row, each taken as
    one vector, from the fp32 reference's own error; g from the fp32
    reference rounded to bf16; dh and dW from the bf16-faithful emulation."""
    c = ce_case(V, K, M)
    r64 = reference(c)
    r32 = reference(c, torch.float32)
    rbf = reference(c, torch.float32, faithful=True)
    e0 = {"lse": ko.nme(r32["lse"], r64["lse"]),
          "loss_row": ko.nme(r32["loss_row"], r64["loss_row"]),
          "g": ko.nme(ko.bf16_round(r32["g"]), r64["g"]),
          "dh": ko.nme(rbf["dh"], r64["dh"]),
          "dW": ko.nme(rbf["dW"], r64["dW"])}
    return r64, e0


MARGINS = {"lse": ko.LSE_MARGIN, "loss_row": ko.LSE_MARGIN, "g": ko.MARGIN,
           "dh": ko.MARGIN, "dW": ko.MARGIN}


def ratio(name: str, out: torch.Tensor, V: int, K: int, M: int) -> float:
    """nme(out, ref64) / tol for output ``name`` of ce_case(V, K, M);
    the rule holds when it is <= 1. nme = 0 gives 0. A reference row that
    is identically zero (g and dh of an ignored row) must come out as
    zero: nme counts anything else there as infinite error."""
    r64, e0 = references(V, K, M)
    got = ko.nme(out.detach().float().cpu(), r64[name])
    tol = ko.tolerance(e0[name], MARGINS[name])
    if got == 0:
        return 0.0
    return got / tol if tol > 0 else float("inf")


def check_mass(V: int, K: int, M: int) -> int:
    """Condition on the inputs: in the fp64 reference W row V-1 holds at
    least DOMINANT_SHARE of the softmax mass of every dominant row (counting
    its 240-odd ghost duplicates would move lse by about log 241 there).
    Returns the number of dominant rows."""
    c = ce_case(V, K, M)
    logits = c["x"].to(F64) @ c["w"].to(F64).t()
    share = logits.softmax(-1)[:, V - 1]
    rows = [i for i in range(M) if is_dominant(i, M)]
    for i in rows:
        assert float(share[i]) >= DOMINANT_SHARE, (V, K, M, i, float(share[i]))
    return len(rows)


# --------------------------------------------------------------------------
# the exact check
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(V: int, K: int, M: int):
    """x row i is one-hot at k_i; W[c(k_i), k_i] = 64 and the rest of W lies
    in [-1, 1], so row i's logits are column k_i of W, exactly, and every
    term of its softmax sum but one is below 2^-24 of it: lse[i] must be
    64.0f and loss_row[i] must be 64 - float(W[label_i, k_i]), bit for bit
    (0.0f for an ignored row). Each k has ONE boosted class, chosen from the
    boundary columns by the position of k in the list, rotated with K so
    that the K of the list together put every boundary column on a k of
    the tail and on one outside it. Returns the case and the expected (lse, loss_row)."""
    gen = torch.Generator().manual_seed(7 * V + 3 * K + M)
    ks = sorted({k for k in (0, 31, 32, 63, 64, K - 32, K - 1) if 0 <= k < K})
    cols = boundary_columns(V)
    w = (torch.rand(V, K, generator=gen) * 2 - 1).to(BF16)
    boosted = {}
    rot = 2 * (KS.index(K) if K in KS else K // 32)
    for j, k in enumerate(ks):
        # counted from the end: the two k of the tail take 2 columns per
        # K of the list, 8 in all, which covers the 6 boundary columns
        boosted[k] = cols[(rot + len(ks) - 1 - j) % len(cols)]
        w[boosted[k], k] = 64.0
    x = torch.zeros(M, K)
    labels = torch.empty(M, dtype=torch.long)
    for i in range(M):
        x[i, ks[i % len(ks)]] = 1.0
        labels[i] = -100 if is_ignored(i, M) else cols[(i // 2) % len(cols)]
    lse = torch.full((M,), 64.0)
    loss_row = torch.zeros(M)
    for i in range(M):
        if labels[i] >= 0:
            loss_row[i] = 64.0 - float(w[labels[i], ks[i % len(ks)]])
    c = {"x": x.to(BF16), "w": w, "labels": labels, "V": V, "K": K, "M": M}
    return c, lse, loss_row


def exact_ok(c_out, lse: torch.Tensor, loss_row: torch.Tensor) -> bool:
    """Bitwise: compared as int32 images, so -0.0 is not 0.0 and no NaN
    compares equal by accident."""
    def bits(t):
        return t.detach().float().cpu().contiguous().view(torch.int32)
    return (torch.equal(bits(c_out["lse"]), bits(lse))
            and torch.equal(bits(c_out["loss_row"]), bits(loss_row)))
