"""CPU tier of the fused cross-entropy suite (docs/TESTING.md, "Fused
cross-entropy"): the oracles of tests/fused_ce_oracle.py against torch, the
torch emulation of the kernels' contract against the rule and the exact
check the GPU tier applies, the mutants that both must reject, and the
dispatcher's CPU route, which must not move by a bit."""

import pytest
import torch
import torch.nn.functional as F

import fused_ce_oracle as fo
import kernel_oracle as ko

OUTPUTS = ("lse", "loss_row", "g", "dh", "dW")
# the mutants' cases: two panels with a partial last one, a K tail, two row
# blocks (a mutant that needs none of these shows on them all the same)
MUTANT_CASES = [(272, 160, 257), (777, 96, 300)]


@pytest.mark.parametrize("V,K,M", [(16, 32, 1), (16, 32, 5), (272, 96, 13),
                                   (777, 160, 24)])
def test_fp64_oracle_equals_torch(V, K, M):
    c = fo.ce_case(V, K, M)
    x = c["x"].double().requires_grad_()
    w = c["w"].double().requires_grad_()
    r = fo.reference(c)
    logits = x @ w.t()
    n_valid = int(fo._valid(c["labels"], V).sum())
    if n_valid == 0:
        # F.cross_entropy's mean over no row is NaN; the op gives 0
        assert float(r["loss"]) == 0.0 and not r["g"].any()
        return
    loss = F.cross_entropy(logits, c["labels"], ignore_index=-100)
    rows = F.cross_entropy(logits, c["labels"], ignore_index=-100,
                           reduction="none")
    logits.retain_grad()
    loss.backward()
    torch.testing.assert_close(r["loss"], loss.detach(), rtol=1e-13, atol=0)
    torch.testing.assert_close(r["loss_row"], rows.detach(), rtol=1e-13,
                               atol=1e-13)
    torch.testing.assert_close(r["lse"], logits.detach().logsumexp(-1),
                               rtol=1e-14, atol=0)
    torch.testing.assert_close(r["g"], logits.grad, rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(r["dh"], x.grad, rtol=1e-11, atol=1e-14)
    torch.testing.assert_close(r["dW"], w.grad, rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("V", fo.VS)
@pytest.mark.parametrize("K", fo.KS)
def test_inputs_meet_their_conditions(V, K):
    for M in fo.MS:
        c = fo.ce_case(V, K, M)
        n_dom = fo.check_mass(V, K, M)
        assert n_dom >= (M - 4) // 4 - 1
        assert (c["labels"] == -100).any()
        if M >= 12:
            r64 = fo.reference(c)
            assert abs(float(r64["lse"][fo.ZERO_ROW]) - torch.tensor(
                float(V)).log().item()) < 1e-6
            assert 70 < float(r64["lse"][fo.BIG_POS]) < 95
            assert -90 < float(r64["lse"][fo.BIG_NEG]) < -65
            assert float(r64["lse"][fo.HUGE_POS]) > 95
            assert float(r64["lse"][fo.HUGE_NEG]) < -90
    # the boundary label columns are all used
    c = fo.ce_case(V, K, 300)
    assert set(fo.boundary_columns(V)) <= set(c["labels"].tolist())


@pytest.mark.parametrize("V", fo.VS)
@pytest.mark.parametrize("K", fo.KS)
def test_panel_emulation_meets_rule_and_exact_check(V, K):
    for M in fo.MS:
        out = fo.panel_emulation(fo.ce_case(V, K, M))
        for name in OUTPUTS:
            r = fo.ratio(name, out[name], V, K, M)
            assert r <= 1.0, (name, V, K, M, r)
        c, lse, loss_row = fo.exact_case(V, K, M)
        assert fo.exact_ok(fo.panel_emulation(c), lse, loss_row), (V, K, M)


def test_exact_cases_cover_every_boundary_column():
    """Over the case list every boundary column is the boosted class of a
    k in the K tail and of one outside it."""
    for V in fo.VS:
        seen_tail, seen_body = set(), set()
        for K in fo.KS:
            c, _, _ = fo.exact_case(V, K, 300)
            w = c["w"].float()
            for col, k in (w == 64).nonzero().tolist():
                (seen_tail if k >= K - 32 else seen_body).add(col)
        assert seen_tail == set(fo.boundary_columns(V)), (V, seen_tail)
        if V > 16:
            assert seen_body == set(fo.boundary_columns(V)), (V, seen_body)


# which mutants the exact check must catch: those that change lse or the
# label logit of a one-hot row. A sum without the max subtraction is exact
# there (exp(64) is finite), merging without rescaling adds terms below
# 2^-24, and the other two leave lse and loss_row of valid rows alone.
EXACT_APPLIES = {"ghost_columns": True, "k_tail_dropped": True,
                 "label_off_by_one": True, "ignored_row_counts": True,
                 "no_max_subtraction": False, "merge_without_rescale": False,
                 "scale_by_all_rows": False}


@pytest.mark.parametrize("mutant", fo.MUTANTS)
def test_mutants_are_rejected(mutant):
    for V, K, M in MUTANT_CASES:
        out = fo.panel_emulation(fo.ce_case(V, K, M), mutant)
        ratios = {n: fo.ratio(n, out[n], V, K, M) for n in OUTPUTS}
        worst = max(ratios, key=ratios.get)
        print(f"CONF mutant {mutant} V{V} K{K} M{M}: {worst} at "
              f"{ratios[worst]:.1f} x tol")
        assert ratios[worst] >= 2.0, (mutant, V, K, M, ratios)
        if EXACT_APPLIES[mutant]:
            c, lse, loss_row = fo.exact_case(V, K, M)
            assert not fo.exact_ok(fo.panel_emulation(c, mutant), lse,
                                   loss_row), (mutant, V, K, M)


def test_dispatcher_cpu_route_is_the_reference_bit_for_bit():
    from tensorlink_amd import ops
    from tensorlink_amd.ops import reference as ref
    torch.manual_seed(5)
    B, S, H, V = 3, 9, 32, 50
    labels = torch.randint(0, V, (B, S))
    labels[1, 4] = -100
    before = ops.fused_ce_dispatch_count
    for dtype in (torch.float32, torch.bfloat16):
        grads = []
        for fn in (ops.chunked_causal_lm_loss, ref.chunked_causal_lm_loss):
            torch.manual_seed(6)
            h = torch.randn(B, S, H).to(dtype).requires_grad_()
            w = torch.randn(V, H).to(dtype).requires_grad_()
            loss = fn(h, w, labels, chunk=7)
            loss.backward()
            grads.append((loss.detach(), h.grad, w.grad))
        for a, b in zip(*grads):
            assert a.dtype == b.dtype and torch.equal(a, b)
    assert ops.fused_ce_dispatch_count == before


def test_linear_cross_entropy_is_public():
    from tensorlink_amd import ops
    assert callable(ops.linear_cross_entropy)
    assert isinstance(ops.fused_ce_dispatch_count, int)
