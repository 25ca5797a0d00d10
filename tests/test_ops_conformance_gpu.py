"""GPU tier of the kernel conformance suite (MI355X).

Every HIP kernel against the float64 oracle of the same operation
(tests/kernel_oracle.py), at the shapes and edges the kernels branch on,
through one metric and one tolerance rule:

    nme(out, ref64) <= MARGIN * E0

with E0 the nme of the bf16-faithful emulation of the op on the same
inputs, computed here. tests/test_kernel_oracle.py shows on CPU that
deliberately wrong kernels fail these same checks by 2x or more. Each
check prints its measured nme / E0 (``CONF`` lines, visible with -s);
docs/TESTING.md records them.
"""

import math

import pytest
import torch

import kernel_oracle as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16


def _ops():
    from tensorlink_amd import ops
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    return ops


def dev(t):
    return t.to(DEV) if isinstance(t, torch.Tensor) else t


def check(name, out, ref64, e0, margin=ko.MARGIN, floor=None):
    got = ko.nme(out.detach().cpu(), ref64.cpu(), floor)
    ratio = got / e0 if e0 > 0 else (0.0 if got == 0 else math.inf)
    print(f"CONF {name}: nme={got:.3e} E0={e0:.3e} nme/E0={ratio:.2f}")
    assert got <= ko.tolerance(e0, margin), \
        f"{name}: nme {got:.3e} > {margin:g} * E0 {e0:.3e}"


# --------------------------------------------------------------------------
# decode attention
# --------------------------------------------------------------------------
def _decode(c, **kw):
    return _ops().attention_decode(dev(c["q"]), dev(c["kc"]), dev(c["vc"]),
                                   dev(c["lens"]), **kw)


@pytest.mark.parametrize("Hq,Hkv,D", [(8, 2, 128), (14, 2, 128),
                                      (16, 1, 128), (8, 2, 64)])
def test_decode_mfma_tile_boundaries(Hq, Hkv, D):
    c = ko.decode_case([1, 15, 16, 17, 64, 65, 129, 160], 160, Hq, Hkv, D)
    ko.check_decode_mass(c)
    ref64, e0, _ = ko.decode_reference(c)
    check(f"decode_mfma Hq{Hq} Hkv{Hkv} D{D}", _decode(c), ref64, e0)


def test_decode_mfma_explicit_split_with_empty_splits():
    c = ko.decode_case([5, 130], 160, 8, 2, 128, splits=[4, 4], seed=1)
    ko.check_decode_mass(c)
    ref64, e0, _ = ko.decode_reference(c)
    check("decode_mfma n_split=4 L{5,130}", _decode(c, n_split=4), ref64, e0)


def test_decode_mfma_auto_split_boundaries():
    c = ko.decode_case([1024, 1025, 2048, 2049], 2100, 8, 2, 128, seed=2)
    ko.check_decode_mass(c)
    ref64, e0, _ = ko.decode_reference(c)
    check("decode_mfma auto split Smax2100", _decode(c), ref64, e0)


def test_decode_mfma_capacity_independence():
    """A row whose own split count is 1 gives the same bits through the
    direct-write kernel (Smax=512) and through the split kernel + combine
    (Smax=2048): the combine's f = exp(0) = 1 claim."""
    big = ko.decode_case([300], 2048, 8, 2, 128, seed=5)
    ko.check_decode_mass(big)
    small = dict(big, kc=big["kc"][:, :, :512].contiguous(),
                 vc=big["vc"][:, :, :512].contiguous())
    ref64, e0, _ = ko.decode_reference(small)
    o_small, o_big = _decode(small), _decode(big)
    check("decode_mfma L300 Smax512", o_small, ref64, e0)
    assert torch.equal(o_small, o_big)


def test_decode_mfma_paged_shuffled_table():
    ops = _ops()
    c = ko.paged_case([1, 128, 129, 300], 3, 8, 8, 2, 128, seed=3)
    ko.check_decode_mass(c)
    ref64, e0, _ = ko.decode_reference(c)
    out = ops.attention_decode(dev(c["q"]), dev(c["pool_k"]),
                               dev(c["pool_v"]), dev(c["lens"]),
                               block_table=dev(c["table"]))
    check("decode_mfma paged 8-page pool", out, ref64, e0)
    flat = ops.attention_decode(
        dev(c["q"]), dev(ko.gather_pages(c["pool_k"], c["table"])),
        dev(ko.gather_pages(c["pool_v"], c["table"])), dev(c["lens"]))
    assert torch.equal(out, flat)


def test_decode_legacy_kernel_group_18():
    """G = 18 > 16 routes to the legacy kernel; its last z-block covers
    gq = 2 heads."""
    c = ko.decode_case([1, 9, 33, 100], 112, 36, 2, 128, seed=6)
    ko.check_decode_mass(c)
    ref64, e0, _ = ko.decode_reference(c)
    check("decode_legacy G18", _decode(c), ref64, e0)


# --------------------------------------------------------------------------
# prefill attention
# --------------------------------------------------------------------------
def _prefill_check(name, c):
    ko.check_mass(c["q"], c["k"], c["v"], c["mask"], c["chosen"])
    out64, lse64, e0, e0_lse = ko.prefill_reference(c)
    out = _ops().attention_prefill(dev(c["q"]), dev(c["k"]), dev(c["v"]),
                                   causal=c["causal"], q_off=c["q_off"])
    check(name, out, out64, e0)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 129])
def test_prefill_causal(S, D):
    _prefill_check(f"prefill causal S{S} D{D}",
                   ko.prefill_case(S, 0, S, 4, 2, D, B=2, seed=10))


def test_prefill_causal_group_7():
    _prefill_check("prefill causal S65 G7",
                   ko.prefill_case(65, 0, 65, 14, 2, 128, seed=11))


@pytest.mark.parametrize("Sq,q_off,Skv", [(33, 31, 100), (1, 64, 128),
                                          (65, 63, 128)])
def test_prefill_q_off_with_cache_slack(Sq, q_off, Skv):
    _prefill_check(f"prefill Sq{Sq} q_off{q_off} Skv{Skv}",
                   ko.prefill_case(Sq, q_off, Skv, 8, 2, 128, seed=4))


@pytest.mark.parametrize("Sq,Skv,D,causal", [
    (1, 1, 128, True), (63, 63, 64, True), (65, 65, 128, True),
    (129, 129, 128, True), (129, 129, 64, True),
    (33, 64, 128, True),       # cache slack behind the last query
    (65, 65, 128, False)])
def test_prefill_lse_is_the_logsumexp(Sq, Skv, D, causal):
    """lse from prefill_attn_lse against the fp64 natural-log logsumexp
    of the scaled scores. E0 is the fp32 reference's own lse error and
    the margin 16: that floor is tiny and fast log/exp legitimately cost
    a few ulps."""
    C = _ops()._require_ext()
    c = ko.prefill_case(Sq, 0, Skv, 4, 2, D, causal=causal, seed=12)
    ko.check_mass(c["q"], c["k"], c["v"], c["mask"], c["chosen"])
    out64, lse64, e0, e0_lse = ko.prefill_reference(c)
    out, lse = C.prefill_attn_lse(dev(c["q"]), dev(c["k"]), dev(c["v"]),
                                  1.0 / math.sqrt(D), causal)
    name = f"prefill_lse Sq{Sq} Skv{Skv} D{D} causal{int(causal)}"
    check(name + " out", out, out64, e0)
    check(name + " lse", lse, lse64, e0_lse, margin=ko.LSE_MARGIN)


# --------------------------------------------------------------------------
# flash backward
# --------------------------------------------------------------------------
_BWD = [(S, G, D, True) for S in (1, 63, 65, 130) for G in (1, 4)
        for D in (64, 128)] + [(65, 4, 128, False)]


@pytest.mark.parametrize("S,G,D,causal", _BWD)
def test_flash_backward(S, G, D, causal):
    ops = _ops()
    Hkv = 2
    c = ko.prefill_case(S, 0, S, Hkv * G, Hkv, D, causal=causal, seed=20)
    ko.check_mass(c["q"], c["k"], c["v"], c["mask"], c["chosen"])
    gen = torch.Generator().manual_seed(21)
    dout = torch.randn(1, S, Hkv * G, D, generator=gen).to(BF16)
    out64, dq64, dk64, dv64 = ko.attention_backward(c["q"], c["k"], c["v"],
                                                    dout, causal)
    eq, ek, ev = ko.attention_backward_emulated(c["q"], c["k"], c["v"],
                                                dout, causal)
    q, k, v = (dev(c[n]).requires_grad_(True) for n in "qkv")
    out = ops.attention_train(q, k, v, causal=causal)
    assert "FlashAttn" in type(out.grad_fn).__name__
    out.backward(dev(dout))
    name = f"flash_bwd S{S} G{G} D{D} causal{int(causal)}"
    floor = ko.grad_floor(dq64, dk64)
    check(name + " dq", q.grad, dq64, ko.nme(eq, dq64, floor), floor=floor)
    check(name + " dk", k.grad, dk64, ko.nme(ek, dk64))
    check(name + " dv", v.grad, dv64, ko.nme(ev, dv64))


# --------------------------------------------------------------------------
# RoPE and RoPE + append
# --------------------------------------------------------------------------
def _check_rope_rows(name, got, x, c):
    """Per position: the largest angle must not hide behind the rest."""
    for i, p in enumerate(c["pos"].tolist()):
        ref64, e0 = ko.rope_reference(x[i:i + 1], c["pos"][i:i + 1],
                                      c["inv"])
        check(f"{name} pos{p}", got[i:i + 1], ref64, e0)


@pytest.mark.parametrize("theta", [1e4, 1e6])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_long_positions(D, theta):
    ops = _ops()
    c = ko.rope_case(D, theta, seed=30)
    q, k = dev(c["q"]).clone(), dev(c["k"]).clone()
    ops.apply_rope_(q, k, dev(c["pos"]), dev(c["inv"]))
    _check_rope_rows(f"rope D{D} theta{theta:g} q", q, c["q"], c)
    _check_rope_rows(f"rope D{D} theta{theta:g} k", k, c["k"], c)


SENTINEL = 0x3F9D      # a bf16 bit pattern (1.2265625) no output hits by plan


def _sentinel_cache(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16,
                      device=DEV).view(BF16)


def _check_append(name, c, S, Hq, Hkv, D, kc, vc, q_out, table=None):
    T = c["qkv"].shape[0]
    q64, k64, v64, rows, slots = ko.rope_append(
        c["qkv"], c["pos"], c["inv"], S, Hq, Hkv, D, table)
    q32, k32, *_ = ko.rope_append(c["qkv"], c["pos"], c["inv"], S, Hq, Hkv,
                                  D, table, dtype=torch.float32)
    for i, p in enumerate(c["pos"].tolist()):
        sl = slice(i, i + 1)
        check(f"{name} q pos{p}", q_out[sl], q64[sl],
              ko.nme(ko.bf16_round(q32[sl]), q64[sl]))
        check(f"{name} k pos{p}", kc[int(rows[i]), :, int(slots[i])][None],
              k64[sl],
              ko.nme(ko.bf16_round(k32[sl]), k64[sl]))
    # v is a copy: bit-exact
    got_v = vc[dev(rows), :, dev(slots)]
    assert torch.equal(got_v.cpu().double(), v64)
    # nothing but the written slots changed
    untouched = torch.ones(kc.shape[0], kc.shape[2], dtype=torch.bool,
                           device=DEV)
    untouched[dev(rows), dev(slots)] = False
    assert int(untouched.sum()) == untouched.numel() - T
    for cache in (kc, vc):
        bits = cache.view(torch.int16).permute(0, 2, 1, 3)[untouched]
        assert bool((bits == SENTINEL).all()), f"{name}: scribbled"


def _append_case(positions, Hq, Hkv, D, theta, seed):
    gen = torch.Generator().manual_seed(seed)
    T = len(positions)
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, generator=gen).to(BF16)
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    return dict(qkv=qkv, pos=torch.tensor(positions, dtype=torch.int32),
                inv=inv)


@pytest.mark.parametrize("theta", [1e4, 1e6])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_append_long_positions_and_sentinel(D, theta):
    ops = _ops()
    Hq, Hkv, S = 4, 2, 5
    c = _append_case([0, 1, 4095, 32767, 131071], Hq, Hkv, D, theta, 31)
    kc = _sentinel_cache(1, Hkv, 131072, D)
    vc = _sentinel_cache(1, Hkv, 131072, D)
    q_out = ops.rope_append_(dev(c["qkv"]), kc, vc, dev(c["pos"]),
                             dev(c["inv"]), S, Hq, Hkv)
    _check_append(f"rope_append D{D} theta{theta:g}", c, S, Hq, Hkv, D, kc,
                  vc, q_out)


def test_rope_append_paged_straddles_a_page():
    ops = _ops()
    Hq, Hkv, D, S = 4, 2, 128, 3
    c = _append_case([126, 127, 128, 127, 128, 129], Hq, Hkv, D, 1e4, 32)
    table = torch.tensor([[4, 1], [5, 2]], dtype=torch.int32)   # of 6 pages
    kc = _sentinel_cache(6, Hkv, ko.PAGE, D)
    vc = _sentinel_cache(6, Hkv, ko.PAGE, D)
    q_out = ops.rope_append_(dev(c["qkv"]), kc, vc, dev(c["pos"]),
                             dev(c["inv"]), S, Hq, Hkv,
                             block_table=dev(table))
    _check_append("rope_append paged", c, S, Hq, Hkv, D, kc, vc, q_out,
                  table)


# --------------------------------------------------------------------------
# RMSNorm
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,H", [(4, 8), (4, 64), (4, 128), (4, 2048),
                                 (1, 2048), (4, 2056), (4, 16384)])
def test_rmsnorm_forward(N, H):
    from tensorlink_amd.ops import reference as ref
    c = ko.rmsnorm_case(N, H)
    ref64 = ko.rmsnorm(c["x"], c["w"], c["eps"])
    e0 = ko.nme(ref.rmsnorm(c["x"], c["w"], c["eps"]), ref64)
    y = _ops().rmsnorm(dev(c["x"]), dev(c["w"]), c["eps"])
    check(f"rmsnorm N{N} H{H}", y, ref64, e0)


def test_rmsnorm_residual_2056():
    from tensorlink_amd.ops import reference as ref
    c = ko.rmsnorm_case(4, 2056, seed=1)
    res = ko.rmsnorm_case(4, 2056, seed=2)["x"]
    y64, r64 = ko.rmsnorm_residual(c["x"], res, c["w"], c["eps"])
    ye, re_ = ref.rmsnorm_residual(c["x"], res, c["w"], c["eps"])
    y, r = _ops().rmsnorm_residual(dev(c["x"]), dev(res), dev(c["w"]),
                                   c["eps"])
    check("rmsnorm_residual H2056 y", y, y64, ko.nme(ye, y64))
    check("rmsnorm_residual H2056 r", r, r64, ko.nme(re_, r64))


@pytest.mark.parametrize("H", [128, 2056])
def test_rmsnorm_backward_row_stride_loop(H):
    """N = 700 > 512 blocks: the row-stride loop and the 512-slab dw
    reduce both run."""
    ops = _ops()
    N = 700
    c = ko.rmsnorm_case(N, H, seed=3)
    dx64, dw64 = ko.rmsnorm_backward(c["dy"], c["x"], c["w"], c["eps"])
    x32 = c["x"].float().requires_grad_(True)
    w32 = c["w"].float().requires_grad_(True)
    ko.rmsnorm(x32, w32, c["eps"], dtype=torch.float32).backward(
        c["dy"].float())
    x = dev(c["x"]).requires_grad_(True)
    w = dev(c["w"]).requires_grad_(True)
    ops.rmsnorm(x, w, c["eps"]).backward(dev(c["dy"]))
    check(f"rmsnorm_bwd N{N} H{H} dx", x.grad, dx64,
          ko.nme(ko.bf16_round(x32.grad), dx64))
    check(f"rmsnorm_bwd N{N} H{H} dw", w.grad[None], dw64[None],
          ko.nme(ko.bf16_round(w32.grad)[None], dw64[None]))


def test_rmsnorm_rejects_unsupported_width():
    ops = _ops()
    C = ops._require_ext()
    H = 16392
    x = torch.randn(2, H, device=DEV, dtype=BF16)
    w = torch.ones(H, device=DEV, dtype=BF16)
    with pytest.raises(RuntimeError, match="16384"):
        ops.rmsnorm(x, w, 1e-5)
    with pytest.raises(RuntimeError, match="16384"):
        ops.rmsnorm_residual(x, x, w, 1e-5)
    with pytest.raises(RuntimeError, match="16384"):
        C.rmsnorm_bwd(x, x, w, torch.ones(2, device=DEV))


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------
ADAMW_MARKS = (1, 2, 10, 1000)
_adamw_cache = {}


def _adamw_population():
    """The n = 1025 trajectory: oracle, E0 and kernel results at every
    mark. E0 = torch.optim.AdamW on fp32 parameters against the oracle,
    taken over these 1025 elements: on 1, 3 or 5 elements it is a sample
    of that few rounding errors and lands near 0 by chance (2.6e-9 seen),
    which no fp32 kernel other than a bit-copy of torch's could meet. The
    short cases are prefixes of this data and are held to this E0."""
    if not _adamw_cache:
        ops = _ops()
        case = ko.adamw_case(1025, ADAMW_MARKS[-1])
        p = dev(case["p"]).clone()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        g = dev(case["g"])
        got, want, e0 = {}, {}, {}
        for s in range(1, ADAMW_MARKS[-1] + 1):
            ops.adamw_(p, g[s - 1], m, v, step=s, **ko.ADAMW_HP)
            if s in ADAMW_MARKS:
                got[s] = (p.clone(), m.clone(), v.clone())
                want[s] = ko.adamw_run(case, s)
                e0[s] = [ko.nme(a[None], b[None]) for a, b in
                         zip(ko.adamw_torch_fp32(case, s), want[s])]
        _adamw_cache.update(case=case, got=got, want=want, e0=e0)
    return _adamw_cache


@pytest.mark.parametrize("n", [1, 3, 5, 1025])
def test_adamw_fp32_params_moments_and_steps(n):
    """fp32 template against the fp64 oracle after 1, 2, 10 and 1000
    steps; param, exp_avg and exp_avg_sq. n = 1, 3, 5 run the kernel on
    the first n elements of the n = 1025 data (the VEC = 4 tail paths):
    the same metric and E0, and bit-equal to the long run's prefix."""
    ops = _ops()
    pop = _adamw_population()
    if n == 1025:
        got = pop["got"]
    else:
        case = pop["case"]
        p = dev(case["p"][:n]).clone()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        g = dev(case["g"][:, :n]).contiguous()
        got = {}
        for s in range(1, ADAMW_MARKS[-1] + 1):
            ops.adamw_(p, g[s - 1], m, v, step=s, **ko.ADAMW_HP)
            if s in ADAMW_MARKS:
                got[s] = (p.clone(), m.clone(), v.clone())
    for s in ADAMW_MARKS:
        for i, nm in enumerate(("p", "m", "v")):
            check(f"adamw fp32 n{n} step{s} {nm}", got[s][i][None],
                  pop["want"][s][i][:n][None], pop["e0"][s][i])
            assert torch.equal(got[s][i], pop["got"][s][i][:n])


@pytest.mark.parametrize("n", [1, 3, 5, 1025])
def test_adamw_bf16_single_step_within_one_ulp(n):
    ops = _ops()
    gen = torch.Generator().manual_seed(40 + n)
    p0 = torch.randn(n, generator=gen).to(BF16)
    g = torch.randn(n, generator=gen).to(BF16)
    m0 = torch.randn(n, generator=gen) * 0.1
    v0 = torch.rand(n, generator=gen) * 0.01
    want, m64, v64 = ko.adamw_step(p0, g, m0, v0, step=7, **ko.ADAMW_HP)
    want = want.to(BF16).double()
    p, m, v = dev(p0).clone(), dev(m0).clone(), dev(v0).clone()
    ops.adamw_(p, dev(g), m, v, step=7, **ko.ADAMW_HP)
    ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want).exponent - 8)
    diff = (p.cpu().double() - want).abs()
    print(f"CONF adamw bf16 n{n}: max diff {float((diff / ulp).max()):.2f} ulp")
    assert bool((diff <= ulp).all())
    # the moments are fp32: E0 from the fp32 reference of the op
    from tensorlink_amd.ops import reference as ref
    pe, me, ve = p0.clone(), m0.clone(), v0.clone()
    ref.adamw_step(pe, g, me, ve, step=7, **ko.ADAMW_HP)
    check(f"adamw bf16 n{n} m", m[None], m64[None],
          ko.nme(me[None], m64[None]))
    check(f"adamw bf16 n{n} v", v[None], v64[None],
          ko.nme(ve[None], v64[None]))


# --------------------------------------------------------------------------
# sampling
# --------------------------------------------------------------------------
def _sample(c):
    return _ops().sample_tokens(
        dev(c["logits"]), temps=dev(c["temps"]), top_ps=dev(c["top_ps"]),
        top_ks=dev(c["top_ks"]), pres=dev(c["pres"]), freqs=dev(c["freqs"]),
        counts=c.get("counts_dev"), seeds=dev(c["seeds"]))


@pytest.mark.parametrize("V", [300, 1000])
@pytest.mark.parametrize("name", ko.SAMPLER_CASES)
def test_sampler_token_exact(name, V):
    """512 rows, every draw equal to the oracle's token; rows whose draw
    sits within 1e-5*S of an interval edge are excluded, at most 2 %."""
    c = ko.sampler_case(name, V)
    ko.check_top_p_cut(c, V)
    want, excluded = ko.sampler_expected(c)
    assert float(excluded.float().mean()) <= 0.02
    if c["counts"] is not None:
        c["counts_dev"] = dev(c["counts"]).clone()
    got = _sample(c).cpu()
    keep = ~excluded
    wrong = int((got[keep] != want[keep]).sum())
    print(f"CONF sampler {name} V{V}: {wrong} wrong of {int(keep.sum())}, "
          f"{int(excluded.sum())} excluded")
    assert wrong == 0
    if c["counts"] is not None:
        after = c["counts_dev"].cpu()
        bump = torch.zeros_like(c["counts"])
        bump[torch.arange(got.numel()), got] = 1
        assert torch.equal(after, c["counts"] + bump)


def test_sampler_neg_inf_logits_never_drawn():
    gen = torch.Generator().manual_seed(50)
    B, V = 512, 300
    c = ko.sampler_case("T1.0", V, B=B, seed=7)
    dead = torch.rand(B, V, generator=gen) < 0.5
    dead[:, 0] = False
    c["logits"] = c["logits"].masked_fill(dead, -math.inf)
    want, excluded = ko.sampler_expected(c)
    assert float(excluded.float().mean()) <= 0.02
    got = _sample(c).cpu()
    assert not bool(dead[torch.arange(B), got].any())
    assert torch.equal(got[~excluded], want[~excluded])


def test_sampler_full_vocab_greedy_and_sampled():
    V = 151936
    gen = torch.Generator().manual_seed(51)
    logits = (torch.randn(2, V, generator=gen) * 3).to(BF16)
    c = dict(logits=logits, temps=torch.tensor([0.0, 1.0]),
             top_ps=torch.ones(2), top_ks=torch.zeros(2, dtype=torch.int32),
             pres=torch.zeros(2), freqs=torch.zeros(2), counts=None)
    # input condition: a draw well inside its interval (the fp32 scan
    # over 152k weights is coarser than over 1k)
    for seed in range(1, 50):
        c["seeds"] = torch.tensor([seed, seed], dtype=torch.int64)
        want, excluded = ko.sampler_expected(c, edge=1e-3)
        if not bool(excluded.any()):
            break
    else:
        pytest.fail("no seed with a draw clear of the interval edges")
    got = _sample(c).cpu()
    assert int(got[0]) == int(logits[0].float().argmax())
    assert torch.equal(got, want)


# --------------------------------------------------------------------------
# GEMM family
# --------------------------------------------------------------------------
def _linear(ops, c, rows=None):
    x = dev(c["x"]) if rows is None else dev(c["x"][rows])
    before = ops.gemm_dispatch_count
    with torch.no_grad():
        out = ops.linear(x, dev(c["w"]), dev(c["b"]))
    assert ops.gemm_dispatch_count == before + 1, "not the hand-written GEMM"
    return out


def _gemm_check(name, c, M):
    ops = _ops()
    sub = dict(c, x=c["x"][:M])
    ref64 = ko.linear(dev(sub["x"]), dev(c["w"]), dev(c["b"]))
    emu = ko.bf16_round(ko.linear(dev(sub["x"]), dev(c["w"]), dev(c["b"]),
                                  dtype=torch.float32))
    check(name, _linear(ops, sub), ref64, ko.nme(emu, ref64))


@pytest.mark.parametrize("M", [1, 64, 65, 257])
@pytest.mark.parametrize("bias", [False, True])
def test_gemm_wide_class(M, bias):
    """N = 65664 >= 65536 takes the 256x256 kernel above M = 64; N is a
    multiple of 64 but not of 256, so the last column panel is partial."""
    c = ko.gemm_case(257, 65664, 128, bias)
    _gemm_check(f"gemm wide N65664 K128 M{M} bias{int(bias)}", c, M)


@pytest.mark.parametrize("M", [1, 65])
def test_gemm_wide_class_k_tail(M):
    c = ko.gemm_case(65, 65664, 96, False)
    _gemm_check(f"gemm wide N65664 K96 M{M}", c, M)


@pytest.mark.parametrize("M,N,K", [(3, 64, 32), (65, 64, 64)])
def test_gemm_tiny_shapes(M, N, K):
    c = ko.gemm_case(M, N, K, True)
    _gemm_check(f"gemm M{M} N{N} K{K}", c, M)


@pytest.mark.parametrize("N,K,Ms", [(65664, 128, (1, 64, 65, 257)),
                                    (128, 8192, (1, 64, 65, 300))])
def test_gemm_row_m_independence_wide_and_deepk(N, K, Ms):
    ops = _ops()
    assert ops._gemm_class(N, K) == ("wide" if N > 65535 else "deepk")
    c = ko.gemm_case(max(Ms), N, K, False, seed=1)
    full = _linear(ops, c)
    for M in Ms[:-1]:
        part = _linear(ops, c, slice(0, M))
        assert torch.equal(part, full[:M]), f"M={M} differs from M={max(Ms)}"
    one = _linear(ops, c, slice(7, 8))
    assert torch.equal(one[0], full[7])


# --------------------------------------------------------------------------
# grouped MoE GEMM
# --------------------------------------------------------------------------
def _moe_run(C, c, ws_dev, scales_dev, seg, tok, fp8):
    wp = torch.tensor([w.data_ptr() for w in ws_dev], dtype=torch.int64,
                      device=DEV)
    sp = None
    if fp8:
        sp = torch.tensor([s.data_ptr() for s in scales_dev],
                          dtype=torch.int64, device=DEV)
    return C.moe_gemm(dev(c["x"]), dev(tok), dev(seg), wp, sp, c["N"], fp8)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("K", [256, 96])
def test_moe_segments_130_64_0_6(K, fp8):
    """Segment sizes {130, 64, 0, 6}: the 64-row re-pipelining loop runs
    three, one and no times, and once on a short tail."""
    C = _ops()._require_ext()
    c = ko.moe_case(K)
    ws, scales = c["ws"], None
    if fp8:
        from tensorlink_amd.models.quant import quantize_fp8_per_channel
        qs = [quantize_fp8_per_channel(dev(w)) for w in ws]
        ws_dev = [a.contiguous() for a, _ in qs]
        scales_dev = [s.float().contiguous() for _, s in qs]
        ws = [a.float().cpu() for a in ws_dev]
        scales = [s.cpu() for s in scales_dev]
    else:
        ws_dev, scales_dev = [dev(w) for w in ws], None
    ref64, e0 = ko.moe_reference(c, ws, scales)
    out = _moe_run(C, c, ws_dev, scales_dev, c["seg"], c["tok"], fp8)
    check(f"moe K{K} fp8{int(fp8)}", out, ref64, e0)
    # a pair's row does not depend on the other segments
    seg = c["seg"].tolist()
    for e in range(len(ko.MOE_SEGMENTS)):
        a, b = seg[e], seg[e + 1]
        if b == a:
            continue
        solo_seg = torch.tensor([0] * (e + 1) + [b - a] * (len(seg) - e - 1),
                                dtype=torch.int32)
        solo = _moe_run(C, c, ws_dev, scales_dev, solo_seg, c["tok"][a:b],
                        fp8)
        assert torch.equal(solo, out[a:b]), f"expert {e} segment alone"


def test_moe_fp8_lut_all_codes():
    """Weight bytes cycle through all 254 non-NaN e4m3 codes; the
    reference decodes them with torch.float8_e4m3fn -> float."""
    C = _ops()._require_ext()
    gen = torch.Generator().manual_seed(60)
    N, K, P = 128, 256, 16
    codes = ko.e4m3_codes()
    wb = codes[torch.arange(N * K) % codes.numel()].view(N, K)
    w8 = wb.view(torch.float8_e4m3fn)
    scale = torch.full((N,), 1.0 / 64)
    x = torch.randn(P, K, generator=gen).to(BF16)
    c = dict(x=x, tok=torch.arange(P, dtype=torch.int32), N=N,
             seg=torch.tensor([0, P], dtype=torch.int32))
    ref64, e0 = ko.moe_reference(c, [w8.float()], [scale])
    out = _moe_run(C, c, [dev(w8).contiguous()], [dev(scale)], c["seg"],
                   c["tok"], True)
    check("moe fp8 LUT 254 codes", out, ref64, e0)
