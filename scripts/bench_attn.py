"""Isolated prefill-attention timing.

    python scripts/bench_attn.py            # ours vs ROCm SDPA
    python scripts/bench_attn.py --ab       # v2 / v3 alternating, + SDPA
    python scripts/bench_attn.py --ab --cache-views   # v3 on the cache views

--ab times the HIP kernel with and without TL_NO_PREFILL_V3=1 (read per
call), alternating the two arms over --rounds rounds so drift hits both,
and checks the outputs bit-equal first. TF counts causal-half FLOPs."""
import argparse, sys, os, time, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensorlink_amd import ops, _C

ap = argparse.ArgumentParser()
ap.add_argument("--ab", action="store_true")
ap.add_argument("--cache-views", action="store_true",
                help="k/v as permuted views of a [B,Hkv,S,D] buffer")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()

def timeit(fn, iters):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3  # ms

def hip_attn(q, k, v):
    # the HIP kernel at every S (ops.attention_prefill routes S >= 4096 to SDPA)
    return _C.prefill_attn(q, k, v, q.shape[-1] ** -0.5, True, 0)

def with_v2(fn):
    os.environ["TL_NO_PREFILL_V3"] = "1"
    try:
        return fn()
    finally:
        del os.environ["TL_NO_PREFILL_V3"]

SHAPES = [(64,512,28,4,128,"qwen7b-prefill-b64"),(256,512,28,4,128,"qwen7b-prefill"),
          (8,4096,32,8,128,"long4k"),(1,8192,32,8,128,"long8k")]
for B,S,Hq,Hkv,D,name in SHAPES:
    q = torch.randn(B,S,Hq,D,device="cuda",dtype=torch.bfloat16)
    k = torch.randn(B,S,Hkv,D,device="cuda",dtype=torch.bfloat16)
    v = torch.randn(B,S,Hkv,D,device="cuda",dtype=torch.bfloat16)
    if args.cache_views:
        k = k.permute(0,2,1,3).contiguous().permute(0,2,1,3)
        v = v.permute(0,2,1,3).contiguous().permute(0,2,1,3)
    flops = 2*2*B*Hq*S*S*D/2
    tf = lambda ms: flops/ms/1e9
    rep = Hq//Hkv
    qt,kt,vt = q.transpose(1,2), k.transpose(1,2).repeat_interleave(rep,1), v.transpose(1,2).repeat_interleave(rep,1)
    sdpa = lambda: torch.nn.functional.scaled_dot_product_attention(qt,kt,vt,is_causal=True)
    if not args.ab:
        t_mine = timeit(lambda: ops.attention_prefill(q,k,v), args.iters)
        t_sdpa = timeit(sdpa, args.iters)
        print(f"{name}: mine {t_mine:.2f}ms ({tf(t_mine):.0f} TF)  sdpa {t_sdpa:.2f}ms ({tf(t_sdpa):.0f} TF)")
        continue
    same = torch.equal(hip_attn(q,k,v), with_v2(lambda: hip_attn(q,k,v)))
    t2, t3 = [], []
    for _ in range(args.rounds):
        t2.append(with_v2(lambda: timeit(lambda: hip_attn(q,k,v), args.iters)))
        t3.append(timeit(lambda: hip_attn(q,k,v), args.iters))
    t_sdpa = timeit(sdpa, args.iters)
    f = lambda ts: " ".join(f"{t:.3f}" for t in ts)
    print(f"{name}: bit-equal {same}\n  v2 ms [{f(t2)}]  best {min(t2):.3f} ({tf(min(t2)):.0f} TF)"
          f"\n  v3 ms [{f(t3)}]  best {min(t3):.3f} ({tf(min(t3)):.0f} TF)  worst {max(t3):.3f}"
          f"\n  v2/v3 {min(t2)/min(t3):.2f}x   sdpa {t_sdpa:.3f} ms ({tf(t_sdpa):.0f} TF)", flush=True)
