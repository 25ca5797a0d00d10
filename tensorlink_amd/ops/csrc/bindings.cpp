// Python bindings for the tensorlink_amd CDNA4 kernel library.
// Host-side glue only — every kernel lives in the sibling .hip files and is
// reached through an extern "C" launcher taking raw pointers + hipStream_t.

#include <torch/extension.h>

#include <cstdlib>

#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "gemm_policy.hpp"

extern "C" {
void tl_rmsnorm_fwd(const void* x, const void* residual, const void* w,
                    void* y, void* r_out, void* rstd, int64_t N, int H,
                    float eps, hipStream_t stream);
void tl_rmsnorm_add_fwd(const void* x, const void* residual, const void* w,
                        void* y, void* r_out, int64_t N, int H, float eps,
                        int n_split, int mode, hipStream_t stream);
void tl_rmsnorm_bwd(const void* dy, const void* x, const void* w,
                    const void* rstd, void* dx, void* dw, void* dw_partial,
                    int n_blocks, int64_t N, int H, hipStream_t stream);
void tl_rope(void* q, void* k, const void* positions, const void* inv_freq,
             int64_t T, int Hq, int Hkv, int D, float sign,
             hipStream_t stream);
void tl_swiglu_fwd(const void* gate, const void* up, void* out, int64_t n,
                   hipStream_t stream);
void tl_swiglu_bwd(const void* dout, const void* gate, const void* up,
                   void* dgate, void* dup, int64_t n, hipStream_t stream);
void tl_adamw(void* param, const void* grad, void* m, void* v, int64_t n,
              int is_bf16, float lr, double beta1, double beta2, float eps,
              float weight_decay, int step, hipStream_t stream);
void tl_decode_attn(const void* q, const void* k_cache, const void* v_cache,
                    const void* seq_lens, void* out, int B, int Hq, int Hkv,
                    int Smax, int D, float scale, int len_add,
                    hipStream_t stream);
void tl_prefill_attn(const void* q, const void* k, const void* v, void* out,
                     int B, int Sq, int Skv, int q_off, int Hq, int Hkv,
                     int D, float scale, int causal,
                     const int64_t* k_strides, const int64_t* v_strides,
                     int use_v3, hipStream_t stream);
void tl_rope_append(const void* qkv, const void* bias, void* q_out,
                    void* k_cache, void* v_cache, const void* positions,
                    const void* inv_freq, const void* block_table,
                    int64_t T, int row_stride, int S, int Hq, int Hkv,
                    int D, int Smax, int bt_stride, int n_split,
                    int inv_bf16, hipStream_t stream);
void tl_swiglu_fused(const void* gu, void* out, int64_t N, int I,
                     hipStream_t stream);
void tl_decode_attn_mfma(const void* q, const void* k_cache,
                         const void* v_cache, const void* seq_lens,
                         const void* block_table, void* out,
                         void* partial, void* partial_ml, int B, int Hq,
                         int Hkv, int Smax, int D, float scale, int n_split,
                         int bt_stride, int per_row, int len_add,
                         hipStream_t stream);
void tl_skinny_gemm(const void* x, const void* w, const void* bias,
                    void* out, void* partial, int M, int N, int K,
                    int n_split, int reduce, hipStream_t stream);
void tl_gemm_tiled(const void* x, const void* w, const void* bias, void* out,
                   void* partial, int M, int N, int K, int n_split,
                   int reduce, hipStream_t stream);
void tl_gemm_colbal(const void* x, const void* w, void* out, int M, int N,
                    int K, int n_blocks, int fused, hipStream_t stream);
void tl_head_argmax(const void* x, const void* w, void* best, void* tok,
                    int M, int N, int K, hipStream_t stream);
void tl_head_ce_stats(const void* x, const void* w, const void* labels,
                      void* ms, void* tgt, void* lse, void* loss_row, int M,
                      int V, int K, int rows_fast, hipStream_t stream);
void tl_head_ce_grad(const void* x, const void* w, const void* labels,
                     const void* lse, const void* scale, void* g, int M,
                     int V, int K, int rows_fast, hipStream_t stream);
void tl_sample(const void* logits, const void* temps, const void* top_ps,
               const void* top_ks, const void* pres, const void* freqs,
               void* counts, const void* seeds, const void* ctr, void* out,
               uint64_t seed_base, int B, int V, hipStream_t stream);
void tl_bump_counter(void* ctr, hipStream_t stream);
void tl_moe_gemm(const void* x, const void* tok_idx, const void* seg_off,
                 const void* w_ptrs, const void* s_ptrs, void* out, int E,
                 int N, int K, int fp8, hipStream_t stream);
void tl_mxfp4_gemm(const void* x, const void* packed, const void* exps,
                   const void* bias, void* out, void* partial, int M, int N,
                   int K, int n_split, hipStream_t stream);
void tl_mxfp4_moe_gemm(const void* x, const void* tok_idx,
                       const void* seg_off, const void* p_ptrs,
                       const void* e_ptrs, void* out, void* partial, int T,
                       int P, int E, int N, int K, int n_split,
                       hipStream_t stream);
void tl_prefill_attn_lse(const void* q, const void* k, const void* v,
                         void* out, void* lse, int B, int Sq, int Skv,
                         int q_off, int Hq, int Hkv, int D, float scale,
                         int causal, const int64_t* k_strides,
                         const int64_t* v_strides, int use_v3,
                         hipStream_t stream);
void tl_prefill_attn_carry(const void* q, const void* k, const void* v,
                           void* out, void* lse, void* o_state,
                           void* ml_state, int B, int Sq, int Skv, int q_off,
                           int Hq, int Hkv, int D, float scale, int causal,
                           int first, int last, int64_t k_sb, int64_t k_sh,
                           int64_t k_ss, int64_t v_sb, int64_t v_sh,
                           int64_t v_ss, hipStream_t stream);
void tl_attn_bwd(const void* q, const void* k, const void* v,
                 const void* dout, const void* lse, const void* delta,
                 void* dq, void* dk, void* dv, int B, int S, int Hq,
                 int Hkv, int D, float scale, int causal,
                 hipStream_t stream);
}

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

#define CHECK_IN(t, d)                                              \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU");                 \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous");       \
  TORCH_CHECK((t).scalar_type() == (d), #t " wrong dtype")

using torch::Tensor;

std::vector<Tensor> rmsnorm_fwd(Tensor x, c10::optional<Tensor> residual,
                                Tensor w, double eps, bool save_rstd) {
  CHECK_IN(x, torch::kBFloat16);
  CHECK_IN(w, torch::kBFloat16);
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "H must be divisible by 8");
  TORCH_CHECK(H <= 16384, "rmsnorm supports H <= 16384");
  const int64_t N = x.numel() / H;
  auto y = torch::empty_like(x);
  Tensor rstd, r_out;
  if (save_rstd) rstd = torch::empty({N}, x.options().dtype(torch::kFloat));
  const void* res_ptr = nullptr;
  void* rout_ptr = nullptr;
  if (residual.has_value()) {
    CHECK_IN(residual.value(), torch::kBFloat16);
    r_out = torch::empty_like(x);
    res_ptr = residual->data_ptr();
    rout_ptr = r_out.data_ptr();
  }
  tl_rmsnorm_fwd(x.data_ptr(), res_ptr, w.data_ptr(), y.data_ptr(), rout_ptr,
                 save_rstd ? rstd.data_ptr() : nullptr, N, H, (float)eps,
                 cur_stream());
  std::vector<Tensor> outs = {y};
  if (residual.has_value()) outs.push_back(r_out);
  if (save_rstd) outs.push_back(rstd);
  return outs;
}

// Residual add + RMSNorm with x either bf16 [.., H] or the GEMM family's
// fp32 split-K partials [n_split, .., H] (skinny_gemm_partials). mode 1 =
// norm of the unrounded sum (rmsnorm_fwd with residual), 2 = norm of the
// bf16-rounded sum (torch add, then rmsnorm_fwd), 3 = the rounded sum
// alone. Returns {y, r} (mode 3: {r}).
std::vector<Tensor> rmsnorm_add_fwd(Tensor x, Tensor residual,
                                    c10::optional<Tensor> w, double eps,
                                    int64_t mode) {
  CHECK_IN(residual, torch::kBFloat16);
  TORCH_CHECK(mode >= 1 && mode <= 3, "mode must be 1, 2 or 3");
  const int H = residual.size(-1);
  TORCH_CHECK(H % 8 == 0, "H must be divisible by 8");
  TORCH_CHECK(H <= 16384, "rmsnorm supports H <= 16384");
  const int64_t N = residual.numel() / H;
  int n_split = 0;
  if (x.scalar_type() == torch::kFloat) {
    CHECK_IN(x, torch::kFloat);
    TORCH_CHECK(x.dim() >= 2 && x.size(-1) == H &&
                    x.numel() == x.size(0) * residual.numel(),
                "partials must be [n_split, rows, H]");
    n_split = (int)x.size(0);
  } else {
    CHECK_IN(x, torch::kBFloat16);
    TORCH_CHECK(x.numel() == residual.numel() && x.size(-1) == H,
                "x / residual shape mismatch");
  }
  auto r_out = torch::empty_like(residual);
  Tensor y;
  const void* wp = nullptr;
  void* yp = nullptr;
  if (mode != 3) {
    TORCH_CHECK(w.has_value(), "weight required");
    CHECK_IN(w.value(), torch::kBFloat16);
    TORCH_CHECK(w->numel() == H, "weight size mismatch");
    y = torch::empty_like(residual);
    wp = w->data_ptr();
    yp = y.data_ptr();
  }
  tl_rmsnorm_add_fwd(x.data_ptr(), residual.data_ptr(), wp, yp,
                     r_out.data_ptr(), N, H, (float)eps, n_split, (int)mode,
                     cur_stream());
  if (mode == 3) return {r_out};
  return {y, r_out};
}

std::vector<Tensor> rmsnorm_bwd(Tensor dy, Tensor x, Tensor w, Tensor rstd) {
  CHECK_IN(dy, torch::kBFloat16);
  CHECK_IN(x, torch::kBFloat16);
  CHECK_IN(w, torch::kBFloat16);
  CHECK_IN(rstd, torch::kFloat);
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "H must be divisible by 8");
  TORCH_CHECK(H <= 16384, "rmsnorm supports H <= 16384");
  const int64_t N = x.numel() / H;
  const int n_blocks = (int)std::min<int64_t>(N, 512);
  auto dx = torch::empty_like(x);
  auto dw = torch::empty_like(w);
  auto partial = torch::empty({n_blocks, (int64_t)H},
                              x.options().dtype(torch::kFloat));
  tl_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(),
                 dx.data_ptr(), dw.data_ptr(), partial.data_ptr(), n_blocks,
                 N, H, cur_stream());
  return {dx, dw};
}

void rope_(Tensor q, Tensor k, Tensor positions, Tensor inv_freq,
           double sign) {
  CHECK_IN(q, torch::kBFloat16);
  CHECK_IN(k, torch::kBFloat16);
  CHECK_IN(positions, torch::kInt);
  CHECK_IN(inv_freq, torch::kFloat);
  const int D = q.size(-1);
  const int Hq = q.size(-2);
  const int Hkv = k.size(-2);
  const int64_t T = q.numel() / ((int64_t)Hq * D);
  TORCH_CHECK(k.numel() / ((int64_t)Hkv * D) == T, "q/k token mismatch");
  TORCH_CHECK(positions.numel() == T, "positions size mismatch");
  tl_rope(q.data_ptr(), k.data_ptr(), positions.data_ptr(),
          inv_freq.data_ptr(), T, Hq, Hkv, D, (float)sign, cur_stream());
}

Tensor swiglu_fwd(Tensor gate, Tensor up) {
  CHECK_IN(gate, torch::kBFloat16);
  CHECK_IN(up, torch::kBFloat16);
  TORCH_CHECK(gate.numel() % 8 == 0, "numel must be divisible by 8");
  auto out = torch::empty_like(gate);
  tl_swiglu_fwd(gate.data_ptr(), up.data_ptr(), out.data_ptr(), gate.numel(),
                cur_stream());
  return out;
}

std::vector<Tensor> swiglu_bwd(Tensor dout, Tensor gate, Tensor up) {
  CHECK_IN(dout, torch::kBFloat16);
  auto dg = torch::empty_like(gate);
  auto du = torch::empty_like(up);
  tl_swiglu_bwd(dout.data_ptr(), gate.data_ptr(), up.data_ptr(), dg.data_ptr(),
                du.data_ptr(), gate.numel(), cur_stream());
  return {dg, du};
}

void adamw_(Tensor param, Tensor grad, Tensor m, Tensor v, double lr,
            double beta1, double beta2, double eps, double weight_decay,
            int64_t step) {
  TORCH_CHECK(param.is_cuda() && param.is_contiguous());
  TORCH_CHECK(m.scalar_type() == torch::kFloat &&
              v.scalar_type() == torch::kFloat);
  TORCH_CHECK(grad.scalar_type() == param.scalar_type());
  const bool is_bf16 = param.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(is_bf16 || param.scalar_type() == torch::kFloat);
  tl_adamw(param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
           param.numel(), is_bf16 ? 1 : 0, (float)lr, beta1, beta2,
           (float)eps, (float)weight_decay, (int)step,
           cur_stream());
}

Tensor decode_attn(Tensor q, Tensor k_cache, Tensor v_cache, Tensor seq_lens,
                   double scale, int64_t n_split,
                   c10::optional<Tensor> block_table, int64_t len_add) {
  CHECK_IN(q, torch::kBFloat16);
  CHECK_IN(k_cache, torch::kBFloat16);
  CHECK_IN(v_cache, torch::kBFloat16);
  CHECK_IN(seq_lens, torch::kInt);
  const int B = q.size(0), Hq = q.size(1), D = q.size(2);
  const int Hkv = k_cache.size(1), Smax = k_cache.size(2);
  const int G = Hq / Hkv;
  const void* bt = nullptr;
  int bt_stride = 0;
  if (block_table.has_value()) {
    CHECK_IN(block_table.value(), torch::kInt);
    TORCH_CHECK(G <= 16, "paged decode requires GQA group <= 16");
    TORCH_CHECK(k_cache.size(2) == 128, "paged pool PAGE must be 128");
    bt = block_table->data_ptr();
    bt_stride = block_table->size(1);
  }
  TORCH_CHECK(D == 64 || D == 128, "head_dim must be 64 or 128");
  TORCH_CHECK(Hq % Hkv == 0, "GQA requires Hq % Hkv == 0");
  auto out = torch::empty_like(q);
  const bool legacy = (getenv("TL_DECODE_LEGACY") != nullptr || G > 16) &&
                      bt == nullptr;
  if (legacy) {
    tl_decode_attn(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                   seq_lens.data_ptr(), out.data_ptr(), B, Hq, Hkv, Smax, D,
                   (float)scale, (int)len_add, cur_stream());
    return out;
  }
  int per_row = 0;
  if (n_split <= 0) {
    // auto: per-ROW split from each row's own length (tl_split_for_len,
    // gemm_policy.hpp) so a sequence's numerics are batch-independent; the
    // launch z-width comes from a batch-shape-free host bound on L
    // (cache capacity, which bounds seq_lens + len_add too), no device
    // sync needed.
    per_row = 1;
    const int upper = bt ? bt_stride * 128 : Smax;
    n_split = tl_split_for_len(upper);
  }
  TORCH_CHECK(n_split <= 64, "n_split too large");
  Tensor partial, partial_ml;
  void *pp = nullptr, *pml = nullptr;
  if (n_split > 1) {
    partial = torch::empty({(int64_t)B * Hq * n_split * D},
                           q.options().dtype(torch::kFloat));
    partial_ml = torch::empty({(int64_t)B * Hq * n_split * 2},
                              q.options().dtype(torch::kFloat));
    pp = partial.data_ptr();
    pml = partial_ml.data_ptr();
  }
  tl_decode_attn_mfma(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                      seq_lens.data_ptr(), bt, out.data_ptr(), pp, pml, B,
                      Hq, Hkv, Smax, D, (float)scale, (int)n_split,
                      bt_stride, per_row, (int)len_add, cur_stream());
  return out;
}

// K/V operands of the prefill kernels: [B,Skv,Hkv,D] views with D
// contiguous. v3 reads them through their {batch, head, token} strides, so
// a permuted [B,Hkv,Smax,D] cache view goes in as it is. TL_NO_PREFILL_V3=1
// (read per call) keeps the v2 kernel, which reads contiguous K/V only, so
// the copy happens here.
struct PrefillKV {
  Tensor k, v;
  int64_t ks[3], vs[3];
  int use_v3;
};

PrefillKV prefill_kv(const Tensor& k_in, const Tensor& v_in,
                     bool v3_only = false) {
  PrefillKV p;
  const char* off = std::getenv("TL_NO_PREFILL_V3");
  p.use_v3 = v3_only || !(off && *off);
  for (const Tensor* t : {&k_in, &v_in}) {
    TORCH_CHECK(t->is_cuda(), "k/v must be on GPU");
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16, "k/v wrong dtype");
    TORCH_CHECK(t->dim() == 4, "k/v must be [B,Skv,Hkv,D]");
  }
  TORCH_CHECK(k_in.sizes() == v_in.sizes(), "k and v shapes differ");
  // 16-byte row loads: D contiguous, every other stride a multiple of 8
  auto direct = [](const Tensor& t) {
    if (t.size(3) != 1 && t.stride(3) != 1) return false;
    for (int d = 0; d < 3; ++d)
      if (t.size(d) != 1 && t.stride(d) % 8 != 0) return false;
    return t.storage_offset() % 8 == 0;
  };
  p.k = (p.use_v3 && direct(k_in)) ? k_in : k_in.contiguous();
  p.v = (p.use_v3 && direct(v_in)) ? v_in : v_in.contiguous();
  const Tensor* ts[2] = {&p.k, &p.v};
  int64_t* ss[2] = {p.ks, p.vs};
  for (int i = 0; i < 2; ++i) {
    const Tensor& t = *ts[i];
    // a size-1 dim's stride is never used: report 0, not what torch kept
    ss[i][0] = t.size(0) > 1 ? t.stride(0) : 0;
    ss[i][1] = t.size(2) > 1 ? t.stride(2) : 0;
    ss[i][2] = t.size(1) > 1 ? t.stride(1) : 0;
  }
  return p;
}

Tensor prefill_attn(Tensor q, Tensor k, Tensor v, double scale, bool causal,
                    int64_t q_off) {
  CHECK_IN(q, torch::kBFloat16);
  auto kv = prefill_kv(k, v);
  const int B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
  const int Skv = k.size(1);
  const int Hkv = k.size(2);
  TORCH_CHECK(D == 64 || D == 128, "head_dim must be 64 or 128");
  TORCH_CHECK(k.size(0) == B && k.size(3) == D && Hq % Hkv == 0,
              "k/v do not match q");
  TORCH_CHECK(q_off + Sq <= Skv || !causal, "q_off + Sq must fit Skv");
  auto out = torch::empty_like(q);
  tl_prefill_attn(q.data_ptr(), kv.k.data_ptr(), kv.v.data_ptr(),
                  out.data_ptr(), B, Sq, Skv, (int)q_off, Hq, Hkv, D,
                  (float)scale, causal ? 1 : 0, kv.ks, kv.vs, kv.use_v3,
                  cur_stream());
  return out;
}

std::vector<Tensor> prefill_attn_lse(Tensor q, Tensor k, Tensor v,
                                     double scale, bool causal) {
  CHECK_IN(q, torch::kBFloat16);
  auto kv = prefill_kv(k, v);
  const int B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
  const int Skv = k.size(1);
  const int Hkv = k.size(2);
  TORCH_CHECK(D == 64 || D == 128, "head_dim must be 64 or 128");
  TORCH_CHECK(k.size(0) == B && k.size(3) == D && Hq % Hkv == 0,
              "k/v do not match q");
  auto out = torch::empty_like(q);
  auto lse = torch::empty({B, Hq, Sq}, q.options().dtype(torch::kFloat));
  tl_prefill_attn_lse(q.data_ptr(), kv.k.data_ptr(), kv.v.data_ptr(),
                      out.data_ptr(), lse.data_ptr(), B, Sq, Skv, 0, Hq,
                      Hkv, D, (float)scale, causal ? 1 : 0, kv.ks, kv.vs,
                      kv.use_v3, cur_stream());
  return {out, lse};
}

// One key chunk of a carried online softmax (prefill_attn_v3.hip, CARRY):
// o_state [B,Sq,Hq,D] and ml_state [B,Hq,Sq,2] are the caller's fp32 state,
// read unless `first`, written in place unless `last`. Returns None, or on
// `last` out (bf16), or (out, lse) with want_lse. v3 only: TL_NO_PREFILL_V3
// does not apply.
py::object prefill_attn_carry(Tensor q, Tensor k, Tensor v, Tensor o_state,
                              Tensor ml_state, double scale, bool causal,
                              int64_t q_off, bool first, bool last,
                              bool want_lse) {
  CHECK_IN(q, torch::kBFloat16);
  TORCH_CHECK(q.dim() == 4, "q must be [B,Sq,Hq,D]");
  auto kv = prefill_kv(k, v, /*v3_only=*/true);
  const int B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
  const int Skv = k.size(1);
  const int Hkv = k.size(2);
  TORCH_CHECK(D == 64 || D == 128, "head_dim must be 64 or 128");
  TORCH_CHECK(k.size(0) == B && k.size(3) == D && Hq % Hkv == 0,
              "k/v do not match q");
  TORCH_CHECK(Sq >= 1 && Skv >= 1, "empty q or k/v chunk");
  TORCH_CHECK(q_off >= 0 && (q_off + Sq <= Skv || !causal),
              "q_off + Sq must fit Skv");
  CHECK_IN(o_state, torch::kFloat);
  CHECK_IN(ml_state, torch::kFloat);
  TORCH_CHECK(o_state.get_device() == q.get_device() &&
                  ml_state.get_device() == q.get_device(),
              "state must be on q's device");
  TORCH_CHECK(o_state.sizes() == q.sizes(), "o_state must be [B,Sq,Hq,D]");
  TORCH_CHECK(ml_state.dim() == 4 && ml_state.size(0) == B &&
                  ml_state.size(1) == Hq && ml_state.size(2) == Sq &&
                  ml_state.size(3) == 2,
              "ml_state must be [B,Hq,Sq,2]");
  Tensor out, lse;
  if (last) {
    out = torch::empty_like(q);
    if (want_lse)
      lse = torch::empty({B, Hq, Sq}, q.options().dtype(torch::kFloat));
  }
  tl_prefill_attn_carry(
      q.data_ptr(), kv.k.data_ptr(), kv.v.data_ptr(),
      last ? out.data_ptr() : nullptr, lse.defined() ? lse.data_ptr() : nullptr,
      o_state.data_ptr(), ml_state.data_ptr(), B, Sq, Skv, (int)q_off, Hq,
      Hkv, D, (float)scale, causal ? 1 : 0, first ? 1 : 0, last ? 1 : 0,
      kv.ks[0], kv.ks[1], kv.ks[2], kv.vs[0], kv.vs[1], kv.vs[2],
      cur_stream());
  if (!last) return py::none();
  if (want_lse) return py::make_tuple(out, lse);
  return py::cast(out);
}

std::vector<Tensor> attn_bwd(Tensor q, Tensor k, Tensor v, Tensor dout,
                             Tensor lse, Tensor delta, double scale,
                             bool causal) {
  CHECK_IN(q, torch::kBFloat16);
  CHECK_IN(k, torch::kBFloat16);
  CHECK_IN(v, torch::kBFloat16);
  CHECK_IN(dout, torch::kBFloat16);
  CHECK_IN(lse, torch::kFloat);
  CHECK_IN(delta, torch::kFloat);
  const int B = q.size(0), S = q.size(1), Hq = q.size(2), D = q.size(3);
  const int Hkv = k.size(2);
  TORCH_CHECK(k.size(1) == S, "training attention needs Sq == Skv");
  TORCH_CHECK(D == 64 || D == 128, "head_dim must be 64 or 128");
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  tl_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), dout.data_ptr(),
              lse.data_ptr(), delta.data_ptr(), dq.data_ptr(),
              dk.data_ptr(), dv.data_ptr(), B, S, Hq, Hkv, D, (float)scale,
              causal ? 1 : 0, cur_stream());
  return {dq, dk, dv};
}

// qkv: [T, row_stride] fused projection output (q | k | v per row), bf16 —
// or the projection's fp32 split-K partials [n_split, T, row_stride]
// (skinny_gemm_partials) with its bias passed alongside. inv_freq fp32 or
// bf16. Returns rotated q as a contiguous [T, Hq, D] tensor; k/v land in
// the caches.
Tensor rope_append_(Tensor qkv, Tensor k_cache, Tensor v_cache,
                    Tensor positions, Tensor inv_freq, int64_t S,
                    int64_t Hq, int64_t Hkv,
                    c10::optional<Tensor> block_table,
                    c10::optional<Tensor> bias) {
  CHECK_IN(k_cache, torch::kBFloat16);
  CHECK_IN(v_cache, torch::kBFloat16);
  CHECK_IN(positions, torch::kInt);
  TORCH_CHECK(inv_freq.is_cuda() && inv_freq.is_contiguous(),
              "inv_freq must be a contiguous GPU tensor");
  const bool inv_bf16 = inv_freq.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(inv_bf16 || inv_freq.scalar_type() == torch::kFloat,
              "inv_freq must be fp32 or bf16");
  const int D = k_cache.size(3);
  TORCH_CHECK(inv_freq.numel() >= D / 2, "inv_freq too short");
  const int row_stride = qkv.size(-1);
  TORCH_CHECK(row_stride == (Hq + 2 * Hkv) * D, "qkv width mismatch");
  int n_split = 0;
  const void* bp = nullptr;
  if (qkv.scalar_type() == torch::kFloat) {
    CHECK_IN(qkv, torch::kFloat);
    TORCH_CHECK(qkv.dim() >= 2, "partials must be [n_split, T, width]");
    n_split = (int)qkv.size(0);
    TORCH_CHECK(row_stride <= 32768, "qkv row too wide for the LDS stage");
    if (bias.has_value()) {
      CHECK_IN(bias.value(), torch::kBFloat16);
      TORCH_CHECK(bias->numel() == row_stride, "bias size mismatch");
      bp = bias->data_ptr();
    }
  } else {
    CHECK_IN(qkv, torch::kBFloat16);
    TORCH_CHECK(!bias.has_value(), "bias goes with partials only");
  }
  const int64_t T = qkv.numel() / row_stride / (n_split ? n_split : 1);
  TORCH_CHECK(positions.numel() == T, "positions size mismatch");
  const int Smax = k_cache.size(2);
  TORCH_CHECK(T % S == 0, "T must be divisible by S");
  TORCH_CHECK(D % 16 == 0, "D must be divisible by 16");
  const void* bt = nullptr;
  int bt_stride = 0;
  if (block_table.has_value()) {
    CHECK_IN(block_table.value(), torch::kInt);
    TORCH_CHECK(k_cache.size(2) == 128, "paged pool PAGE must be 128");
    bt = block_table->data_ptr();
    bt_stride = block_table->size(1);
    TORCH_CHECK(block_table->size(0) * S == T, "table batch mismatch");
  } else {
    TORCH_CHECK(k_cache.size(0) * S == T, "cache batch mismatch");
  }
  auto q_out = torch::empty({T, Hq, (int64_t)D}, k_cache.options());
  tl_rope_append(qkv.data_ptr(), bp, q_out.data_ptr(), k_cache.data_ptr(),
                 v_cache.data_ptr(), positions.data_ptr(),
                 inv_freq.data_ptr(), bt, T, row_stride, (int)S, (int)Hq,
                 (int)Hkv, D, Smax, bt_stride, n_split, inv_bf16 ? 1 : 0,
                 cur_stream());
  return q_out;
}

Tensor swiglu_fused(Tensor gu) {
  CHECK_IN(gu, torch::kBFloat16);
  const int64_t I2 = gu.size(-1);
  TORCH_CHECK(I2 % 16 == 0, "fused width must be divisible by 16");
  const int64_t I = I2 / 2;
  const int64_t N = gu.numel() / I2;
  auto sizes = gu.sizes().vec();
  sizes.back() = I;
  auto out = torch::empty(sizes, gu.options());
  tl_swiglu_fused(gu.data_ptr(), out.data_ptr(), N, (int)I, cur_stream());
  return out;
}

// Split-K policy SHARED by the streaming and tiled GEMM kernels
// (gemm_n_split_for, gemm_policy.hpp): pure in (N, K), never M. The
// split-block target is env-tunable for in-pipeline A/B — read ONCE so the
// policy stays (N,K)-pure in-process.
static int gemm_n_split(int N, int K) {
  static const int target = [] {
    const char* e = getenv("TL_GEMM_SPLIT_TARGET");
    return e ? atoi(e) : 256;
  }();
  return gemm_n_split_for(N, K, target);
}

// The [begin, end) of every split for (K, n_split), from the function the
// kernels slice K with (gemm_k_slice, gemm_policy.hpp): lets a test hold the
// slice contract against the code itself, with no device involved.
static std::vector<std::pair<int, int>> gemm_k_slices(int K, int n_split) {
  TORCH_CHECK(K > 0 && K % 32 == 0 && n_split >= 1, "unsupported shape");
  std::vector<std::pair<int, int>> out;
  for (int s = 0; s < n_split; ++s) {
    const KSlice ks = gemm_k_slice(K, n_split, s);
    out.emplace_back(ks.begin, ks.end);
  }
  return out;
}

// x @ W^T (+ bias) through the streaming (M <= TL_GEMM_STREAM_M) or tiled
// kernel. reduce: the bf16 output [.., N]. !reduce: the fp32 split-K
// partials [n_split, .., N] for a consumer kernel to sum (s order from 0,
// then bias, then one bf16 rounding — exactly what the reduce kernel does),
// so bias is NOT applied; when the policy gives n_split == 1 there is
// nothing to hand out and the bf16 output comes back, bias included.
static Tensor family_gemm(Tensor x, Tensor w, c10::optional<Tensor> bias,
                          bool reduce) {
  CHECK_IN(x, torch::kBFloat16);
  CHECK_IN(w, torch::kBFloat16);
  const int K = x.size(-1);
  const int64_t M = x.numel() / K;
  const int N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "K mismatch");
  TORCH_CHECK(K % 32 == 0 && N % 64 == 0, "unsupported shape");
  const int n_split = gemm_n_split(N, K);
  const bool hand_out = !reduce && n_split > 1;
  auto sizes = x.sizes().vec();
  sizes.back() = N;
  Tensor out, partial;
  const void* bp = nullptr;
  if (hand_out) {
    sizes.insert(sizes.begin(), n_split);
    partial = torch::empty(sizes, x.options().dtype(torch::kFloat));
  } else {
    out = torch::empty(sizes, x.options());
    if (bias.has_value()) {
      CHECK_IN(bias.value(), torch::kBFloat16);
      bp = bias->data_ptr();
    }
    if (n_split > 1)
      partial = torch::empty({(int64_t)n_split * M * N},
                             x.options().dtype(torch::kFloat));
  }
  auto launch = M <= TL_GEMM_STREAM_M ? tl_skinny_gemm : tl_gemm_tiled;
  launch(x.data_ptr(), w.data_ptr(), bp, hand_out ? nullptr : out.data_ptr(),
         n_split > 1 ? partial.data_ptr() : nullptr, (int)M, N, K, n_split,
         hand_out ? 0 : 1, cur_stream());
  return hand_out ? partial : out;
}

Tensor skinny_gemm(Tensor x, Tensor w, c10::optional<Tensor> bias) {
  return family_gemm(x, w, bias, true);
}

Tensor skinny_gemm_partials(Tensor x, Tensor w, c10::optional<Tensor> bias) {
  return family_gemm(x, w, bias, false);
}

// CU count of a device, read once: the column-balanced GEMM launches one
// workgroup per CU (gemm_colbal.hip).
static int device_cu_count(int dev) {
  static int cus[64] = {0};
  TORCH_CHECK(dev >= 0 && dev < 64, "device index out of range");
  if (cus[dev] == 0) {
    int n = 0;
    TORCH_CHECK(hipDeviceGetAttribute(
                    &n, hipDeviceAttributeMultiprocessorCount, dev) ==
                        hipSuccess && n > 0,
                "cannot read the CU count");
    cus[dev] = n;
  }
  return cus[dev];
}

// Column-balanced one-pass GEMM (gemm_colbal.hip): x @ W^T for the wide
// shapes where the policy gives n_split == 1, bitwise equal to skinny_gemm
// there. fused: W is [2I, K] (gate rows, then up rows) and the result is
// swiglu_fused(x @ W^T), [.., I]. n_blocks (workgroups per 256-row block)
// defaults to the CU count; the bits do not depend on it, tests use it to
// force uneven and multi-pass column ranges.
static Tensor gemm_colbal_impl(Tensor x, Tensor w, int64_t n_blocks,
                               bool fused) {
  CHECK_IN(x, torch::kBFloat16);
  CHECK_IN(w, torch::kBFloat16);
  const int K = x.size(-1);
  const int64_t M = x.numel() / K;
  const int N = w.size(0);
  TORCH_CHECK(w.dim() == 2 && w.size(1) == K, "K mismatch");
  TORCH_CHECK(K % 32 == 0 && K >= 32 && M >= 1 && M < (1 << 24),
              "unsupported shape");
  TORCH_CHECK(N % (fused ? 32 : 16) == 0 && N > 0, "unsupported width");
  TORCH_CHECK(gemm_n_split(N, K) == 1,
              "gemm_colbal serves only shapes the policy does not split");
  if (n_blocks <= 0) n_blocks = device_cu_count(x.get_device());
  TORCH_CHECK(n_blocks <= 65535, "n_blocks too large");
  const int NO = fused ? N / 2 : N;
  auto sizes = x.sizes().vec();
  sizes.back() = NO;
  auto out = torch::empty(sizes, x.options());
  tl_gemm_colbal(x.data_ptr(), w.data_ptr(), out.data_ptr(), (int)M, NO, K,
                 (int)n_blocks, fused ? 1 : 0, cur_stream());
  return out;
}

Tensor gemm_colbal(Tensor x, Tensor w, int64_t n_blocks) {
  return gemm_colbal_impl(x, w, n_blocks, false);
}

Tensor gemm_colbal_swiglu(Tensor x, Tensor w_gate_up, int64_t n_blocks) {
  return gemm_colbal_impl(x, w_gate_up, n_blocks, true);
}

// Fused greedy head (head_argmax.hip): argmax over N of bf16(x @ W^T) for
// the wide class where the policy gives n_split == 1, equal to
// skinny_gemm(x, w).argmax(-1) there. The logits are never written; the
// only scratch is one packed winner per (256-column panel, row), fully
// written by the first kernel. Returns int64 with x's leading dimensions.
// The row limit is ops.GEMM_M_MAX (TL_GEMM_M_MAX, read once as there).
Tensor lm_head_argmax(Tensor x, Tensor w) {
  static const int m_max = [] {
    const char* e = getenv("TL_GEMM_M_MAX");
    return e ? atoi(e) : 512;
  }();
  CHECK_IN(x, torch::kBFloat16);
  CHECK_IN(w, torch::kBFloat16);
  TORCH_CHECK(x.dim() >= 1 && w.dim() == 2, "x must be [.., K], w [N, K]");
  const int64_t K = x.size(-1);
  const int64_t N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "K mismatch");
  TORCH_CHECK(w.device() == x.device(), "operands must share a device");
  TORCH_CHECK(K >= 32 && K % 32 == 0 && K < (1 << 24), "unsupported K");
  TORCH_CHECK(N >= TL_GEMM_WIDE_N && N % 64 == 0 && N < (1 << 24),
              "lm_head_argmax serves the wide class: N >= ", TL_GEMM_WIDE_N,
              ", N % 64 == 0");
  TORCH_CHECK(gemm_n_split((int)N, (int)K) == 1,
              "lm_head_argmax serves only shapes the policy does not split");
  const int64_t M = x.numel() / K;
  TORCH_CHECK(M >= 1 && M <= m_max && M < (1 << 24),
              "lm_head_argmax supports 1 <= M <= ", m_max);
  auto sizes = x.sizes().vec();
  sizes.pop_back();
  auto tok = torch::empty(sizes, x.options().dtype(torch::kLong));
  auto best = torch::empty({(N + 255) / 256, M},
                           x.options().dtype(torch::kInt));
  tl_head_argmax(x.data_ptr(), w.data_ptr(), best.data_ptr(), tok.data_ptr(),
                 (int)M, (int)N, (int)K, cur_stream());
  return tok;
}

// Fused linear cross-entropy (head_ce.hip). x [M, K] and w [V, K] bf16,
// labels [M] int64; K % 32 == 0, any V >= 1, any M >= 1. The logits are
// never written. Rows are walked in launches of rows_per_launch (0 = the
// default) so the stats scratch, one (m, s) float2 per (256-column panel,
// row) plus one float per row, stays bounded: at the default of 8192 rows
// it is cdiv(V, 256) * 8192 * 8 B + 32 KB, 39 MB at V = 152064. A row's
// bits depend on nothing but that row, so they do not depend on
// rows_per_launch. rows_fast picks the grid order (head_ce.hip) for A/B
// runs; it does not change a bit either.
constexpr int64_t HEAD_CE_ROWS_PER_LAUNCH = 8192;

static void head_ce_check(const Tensor& x, const Tensor& w,
                          const Tensor& labels, int64_t rows_per_launch) {
  CHECK_IN(x, torch::kBFloat16);
  CHECK_IN(w, torch::kBFloat16);
  CHECK_IN(labels, torch::kLong);
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && labels.dim() == 1,
              "x must be [M, K], w [V, K], labels [M]");
  TORCH_CHECK(w.size(1) == x.size(1), "K mismatch");
  TORCH_CHECK(labels.size(0) == x.size(0), "labels must have one per row");
  TORCH_CHECK(w.device() == x.device() && labels.device() == x.device(),
              "operands must share a device");
  const int64_t K = x.size(1);
  TORCH_CHECK(K >= 32 && K % 32 == 0 && K < (1 << 24), "unsupported K");
  TORCH_CHECK(w.size(0) >= 1 && w.size(0) < (1 << 24), "unsupported V");
  TORCH_CHECK(x.size(0) >= 1, "M must be >= 1");
  TORCH_CHECK(rows_per_launch >= 0 && rows_per_launch < (1 << 24),
              "rows_per_launch out of range");
}

std::vector<Tensor> head_ce_stats(Tensor x, Tensor w, Tensor labels,
                                  int64_t rows_per_launch,
                                  int64_t rows_fast) {
  head_ce_check(x, w, labels, rows_per_launch);
  const int64_t M = x.size(0), K = x.size(1), V = w.size(0);
  const int64_t rpl = std::min(
      M, rows_per_launch ? rows_per_launch : HEAD_CE_ROWS_PER_LAUNCH);
  const int64_t P = (V + 255) / 256;
  auto f32 = x.options().dtype(torch::kFloat);
  auto lse = torch::empty({M}, f32);
  auto loss_row = torch::empty({M}, f32);
  // [P, rpl] float2 (m, s), then [rpl] label logits
  auto scratch = torch::empty({P * rpl * 2 + rpl}, f32);
  float* ms = scratch.data_ptr<float>();
  float* tgt = ms + P * rpl * 2;
  for (int64_t r0 = 0; r0 < M; r0 += rpl) {
    const int64_t rows = std::min(rpl, M - r0);
    tl_head_ce_stats(
        static_cast<const char*>(x.data_ptr()) + r0 * K * 2, w.data_ptr(),
        labels.data_ptr<int64_t>() + r0, ms, tgt,
        lse.data_ptr<float>() + r0, loss_row.data_ptr<float>() + r0,
        (int)rows, (int)V, (int)K, (int)rows_fast, cur_stream());
  }
  return {lse, loss_row};
}

Tensor head_ce_grad(Tensor x, Tensor w, Tensor labels, Tensor lse,
                    Tensor scale, int64_t rows_per_launch, int64_t rows_fast,
                    c10::optional<Tensor> out) {
  head_ce_check(x, w, labels, rows_per_launch);
  CHECK_IN(lse, torch::kFloat);
  CHECK_IN(scale, torch::kFloat);
  const int64_t M = x.size(0), K = x.size(1), V = w.size(0);
  TORCH_CHECK(lse.dim() == 1 && lse.size(0) == M && scale.dim() == 1 &&
                  scale.size(0) == M,
              "lse and scale must be [M]");
  TORCH_CHECK(lse.device() == x.device() && scale.device() == x.device(),
              "operands must share a device");
  Tensor g;
  if (out.has_value()) {
    g = *out;
    CHECK_IN(g, torch::kBFloat16);
    TORCH_CHECK(g.dim() == 2 && g.size(0) == M && g.size(1) == V &&
                    g.device() == x.device(),
                "out must be [M, V] on x's device");
  } else {
    g = torch::empty({M, V}, x.options());
  }
  const int64_t rpl = std::min(
      M, rows_per_launch ? rows_per_launch : HEAD_CE_ROWS_PER_LAUNCH);
  for (int64_t r0 = 0; r0 < M; r0 += rpl) {
    const int64_t rows = std::min(rpl, M - r0);
    tl_head_ce_grad(
        static_cast<const char*>(x.data_ptr()) + r0 * K * 2, w.data_ptr(),
        labels.data_ptr<int64_t>() + r0, lse.data_ptr<float>() + r0,
        scale.data_ptr<float>() + r0,
        static_cast<char*>(g.data_ptr()) + r0 * V * 2, (int)rows, (int)V,
        (int)K, (int)rows_fast, cur_stream());
  }
  return g;
}

// Split-K policy of the MXFP4 kernels: mxfp4_split_for_blocks
// (gemm_policy.hpp) over the grid before the split.
static int mxfp4_n_split(int N, int K) {
  return mxfp4_split_for_blocks(N / 64, K);
}

// Grouped expert kernel (mxfp4_moe_gemm.hip): pure in (N, K, E), never P
// or the routing, so a pair's row is the same in every call.
static int mxfp4_moe_n_split(int N, int K, int E) {
  return mxfp4_split_for_blocks((N / 64) * E, K);
}

int64_t mxfp4_n_split_py(int64_t N, int64_t K) {
  TORCH_CHECK(N > 0 && K > 0 && N % 64 == 0 && K % 128 == 0,
              "unsupported shape");
  return mxfp4_n_split((int)N, (int)K);
}

int64_t mxfp4_moe_n_split_py(int64_t N, int64_t K, int64_t E) {
  TORCH_CHECK(N > 0 && K > 0 && E > 0 && N % 64 == 0 && K % 128 == 0,
              "unsupported shape");
  return mxfp4_moe_n_split((int)N, (int)K, (int)E);
}

Tensor mxfp4_gemm(Tensor x, Tensor packed, Tensor exponents,
                  c10::optional<Tensor> bias) {
  CHECK_IN(x, torch::kBFloat16);
  CHECK_IN(packed, torch::kByte);
  CHECK_IN(exponents, torch::kChar);
  TORCH_CHECK(packed.dim() == 2 && exponents.dim() == 2,
              "packed / exponents must be 2-D");
  TORCH_CHECK(x.dim() >= 1, "x must have a K dimension");
  const int64_t K = x.size(-1);
  const int64_t N = packed.size(0);
  TORCH_CHECK(K > 0 && N > 0 && N % 64 == 0 && K % 128 == 0,
              "unsupported shape: need N % 64 == 0 and K % 128 == 0");
  TORCH_CHECK(packed.size(1) * 2 == K, "packed must be [N, K/2]");
  TORCH_CHECK(exponents.size(0) == N && exponents.size(1) * 32 == K,
              "exponents must be [N, K/32]");
  const int64_t M = x.numel() / K;
  TORCH_CHECK(M >= 1 && M <= 512, "mxfp4_gemm supports 1 <= M <= 512");
  TORCH_CHECK(packed.device() == x.device() &&
                  exponents.device() == x.device(),
              "operands must share a device");
  auto sizes = x.sizes().vec();
  sizes.back() = N;
  auto out = torch::empty(sizes, x.options());
  const void* bp = nullptr;
  if (bias.has_value()) {
    CHECK_IN(bias.value(), torch::kBFloat16);
    TORCH_CHECK(bias->numel() == N, "bias must be [N]");
    bp = bias->data_ptr();
  }
  const int n_split = mxfp4_n_split((int)N, (int)K);
  Tensor partial;
  void* pp = nullptr;
  if (n_split > 1) {
    partial = torch::empty({(int64_t)n_split * M * N},
                           x.options().dtype(torch::kFloat));
    pp = partial.data_ptr();
  }
  tl_mxfp4_gemm(x.data_ptr(), packed.data_ptr(), exponents.data_ptr(), bp,
                out.data_ptr(), pp, (int)M, (int)N, (int)K, n_split,
                cur_stream());
  return out;
}

Tensor sample_tokens(Tensor logits, Tensor temps, Tensor top_ps,
                     Tensor top_ks, Tensor pres, Tensor freqs,
                     c10::optional<Tensor> counts,
                     c10::optional<Tensor> seeds,
                     c10::optional<Tensor> counter, int64_t seed_base) {
  CHECK_IN(logits, torch::kBFloat16);
  CHECK_IN(temps, torch::kFloat);
  CHECK_IN(top_ps, torch::kFloat);
  CHECK_IN(top_ks, torch::kInt);
  CHECK_IN(pres, torch::kFloat);
  CHECK_IN(freqs, torch::kFloat);
  const int B = logits.size(0);
  const int V = logits.size(1);
  void* cnt = nullptr;
  if (counts.has_value()) {
    CHECK_IN(counts.value(), torch::kInt);
    TORCH_CHECK(counts->size(0) == B && counts->size(1) == V,
                "counts must be [B, V]");
    cnt = counts->data_ptr();
  }
  const void* sd = nullptr;
  if (seeds.has_value()) {
    CHECK_IN(seeds.value(), torch::kLong);
    sd = seeds->data_ptr();
  }
  const void* ct = nullptr;
  if (counter.has_value()) {
    CHECK_IN(counter.value(), torch::kLong);
    ct = counter->data_ptr();
  }
  auto out = torch::empty({B}, logits.options().dtype(torch::kLong));
  tl_sample(logits.data_ptr(), temps.data_ptr(), top_ps.data_ptr(),
            top_ks.data_ptr(), pres.data_ptr(), freqs.data_ptr(), cnt, sd,
            ct, out.data_ptr(), (uint64_t)seed_base, B, V, cur_stream());
  return out;
}

void bump_sample_counter(Tensor ctr) {
  CHECK_IN(ctr, torch::kLong);
  tl_bump_counter(ctr.data_ptr(), cur_stream());
}

Tensor moe_gemm(Tensor x, c10::optional<Tensor> tok_idx, Tensor seg_off,
                Tensor w_ptrs, c10::optional<Tensor> s_ptrs, int64_t N,
                bool fp8) {
  CHECK_IN(x, torch::kBFloat16);
  CHECK_IN(seg_off, torch::kInt);
  CHECK_IN(w_ptrs, torch::kLong);
  const int K = x.size(-1);
  TORCH_CHECK(K % 32 == 0 && N % 64 == 0, "unsupported MoE shape");
  const int E = w_ptrs.size(0);
  TORCH_CHECK(seg_off.size(0) == E + 1, "seg_off must be [E+1]");
  const void* ti = nullptr;
  int64_t P;
  if (tok_idx.has_value()) {
    CHECK_IN(tok_idx.value(), torch::kInt);
    ti = tok_idx->data_ptr();
    P = tok_idx->size(0);
  } else {
    P = x.size(0);
  }
  const void* sp = nullptr;
  if (fp8) {
    TORCH_CHECK(s_ptrs.has_value(), "fp8 needs scale pointers");
    CHECK_IN(s_ptrs.value(), torch::kLong);
    sp = s_ptrs->data_ptr();
  }
  auto out = torch::empty({P, N}, x.options());
  tl_moe_gemm(x.data_ptr(), ti, seg_off.data_ptr(), w_ptrs.data_ptr(), sp,
              out.data_ptr(), E, (int)N, K, fp8 ? 1 : 0, cur_stream());
  return out;
}

// x [T, K] bf16 (or [P, K] pair rows when tok_idx is absent); p_ptrs /
// e_ptrs: [E] int64 device addresses of each expert's packed [N, K/2]
// uint8 and exponents [N, K/32] int8 (16-byte aligned, contiguous: the
// caller's table builder asserts it, the addresses cannot be read here
// without a sync). n_split_override > 0 is for measurement only.
Tensor mxfp4_moe_gemm(Tensor x, c10::optional<Tensor> tok_idx,
                      Tensor seg_off, Tensor p_ptrs, Tensor e_ptrs,
                      int64_t N, int64_t n_split_override) {
  CHECK_IN(x, torch::kBFloat16);
  CHECK_IN(seg_off, torch::kInt);
  CHECK_IN(p_ptrs, torch::kLong);
  CHECK_IN(e_ptrs, torch::kLong);
  TORCH_CHECK(x.dim() == 2, "x must be [T, K]");
  const int64_t T = x.size(0);
  const int64_t K = x.size(1);
  TORCH_CHECK(K > 0 && N > 0 && N % 64 == 0 && K % 128 == 0,
              "unsupported shape: need N % 64 == 0 and K % 128 == 0");
  TORCH_CHECK(p_ptrs.dim() == 1 && e_ptrs.dim() == 1 &&
                  p_ptrs.size(0) == e_ptrs.size(0),
              "pointer tables must both be [E]");
  const int64_t E = p_ptrs.size(0);
  TORCH_CHECK(E >= 1 && E <= 65535, "need 1 <= E <= 65535");
  TORCH_CHECK(seg_off.dim() == 1 && seg_off.size(0) == E + 1,
              "seg_off must be [E+1]");
  TORCH_CHECK(seg_off.device() == x.device() &&
                  p_ptrs.device() == x.device() &&
                  e_ptrs.device() == x.device(),
              "operands must share a device");
  const void* ti = nullptr;
  int64_t P = T;
  if (tok_idx.has_value()) {
    CHECK_IN(tok_idx.value(), torch::kInt);
    TORCH_CHECK(tok_idx->dim() == 1, "tok_idx must be [P]");
    TORCH_CHECK(tok_idx->device() == x.device(),
                "operands must share a device");
    ti = tok_idx->data_ptr();
    P = tok_idx->size(0);
  }
  TORCH_CHECK(P * N < (int64_t)1 << 31 && T * K < (int64_t)1 << 40,
              "mxfp4_moe_gemm: call too large");
  auto out = torch::empty({P, N}, x.options());
  if (P == 0) return out;
  TORCH_CHECK(T >= 1, "x has no rows");
  const int n_split = n_split_override > 0
                          ? (int)n_split_override
                          : mxfp4_moe_n_split((int)N, (int)K, (int)E);
  TORCH_CHECK(n_split >= 1 && n_split <= 8, "bad split count");
  Tensor partial;
  void* pp = nullptr;
  if (n_split > 1) {
    partial = torch::empty({(int64_t)n_split * P * N},
                           x.options().dtype(torch::kFloat));
    pp = partial.data_ptr();
  }
  tl_mxfp4_moe_gemm(x.data_ptr(), ti, seg_off.data_ptr(), p_ptrs.data_ptr(),
                    e_ptrs.data_ptr(), out.data_ptr(), pp, (int)T, (int)P,
                    (int)E, (int)N, (int)K, n_split, cur_stream());
  return out;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("rope_append_", &rope_append_,
          "fused RoPE + KV-cache append from fused-QKV rows");
  mod.def("swiglu_fused", &swiglu_fused, "silu-mul on fused [.,2I] rows");
  mod.def("skinny_gemm", &skinny_gemm, "decode-M GEMM: x @ W^T + bias");
  mod.def("gemm_n_split", &gemm_n_split,
          "split-K count the GEMM family's (N,K)-only policy gives");
  mod.def("gemm_k_slices", &gemm_k_slices,
          "[(begin, end)] of each split-K slice the GEMM family takes");
  mod.def("gemm_colbal", &gemm_colbal,
          "column-balanced one-pass GEMM: x @ W^T (n_split == 1 shapes)",
          py::arg("x"), py::arg("w"), py::arg("n_blocks") = 0);
  mod.def("gemm_colbal_swiglu", &gemm_colbal_swiglu,
          "column-balanced gate_up GEMM with SwiGLU on the accumulators",
          py::arg("x"), py::arg("w_gate_up"), py::arg("n_blocks") = 0);
  mod.def("lm_head_argmax", &lm_head_argmax,
          "fused greedy head: argmax of bf16(x @ W^T) without the logits");
  mod.def("head_ce_stats", &head_ce_stats,
          "fused linear cross-entropy, forward: (lse, loss_row) per row",
          py::arg("x"), py::arg("w"), py::arg("labels"),
          py::arg("rows_per_launch") = 0, py::arg("rows_fast") = 1);
  mod.def("head_ce_grad", &head_ce_grad,
          "fused linear cross-entropy, backward: g = dloss/dlogits in bf16",
          py::arg("x"), py::arg("w"), py::arg("labels"), py::arg("lse"),
          py::arg("scale"), py::arg("rows_per_launch") = 0,
          py::arg("rows_fast") = 1, py::arg("out") = py::none());
  mod.def("skinny_gemm_partials", &skinny_gemm_partials,
          "decode-M GEMM handing out its fp32 split-K partials");
  mod.def("rmsnorm_add_fwd", &rmsnorm_add_fwd,
          "residual add + RMSNorm from bf16 or split-K partials");
  mod.def("rmsnorm_fwd", &rmsnorm_fwd, "fused RMSNorm fwd (+residual)");
  mod.def("rmsnorm_bwd", &rmsnorm_bwd, "RMSNorm bwd");
  mod.def("rope_", &rope_, "in-place RoPE apply");
  mod.def("swiglu_fwd", &swiglu_fwd, "silu(gate)*up");
  mod.def("swiglu_bwd", &swiglu_bwd, "SwiGLU bwd");
  mod.def("adamw_", &adamw_, "fused AdamW step");
  mod.def("decode_attn", &decode_attn, "GQA decode attention over KV cache");
  mod.def("prefill_attn", &prefill_attn, "causal GQA prefill attention");
  mod.def("sample_tokens", &sample_tokens,
          "fused penalties/temperature/top-k/top-p sampling, one block/row");
  mod.def("bump_sample_counter", &bump_sample_counter,
          "advance the graph-safe sampling RNG counter");
  mod.def("moe_gemm", &moe_gemm,
          "grouped expert GEMM over expert-sorted pair rows");
  mod.def("mxfp4_gemm", &mxfp4_gemm,
          "weight-only MXFP4 GEMM: x @ dequant(packed, exponents)^T + bias");
  mod.def("mxfp4_n_split", &mxfp4_n_split_py,
          "split-K count of mxfp4_gemm for (N, K)");
  mod.def("mxfp4_moe_gemm", &mxfp4_moe_gemm,
          "grouped MXFP4 expert GEMM over expert-sorted pair rows",
          pybind11::arg("x"), pybind11::arg("tok_idx"),
          pybind11::arg("seg_off"), pybind11::arg("p_ptrs"),
          pybind11::arg("e_ptrs"), pybind11::arg("N"),
          pybind11::arg("n_split_override") = 0);
  mod.def("mxfp4_moe_n_split", &mxfp4_moe_n_split_py,
          "split-K count of mxfp4_moe_gemm for (N, K, E)");
  mod.def("prefill_attn_lse", &prefill_attn_lse,
          "causal GQA prefill attention returning (out, logsumexp)");
  mod.def("prefill_attn_carry", &prefill_attn_carry,
          "prefill attention over one key chunk with carried (o, m, l) state",
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o_state"),
          py::arg("ml_state"), py::arg("scale"), py::arg("causal"),
          py::arg("q_off"), py::arg("first"), py::arg("last"),
          py::arg("want_lse") = false);
  mod.def("attn_bwd", &attn_bwd,
          "flash-attention backward: (dq, dk, dv) from saved lse/delta");
}
