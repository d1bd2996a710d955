// pybind11 bindings of the loss, elementwise, embedding, optimizer, LayerNorm and attention ops and the
// occupancy probes (the GEMM / convolution ops: conv.cpp; BatchNorm and pooling: bn.cpp).  Every entry point
// validates device / dtype / layout and fails loudly (no silent fallback) and enqueues on torch's current
// HIP stream, so the ops compose with the caching allocator and hipGraph
// capture (no host sync, no hipMalloc inside).
#include <algorithm>
#include <vector>

#include "ops_common.h"

namespace dpe_ops {
namespace {

// ------------------------------------------------------------------- loss
// returns (loss_rows [B] f32, loss_sum [1], correct [1], dlogits or empty)
std::vector<Tensor> cross_entropy(const Tensor& logits, const Tensor& labels, int64_t V, double grad_scale, bool want_grad,
                                  bool grad_bf16, int64_t ignore_index, bool inplace) {
  CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_CONTIG(labels);
  TORCH_CHECK(labels.scalar_type() == at::kLong, "labels must be int64");
  const bool in_bf16 = logits.scalar_type() == at::kBFloat16;
  TORCH_CHECK(in_bf16 || logits.scalar_type() == at::kFloat, "logits must be f32 or bf16");
  const int64_t ld = logits.size(-1), B = logits.numel() / ld;
  TORCH_CHECK(labels.numel() == B, "labels size mismatch");
  auto fo = logits.options().dtype(at::kFloat);
  Tensor rows = at::empty({B}, fo);
  Tensor sums = at::zeros({2}, fo);
  Tensor d;
  if (want_grad && inplace) {
    TORCH_CHECK(grad_bf16 == in_bf16, "cross_entropy: in-place gradient needs the logits dtype");
    d = logits;  // the row is held in registers: the gradient overwrites the logits
  } else if (want_grad) {
    d = at::empty(logits.sizes(), logits.options().dtype(grad_bf16 ? at::kBFloat16 : at::kFloat));
  }
  CHECK_RC(dpe_cross_entropy(logits.data_ptr(), in_bf16, (const int64_t*)labels.data_ptr(), (int)B, (int)V, ld,
                             (float)grad_scale, want_grad ? d.data_ptr() : nullptr, grad_bf16, fp(rows), fp(sums),
                             fp(sums) + 1, (int)ignore_index, cur_stream()), "cross_entropy");
  return {rows, sums.slice(0, 0, 1), sums.slice(0, 1, 2), d};
}

// Training form: (out4 = [loss_sum, correct, mean over non-ignored rows, 1 / their count], dlogits).  The
// mean and the backward scale come out of the reduction kernel itself (no torch count / clamp / divide
// launches at the forward -> backward seam).
// label_smoothing / z_loss (both 0: the plain kernels): see csrc/kernels/loss.hip.
// labels2 / mix_w (together): a second label per row (ignore_index: none) and the weight of the first one, a
// device fp32 tensor of 1 element (the batch's) or B (per row) that the kernels read -- the MIX kernels.
std::vector<Tensor> cross_entropy_mean(const Tensor& logits, const Tensor& labels, int64_t V, bool grad_bf16,
                                       int64_t ignore_index, bool inplace, double label_smoothing, double z_loss,
                                       const c10::optional<Tensor>& labels2, const c10::optional<Tensor>& mix_w) {
  CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_CONTIG(labels);
  TORCH_CHECK(labels.scalar_type() == at::kLong, "labels must be int64");
  const bool in_bf16 = logits.scalar_type() == at::kBFloat16;
  TORCH_CHECK(in_bf16 || logits.scalar_type() == at::kFloat, "logits must be f32 or bf16");
  const int64_t ld = logits.size(-1), B = logits.numel() / ld;
  TORCH_CHECK(labels.numel() == B, "labels size mismatch");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing < 1.0, "cross_entropy_mean: label_smoothing must be in [0, 1)");
  TORCH_CHECK(z_loss >= 0.0, "cross_entropy_mean: z_loss must be >= 0");
  auto fo = logits.options().dtype(at::kFloat);
  Tensor rows = at::empty({B}, fo);
  Tensor out4 = at::zeros({4}, fo);
  Tensor d;
  if (inplace) {
    TORCH_CHECK(grad_bf16 == in_bf16, "cross_entropy: in-place gradient needs the logits dtype");
    d = logits;
  } else {
    d = at::empty(logits.sizes(), logits.options().dtype(grad_bf16 ? at::kBFloat16 : at::kFloat));
  }
  TORCH_CHECK(has(labels2) == has(mix_w), "cross_entropy_mean: labels2 and mix_w go together");
  if (has(labels2)) {
    TORCH_CHECK(V > 0 && V <= ld, "cross_entropy_mean: V must be in [1, row length]");
    TORCH_CHECK(labels2->is_cuda() && labels2->device() == logits.device() && labels2->scalar_type() == at::kLong &&
                    labels2->is_contiguous() && labels2->numel() == B,
                "cross_entropy_mean: labels2 must be a contiguous int64 tensor of one label per row on the logits' device");
    TORCH_CHECK(labels.is_cuda() && labels.device() == logits.device(), "cross_entropy_mean: labels must be on the logits' device");
    TORCH_CHECK(mix_w->is_cuda() && mix_w->device() == logits.device() && mix_w->scalar_type() == at::kFloat &&
                    (mix_w->numel() == 1 || (mix_w->numel() == B && mix_w->is_contiguous())),
                "cross_entropy_mean: mix_w must be an fp32 tensor of 1 or B (contiguous) elements on the logits' device");
    CHECK_RC(dpe_cross_entropy_mean_mix(logits.data_ptr(), in_bf16, (const int64_t*)labels.data_ptr(),
                                        (const int64_t*)labels2->data_ptr(), fp(*mix_w), mix_w->numel() == 1 ? 0 : 1, (int)B,
                                        (int)V, ld, 1.f, d.data_ptr(), grad_bf16, fp(rows), fp(out4), (int)ignore_index,
                                        (float)label_smoothing, (float)z_loss, cur_stream()),
             "cross_entropy_mean");
  } else if (label_smoothing == 0.0 && z_loss == 0.0) {
    CHECK_RC(dpe_cross_entropy_mean(logits.data_ptr(), in_bf16, (const int64_t*)labels.data_ptr(), (int)B, (int)V, ld, 1.f,
                                    d.data_ptr(), grad_bf16, fp(rows), fp(out4), (int)ignore_index, cur_stream()),
             "cross_entropy_mean");
  } else {
    TORCH_CHECK(V > 0 && V <= ld, "cross_entropy_mean: V must be in [1, row length]");
    CHECK_RC(dpe_cross_entropy_mean_reg(logits.data_ptr(), in_bf16, (const int64_t*)labels.data_ptr(), (int)B, (int)V, ld, 1.f,
                                        d.data_ptr(), grad_bf16, fp(rows), fp(out4), (int)ignore_index,
                                        (float)label_smoothing, (float)z_loss, cur_stream()),
             "cross_entropy_mean");
  }
  return {out4, d};
}

// d * g * inv_n (g, inv_n: one-element fp32 device tensors) in the dtype of d
Tensor ce_grad_scale(const Tensor& d, const Tensor& g, const Tensor& inv_n) {
  CHECK_GPU(d); CHECK_CONTIG(d); CHECK_F32(g); CHECK_F32(inv_n);
  const bool bf = d.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf || d.scalar_type() == at::kFloat, "ce_grad_scale: f32 or bf16");
  TORCH_CHECK(g.numel() == 1 && inv_n.numel() == 1 && g.is_cuda() && inv_n.is_cuda(), "ce_grad_scale: device scalars");
  Tensor o = at::empty_like(d);
  CHECK_RC(dpe_ce_grad_scale(d.data_ptr(), o.data_ptr(), d.numel(), bf ? 1 : 0, fp(g.contiguous()), fp(inv_n.contiguous()),
                             cur_stream()),
           "ce_grad_scale");
  return o;
}

// ---------------------------------------------------------------- eltwise
Tensor cast_bf16(const Tensor& x, const c10::optional<Tensor>& out) {
  CHECK_GPU(x); CHECK_F32(x); CHECK_CONTIG(x);
  Tensor y = has(out) ? *out : at::empty(x.sizes(), x.options().dtype(at::kBFloat16));
  TORCH_CHECK(y.numel() == x.numel() && y.is_contiguous() && y.scalar_type() == at::kBFloat16, "cast_bf16: bad out");
  CHECK_RC(dpe_cast_f32_bf16(fp(x), bpm(y), x.numel(), cur_stream()), "cast");
  return y;
}

Tensor cast_f32(const Tensor& x) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_CONTIG(x);
  Tensor y = at::empty(x.sizes(), x.options().dtype(at::kFloat));
  CHECK_RC(dpe_cast_bf16_f32(bp(x), fp(y), x.numel(), cur_stream()), "cast");
  return y;
}

// op: 0 relu, 1 relu_bwd(dy, y), 2 gelu, 3 gelu_bwd(dy, x)
Tensor act(const Tensor& a, const c10::optional<Tensor>& b, int64_t op) {
  CHECK_GPU(a); CHECK_CONTIG(a);
  const bool bf = a.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf || a.scalar_type() == at::kFloat, "act: f32/bf16 only");
  Tensor out = at::empty_like(a);
  const void* bpv = has(b) ? b->data_ptr() : nullptr;
  if (op == 1 || op == 3) TORCH_CHECK(bpv && b->is_contiguous() && b->scalar_type() == a.scalar_type(), "act: second operand");
  CHECK_RC(dpe_act(a.data_ptr(), bpv, out.data_ptr(), a.numel(), (int)op, bf, cur_stream()), "act");
  return out;
}

Tensor dropout(const Tensor& x, double p, int64_t seed, int64_t offset) {
  CHECK_GPU(x); CHECK_CONTIG(x);
  const bool bf = x.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf || x.scalar_type() == at::kFloat, "dropout: f32/bf16 only");
  Tensor y = at::empty_like(x);
  CHECK_RC(dpe_dropout(x.data_ptr(), y.data_ptr(), x.numel(), (float)p, (uint64_t)seed, (uint64_t)offset, bf, cur_stream()),
           "dropout");
  return y;
}

// rng: the device dropout state, int64[2] (seed, offset), read by the kernels
const int64_t* rng_ptr(const Tensor& rng, const Tensor& like, const char* what) {
  TORCH_CHECK(rng.is_cuda() && rng.device() == like.device() && rng.scalar_type() == at::kLong && rng.dim() == 1 &&
                  rng.numel() == 2 && rng.is_contiguous(),
              what, ": rng must be a contiguous int64[2] tensor on the input's device");
  return (const int64_t*)rng.data_ptr();
}

Tensor dropout_add(const Tensor& res, const Tensor& y, double p, const Tensor& rng, int64_t stream,
                   const c10::optional<Tensor>& out_) {
  CHECK_GPU(res); CHECK_F32(res); CHECK_CONTIG(res); CHECK_GPU(y); CHECK_CONTIG(y);
  const bool bf = y.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf || y.scalar_type() == at::kFloat, "dropout_add: y is f32 or bf16");
  TORCH_CHECK(y.numel() == res.numel() && y.device() == res.device(), "dropout_add: res and y differ in size or device");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_add: p must be in [0, 1), got ", p);
  TORCH_CHECK(stream >= 0 && stream <= 0xffffffffLL, "dropout_add: stream must fit 32 bits");
  Tensor out = has(out_) ? *out_ : at::empty_like(res);
  CHECK_GPU(out); CHECK_F32(out); CHECK_CONTIG(out);
  TORCH_CHECK(out.numel() == res.numel() && out.device() == res.device(), "dropout_add: out must have res's size and device");
  CHECK_RC(dpe_dropout_add(fp(res), y.data_ptr(), bf ? 1 : 0, fp(out), res.numel(), (float)p,
                           rng_ptr(rng, res, "dropout_add"), (uint32_t)stream, cur_stream()), "dropout_add");
  return out;
}

Tensor dropout_cast(const Tensor& g, double p, const Tensor& rng, int64_t stream, const c10::optional<Tensor>& out_) {
  CHECK_GPU(g); CHECK_F32(g); CHECK_CONTIG(g);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_cast: p must be in [0, 1), got ", p);
  TORCH_CHECK(stream >= 0 && stream <= 0xffffffffLL, "dropout_cast: stream must fit 32 bits");
  Tensor out = has(out_) ? *out_ : at::empty_like(g, g.options().dtype(at::kBFloat16));
  CHECK_GPU(out); CHECK_BF16(out); CHECK_CONTIG(out);
  TORCH_CHECK(out.numel() == g.numel() && out.device() == g.device(), "dropout_cast: out must have g's size and device");
  CHECK_RC(dpe_dropout_cast(fp(g), bpm(out), g.numel(), (float)p, rng_ptr(rng, g, "dropout_cast"),
                            (uint32_t)stream, cur_stream()), "dropout_cast");
  return out;
}

Tensor add(const Tensor& a, const Tensor& b, double alpha) {
  CHECK_GPU(a); CHECK_CONTIG(a); CHECK_CONTIG(b);
  TORCH_CHECK(a.scalar_type() == b.scalar_type() && a.numel() == b.numel(), "add: mismatch");
  const bool bf = a.scalar_type() == at::kBFloat16;
  Tensor out = at::empty_like(a);
  CHECK_RC(dpe_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), (float)alpha, bf, cur_stream()), "add");
  return out;
}

void colsum(const Tensor& dy, Tensor& db, bool accumulate) {
  CHECK_GPU(dy); CHECK_CONTIG(dy); CHECK_F32(db);
  const int64_t N = dy.size(-1), M = dy.numel() / N;
  const bool bf = dy.scalar_type() == at::kBFloat16;
  CHECK_RC(dpe_colsum(dy.data_ptr(), M, (int)N, N, fp(db), accumulate ? 1 : 0, bf, cur_stream()), "colsum");
}

Tensor nchw_to_nhwc(const Tensor& x, int64_t cpad) {
  CHECK_GPU(x); CHECK_F32(x); CHECK_CONTIG(x);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t Cp = std::max<int64_t>(C, cpad);
  Tensor y = at::empty({N, H, W, Cp}, x.options().dtype(at::kBFloat16));
  CHECK_RC(dpe_nchw_to_nhwc(fp(x), bpm(y), (int)N, (int)C, (int)(H * W), (int)Cp, cur_stream()), "nchw_to_nhwc");
  return y;
}

Tensor patchify(const Tensor& x, int64_t p) {
  CHECK_GPU(x); CHECK_F32(x); CHECK_CONTIG(x);
  TORCH_CHECK(x.dim() == 4, "patchify: x must be [N,C,H,W]");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(p >= 8 && p % 8 == 0 && H % p == 0 && W % p == 0, "patchify: patch must be a multiple of 8 that divides H and W");
  Tensor y = at::empty({N, (H / p) * (W / p), C * p * p}, x.options().dtype(at::kBFloat16));
  CHECK_RC(dpe_patchify(fp(x), bpm(y), (int)N, (int)C, (int)H, (int)W, (int)p, cur_stream()), "patchify");
  return y;
}

Tensor nchw_to_s2d(const Tensor& x) {
  CHECK_GPU(x); CHECK_F32(x); CHECK_CONTIG(x);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(C <= 4 && H % 2 == 0 && W % 2 == 0, "nchw_to_s2d: needs C <= 4 and even H, W");
  Tensor y = at::empty({N, H / 2, W / 2, 16}, x.options().dtype(at::kBFloat16));
  CHECK_RC(dpe_nchw_to_s2d(fp(x), bpm(y), (int)N, (int)C, (int)H, (int)W, cur_stream()), "nchw_to_s2d");
  return y;
}

// One mixing decision per row of `count`: [count, 8] fp32 rows [w_pix, w_lab, x1, y1, x2, y2, mode, lam_raw] drawn from
// the device state rng (int64[2] seed, offset; rows use offset, offset + 1, ...; the caller advances it by count).
Tensor mix_draw(const Tensor& rng, int64_t stream, int64_t H, int64_t W, double mixup_alpha, double cutmix_alpha, double prob,
                double switch_prob, int64_t count) {
  TORCH_CHECK(rng.is_cuda() && rng.scalar_type() == at::kLong && rng.dim() == 1 && rng.numel() == 2 && rng.is_contiguous(),
              "mix_draw: rng must be a contiguous int64[2] GPU tensor");
  TORCH_CHECK(stream >= 0 && stream <= 0xffffffffLL, "mix_draw: stream must fit 32 bits");
  TORCH_CHECK(H > 0 && W > 0 && H <= 65536 && W <= 65536, "mix_draw: H and W must be in [1, 65536]");
  TORCH_CHECK(count >= 1 && count <= (1 << 20), "mix_draw: count must be in [1, 2^20]");
  TORCH_CHECK(mixup_alpha >= 0.0 && cutmix_alpha >= 0.0, "mix_draw: alphas must be >= 0");
  TORCH_CHECK(prob >= 0.0 && prob <= 1.0 && switch_prob >= 0.0 && switch_prob <= 1.0, "mix_draw: probabilities must be in [0, 1]");
  Tensor out = at::empty({count, 8}, rng.options().dtype(at::kFloat));
  CHECK_RC(dpe_mix_draw((const int64_t*)rng.data_ptr(), (uint32_t)stream, (int)H, (int)W, (float)mixup_alpha, (float)cutmix_alpha,
                        (float)prob, (float)switch_prob, (int)count, fp(out), cur_stream()),
           "mix_draw");
  return out;
}

// x NCHW fp32 mixed with x.roll(1, 0) by the row `params` (8 fp32 on the device, read by the kernel) and packed:
// layout 0 space-to-depth [N,H/2,W/2,16] bf16, 1 NHWC bf16 padded to cpad channels.  `out`: a caller's buffer.
Tensor mix_pack(const Tensor& x, const Tensor& params, int64_t layout, int64_t cpad, const c10::optional<Tensor>& out_) {
  CHECK_GPU(x); CHECK_F32(x); CHECK_CONTIG(x);
  TORCH_CHECK(x.dim() == 4, "mix_pack: x must be NCHW");
  TORCH_CHECK(params.is_cuda() && params.device() == x.device() && params.scalar_type() == at::kFloat &&
                  params.numel() == 8 && params.is_contiguous(),
              "mix_pack: params must be 8 contiguous fp32 values on x's device");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(N >= 1 && C >= 1 && H >= 1 && W >= 1 && N <= 0x7fffffffLL && H * W <= 0x7fffffffLL, "mix_pack: bad shape");
  TORCH_CHECK(layout == 0 || layout == 1, "mix_pack: layout 0 (s2d) or 1 (nhwc)");
  std::vector<int64_t> shape;
  const int64_t Cp = std::max<int64_t>(C, cpad);
  if (layout == 0) {
    TORCH_CHECK(C <= 4 && H % 2 == 0 && W % 2 == 0, "mix_pack: the s2d layout needs C <= 4 and even H, W");
    shape = {N, H / 2, W / 2, 16};
  } else {
    shape = {N, H, W, Cp};
  }
  Tensor y = has(out_) ? *out_ : at::empty(shape, x.options().dtype(at::kBFloat16));
  CHECK_GPU(y); CHECK_BF16(y); CHECK_CONTIG(y);
  TORCH_CHECK(y.device() == x.device() && y.sizes().vec() == shape, "mix_pack: out must have the packed shape on x's device");
  CHECK_RC(dpe_mix_pack(fp(x), fp(params), bpm(y), (int)N, (int)C, (int)H, (int)W, (int)layout, (int)Cp, cur_stream()), "mix_pack");
  return y;
}

// an optional int32 GPU tensor of exactly n elements (position ids, document bounds); null when absent
const int32_t* i32_opt(const c10::optional<Tensor>& t, int64_t n, const Tensor& like, const char* what) {
  if (!has(t)) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->device() == like.device() && t->scalar_type() == at::kInt && t->is_contiguous() &&
                  t->numel() == n, what, " must be a contiguous int32 tensor of ", n, " elements on the inputs' device");
  return (const int32_t*)t->data_ptr();
}

Tensor embedding_fwd(const Tensor& idx, const Tensor& wte, const c10::optional<Tensor>& wpe,
                     const c10::optional<Tensor>& pos) {
  CHECK_GPU(idx); CHECK_CONTIG(idx); CHECK_BF16(wte); CHECK_CONTIG(wte);
  TORCH_CHECK(idx.scalar_type() == at::kLong && idx.dim() == 2, "embedding: idx must be int64 [B,T]");
  const int64_t B = idx.size(0), T = idx.size(1), D = wte.size(1);
  Tensor out = at::empty({B, T, D}, wte.options().dtype(at::kFloat));
  const uint16_t* pe = has(wpe) ? bp(*wpe) : nullptr;
  CHECK_RC(dpe_embedding_fwd((const int64_t*)idx.data_ptr(), bp(wte), pe, fp(out), B * T, (int)T, (int)D,
                             i32_opt(pos, B * T, idx, "embedding: pos"), cur_stream()),
           "embedding_fwd");
  return out;
}

void embedding_bwd(const Tensor& idx, const Tensor& dout, Tensor& dwte, const c10::optional<Tensor>& dwpe,
                   const c10::optional<Tensor>& pos) {
  CHECK_GPU(dout); CHECK_F32(dout); CHECK_CONTIG(dout); CHECK_F32(dwte);
  const int64_t B = idx.size(0), T = idx.size(1), D = dwte.size(1);
  CHECK_RC(dpe_embedding_bwd((const int64_t*)idx.data_ptr(), fp(dout), fp(dwte), fpom(dwpe), B * T, (int)T, (int)D,
                             i32_opt(pos, B * T, idx, "embedding: pos"), cur_stream()), "embedding_bwd");
}

// --------------------------------------------------------------- optimizer
void optim_step(int64_t kind, const Tensor& desc, const Tensor& chunks, const Tensor& hp, const Tensor& steps) {
  CHECK_GPU(desc); CHECK_GPU(chunks); CHECK_GPU(hp); CHECK_GPU(steps); CHECK_F32(hp); CHECK_F32(steps);
  TORCH_CHECK(chunks.scalar_type() == at::kInt && chunks.dim() == 2 && chunks.size(1) == 2, "chunks must be int32 [n,2]");
  CHECK_RC(dpe_optim_step((int)kind, desc.data_ptr(), chunks.data_ptr(), (int)chunks.size(0), fp(hp), fp(steps), cur_stream()),
           "optim_step");
}

static void check_optim_table(const Tensor& desc, const Tensor& chunks) {
  CHECK_GPU(desc); CHECK_GPU(chunks);
  TORCH_CHECK(chunks.scalar_type() == at::kInt && chunks.dim() == 2 && chunks.size(1) == 2, "chunks must be int32 [n,2]");
  TORCH_CHECK(chunks.is_contiguous() && desc.is_contiguous(), "optimizer table must be contiguous");
}

// Global gradient norm over the (tensor, chunk) table: out = [total_norm, coef, ok, skipped steps]; with `hp`
// (the optimizer's hyper-parameter rows, 12 floats per group) coef and ok also go into every row.
void optim_grad_norm(const Tensor& desc, const Tensor& chunks, Tensor& partials, Tensor& out, const Tensor& max_norm,
                     const c10::optional<Tensor>& hp, bool skip_nonfinite) {
  check_optim_table(desc, chunks);
  CHECK_GPU(partials); CHECK_F32(partials); CHECK_CONTIG(partials);
  CHECK_GPU(out); CHECK_F32(out); CHECK_CONTIG(out);
  CHECK_GPU(max_norm); CHECK_F32(max_norm);
  TORCH_CHECK(partials.numel() >= chunks.size(0), "optim_grad_norm: one partial per chunk");
  TORCH_CHECK(out.numel() >= 4 && max_norm.numel() >= 1, "optim_grad_norm: out needs 4 floats, max_norm 1");
  int ngroups = 0;
  if (hp.has_value()) {
    CHECK_GPU((*hp)); CHECK_F32((*hp)); CHECK_CONTIG((*hp));
    TORCH_CHECK(hp->numel() % 12 == 0, "optim_grad_norm: hp holds 12 floats per group");
    ngroups = (int)(hp->numel() / 12);
  }
  CHECK_RC(dpe_optim_grad_norm(desc.data_ptr(), chunks.data_ptr(), (int)chunks.size(0), fp(partials), fp(out), fp(max_norm),
                               fpom(hp), ngroups, skip_nonfinite ? 1 : 0, cur_stream()),
           "optim_grad_norm");
}

// In-place g *= out[1] (the coef optim_grad_norm left) over the table's gradients.
void optim_grad_scale(const Tensor& desc, const Tensor& chunks, const Tensor& out) {
  check_optim_table(desc, chunks);
  CHECK_GPU(out); CHECK_F32(out); CHECK_CONTIG(out);
  TORCH_CHECK(out.numel() >= 4, "optim_grad_scale: out needs 4 floats");
  CHECK_RC(dpe_optim_grad_scale(desc.data_ptr(), chunks.data_ptr(), (int)chunks.size(0), fp(out), cur_stream()),
           "optim_grad_scale");
}

// The finishing kernel of optim_grad_norm alone, on `partials` that optim_trust_partials(kind 0) wrote.
void optim_clip_coef(const Tensor& partials, int64_t nchunks, Tensor& out, const Tensor& max_norm, Tensor& hp,
                     bool skip_nonfinite) {
  CHECK_GPU(partials); CHECK_F32(partials); CHECK_CONTIG(partials);
  CHECK_GPU(out); CHECK_F32(out); CHECK_CONTIG(out);
  CHECK_GPU(max_norm); CHECK_F32(max_norm);
  CHECK_GPU(hp); CHECK_F32(hp); CHECK_CONTIG(hp);
  TORCH_CHECK(nchunks >= 0 && partials.numel() >= nchunks, "optim_clip_coef: one partial per chunk");
  TORCH_CHECK(out.numel() >= 4 && max_norm.numel() >= 1, "optim_clip_coef: out needs 4 floats, max_norm 1");
  TORCH_CHECK(hp.numel() % 12 == 0, "optim_clip_coef: hp holds 12 floats per group");
  CHECK_RC(dpe_optim_clip_coef(fp(partials), (int)nchunks, fp(out), fp(max_norm), fp(hp), (int)(hp.numel() / 12),
                               skip_nonfinite ? 1 : 0, cur_stream()),
           "optim_clip_coef");
}

// The scheduled lr of this step into every group's hp row and `cur`; the device counter sched[0] advances by
// the step's ok flag.  sched: fp64 [optim_sched_header() + n_groups] (csrc/kernels/optim.hip).
void optim_lr_schedule(Tensor& hp, Tensor& sched, Tensor& cur) {
  CHECK_GPU(hp); CHECK_F32(hp); CHECK_CONTIG(hp);
  CHECK_GPU(sched); CHECK_CONTIG(sched);
  CHECK_GPU(cur); CHECK_F32(cur); CHECK_CONTIG(cur);
  TORCH_CHECK(sched.scalar_type() == at::kDouble, "optim_lr_schedule: sched is fp64");
  TORCH_CHECK(hp.numel() > 0 && hp.numel() % 12 == 0, "optim_lr_schedule: hp holds 12 floats per group");
  const int64_t ng = hp.numel() / 12;
  TORCH_CHECK(sched.numel() == dpe_optim_sched_header() + ng, "optim_lr_schedule: sched holds the header and one base lr per group");
  TORCH_CHECK(cur.numel() == ng, "optim_lr_schedule: cur holds one lr per group");
  CHECK_RC(dpe_optim_lr_schedule(fp(hp), (int)ng, (double*)sched.data_ptr(), fp(cur), cur_stream()), "optim_lr_schedule");
}

// LARS / LAMB (kind 0 / 1): the table checks of the other entry points plus the sizes of what the trust
// kernels index per chunk (partials) and per tensor (first_chunk, stats).
static int64_t check_trust_args(const char* what, const Tensor& desc, const Tensor& hp, const Tensor* steps_or_null,
                                const Tensor& part_w, const Tensor& part_x, int64_t nchunks) {
  CHECK_GPU(hp); CHECK_F32(hp); CHECK_CONTIG(hp);
  CHECK_GPU(part_w); CHECK_F32(part_w); CHECK_CONTIG(part_w);
  CHECK_GPU(part_x); CHECK_F32(part_x); CHECK_CONTIG(part_x);
  const int64_t db = dpe_optim_desc_bytes();
  TORCH_CHECK(desc.scalar_type() == at::kByte && desc.numel() % db == 0, what, ": desc is a byte tensor of whole TensorDescs");
  const int64_t nt = desc.numel() / db;
  TORCH_CHECK(hp.numel() >= 12 && hp.numel() % 12 == 0, what, ": hp holds 12 floats per group");
  if (steps_or_null != nullptr) {
    const Tensor& steps = *steps_or_null;
    CHECK_GPU(steps); CHECK_F32(steps); CHECK_CONTIG(steps);
    TORCH_CHECK(steps.numel() >= nt, what, ": one step counter per tensor");
  }
  TORCH_CHECK(part_w.numel() >= nchunks && part_x.numel() >= nchunks, what, ": one partial per chunk in both arrays");
  return nt;
}

void optim_trust_partials(int64_t kind, const Tensor& desc, const Tensor& chunks, const Tensor& hp, const Tensor& steps,
                          Tensor& part_w, Tensor& part_x) {
  TORCH_CHECK(kind == 0 || kind == 1, "optim_trust_partials: kind 0 (LARS) or 1 (LAMB)");
  check_optim_table(desc, chunks);
  check_trust_args("optim_trust_partials", desc, hp, &steps, part_w, part_x, chunks.size(0));
  CHECK_RC(dpe_optim_trust_partials((int)kind, desc.data_ptr(), chunks.data_ptr(), (int)chunks.size(0), fp(hp), fp(steps),
                                    fp(part_w), fp(part_x), cur_stream()),
           "optim_trust_partials");
}

void optim_trust_ratio(int64_t kind, const Tensor& desc, const Tensor& first_chunk, int64_t nchunks, const Tensor& part_w,
                       const Tensor& part_x, const Tensor& hp, Tensor& stats) {
  TORCH_CHECK(kind == 0 || kind == 1, "optim_trust_ratio: kind 0 (LARS) or 1 (LAMB)");
  CHECK_GPU(desc); CHECK_CONTIG(desc);
  CHECK_GPU(first_chunk); CHECK_CONTIG(first_chunk);
  CHECK_GPU(stats); CHECK_F32(stats); CHECK_CONTIG(stats);
  TORCH_CHECK(nchunks >= 0, "optim_trust_ratio: nchunks");
  const int64_t nt = check_trust_args("optim_trust_ratio", desc, hp, nullptr, part_w, part_x, nchunks);
  TORCH_CHECK(first_chunk.scalar_type() == at::kInt && first_chunk.numel() == nt + 1,
              "optim_trust_ratio: first_chunk is int32 [n_tensors + 1]");
  TORCH_CHECK(stats.numel() >= 3 * nt, "optim_trust_ratio: stats holds 3 floats per tensor");
  CHECK_RC(dpe_optim_trust_ratio((int)kind, desc.data_ptr(), (int)nt, (const int*)first_chunk.data_ptr(), (int)nchunks,
                                 fp(part_w), fp(part_x), fp(hp), fp(stats), cur_stream()),
           "optim_trust_ratio");
}

void optim_trust_step(int64_t kind, const Tensor& desc, const Tensor& chunks, const Tensor& hp, const Tensor& steps,
                      const Tensor& stats) {
  TORCH_CHECK(kind == 0 || kind == 1, "optim_trust_step: kind 0 (LARS) or 1 (LAMB)");
  check_optim_table(desc, chunks);
  CHECK_GPU(stats); CHECK_F32(stats); CHECK_CONTIG(stats);
  const int64_t nt = check_trust_args("optim_trust_step", desc, hp, &steps, stats, stats, 0);
  TORCH_CHECK(stats.numel() >= 3 * nt, "optim_trust_step: stats holds 3 floats per tensor");
  CHECK_RC(dpe_optim_trust_step((int)kind, desc.data_ptr(), chunks.data_ptr(), (int)chunks.size(0), fp(hp), fp(steps), fp(stats),
                                cur_stream()),
           "optim_trust_step");
}

// The weight EMA.  `ema`: int64 [n_tensors] on the device, the fp32 average of every tensor of the table (raw
// pointers, in table order); `blk`: fp64 [3] n, decay, warm-up; `cur`: fp32 [1], the d_n of the last step.
static int64_t check_ema_ptrs(const char* what, const Tensor& desc, const Tensor& ema) {
  CHECK_GPU(ema); CHECK_CONTIG(ema);
  const int64_t db = dpe_optim_desc_bytes();
  TORCH_CHECK(desc.scalar_type() == at::kByte && desc.numel() % db == 0, what, ": desc is a byte tensor of whole TensorDescs");
  TORCH_CHECK(ema.scalar_type() == at::kLong && ema.numel() == desc.numel() / db, what, ": ema is int64 [n_tensors]");
  return desc.numel() / db;
}

void optim_step_ema(int64_t kind, const Tensor& desc, const Tensor& chunks, const Tensor& hp, const Tensor& steps,
                    const Tensor& ema) {
  TORCH_CHECK(kind == 0 || kind == 1, "optim_step_ema: kind 0 (Adam) or 1 (SGD)");
  check_optim_table(desc, chunks);
  CHECK_GPU(hp); CHECK_F32(hp); CHECK_CONTIG(hp); CHECK_GPU(steps); CHECK_F32(steps); CHECK_CONTIG(steps);
  TORCH_CHECK(hp.numel() >= 12 && hp.numel() % 12 == 0, "optim_step_ema: hp holds 12 floats per group");
  const int64_t nt = check_ema_ptrs("optim_step_ema", desc, ema);
  TORCH_CHECK(steps.numel() >= nt, "optim_step_ema: one step counter per tensor");
  CHECK_RC(dpe_optim_step_ema((int)kind, desc.data_ptr(), chunks.data_ptr(), (int)chunks.size(0), fp(hp), fp(steps),
                              ema.data_ptr(), cur_stream()),
           "optim_step_ema");
}

void optim_trust_step_ema(int64_t kind, const Tensor& desc, const Tensor& chunks, const Tensor& hp, const Tensor& steps,
                          const Tensor& stats, const Tensor& ema) {
  TORCH_CHECK(kind == 0 || kind == 1, "optim_trust_step_ema: kind 0 (LARS) or 1 (LAMB)");
  check_optim_table(desc, chunks);
  CHECK_GPU(stats); CHECK_F32(stats); CHECK_CONTIG(stats);
  const int64_t nt = check_trust_args("optim_trust_step_ema", desc, hp, &steps, stats, stats, 0);
  TORCH_CHECK(stats.numel() >= 3 * nt, "optim_trust_step_ema: stats holds 3 floats per tensor");
  check_ema_ptrs("optim_trust_step_ema", desc, ema);
  CHECK_RC(dpe_optim_trust_step_ema((int)kind, desc.data_ptr(), chunks.data_ptr(), (int)chunks.size(0), fp(hp), fp(steps),
                                    fp(stats), ema.data_ptr(), cur_stream()),
           "optim_trust_step_ema");
}

// 1 - d_n into slot 11 of every hp row and d_n into cur[0]; the device counter blk[0] advances by the step's ok flag.
void optim_ema_decay(Tensor& hp, Tensor& blk, Tensor& cur) {
  CHECK_GPU(hp); CHECK_F32(hp); CHECK_CONTIG(hp);
  CHECK_GPU(blk); CHECK_CONTIG(blk);
  CHECK_GPU(cur); CHECK_F32(cur); CHECK_CONTIG(cur);
  TORCH_CHECK(blk.scalar_type() == at::kDouble && blk.numel() == 3, "optim_ema_decay: blk is fp64 [3]");
  TORCH_CHECK(hp.numel() > 0 && hp.numel() % 12 == 0, "optim_ema_decay: hp holds 12 floats per group");
  TORCH_CHECK(cur.numel() >= 1, "optim_ema_decay: cur holds one float");
  CHECK_RC(dpe_optim_ema_decay(fp(hp), (int)(hp.numel() / 12), (double*)blk.data_ptr(), fp(cur), cur_stream()),
           "optim_ema_decay");
}

// w <-> ema over the table, and the bf16 shadows of the new w.
void optim_ema_swap(const Tensor& desc, const Tensor& chunks, const Tensor& ema) {
  check_optim_table(desc, chunks);
  check_ema_ptrs("optim_ema_swap", desc, ema);
  CHECK_RC(dpe_optim_ema_swap(desc.data_ptr(), chunks.data_ptr(), (int)chunks.size(0), ema.data_ptr(), cur_stream()),
           "optim_ema_swap");
}

// -------------------------------------------------------------- LayerNorm
// x [rows, D] (f32 or bf16) -> y bf16, mean/rstd f32 [rows]
std::vector<Tensor> layernorm_fwd(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b, double eps) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_F32(w);
  const bool xb = x.scalar_type() == at::kBFloat16;
  TORCH_CHECK(xb || x.scalar_type() == at::kFloat, "layernorm: f32/bf16 input");
  const int64_t D = x.size(-1), rows = x.numel() / D;
  TORCH_CHECK(D % 8 == 0 && D <= 8192, "layernorm: D must be a multiple of 8 and <= 8192");
  Tensor y = at::empty(x.sizes(), x.options().dtype(at::kBFloat16));
  Tensor mean = at::empty({rows}, x.options().dtype(at::kFloat));
  Tensor rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  CHECK_RC(dpe_layernorm_fwd(x.data_ptr(), xb, fp(w), fpo(b), bpm(y), fp(mean), fp(rstd), rows, (int)D, (float)eps,
                             cur_stream()), "layernorm_fwd");
  return {y, mean, rstd};
}

// dx: if dx_out (f32) given, dx is ACCUMULATED into it (residual stream); else a new tensor of x's dtype
Tensor layernorm_bwd(const Tensor& dy, const Tensor& x, const Tensor& w, const Tensor& mean, const Tensor& rstd, Tensor& dw,
                     const c10::optional<Tensor>& db, const c10::optional<Tensor>& dx_out) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_CONTIG(dy); CHECK_CONTIG(x); CHECK_F32(dw);
  const bool xb = x.scalar_type() == at::kBFloat16;
  const int64_t D = x.size(-1), rows = x.numel() / D;
  Tensor dx;
  bool acc = false;
  if (has(dx_out)) {
    dx = *dx_out;
    CHECK_F32(dx); CHECK_CONTIG(dx);
    acc = true;
  } else {
    dx = at::empty_like(x);
  }
  Tensor part = at::empty({dpe_layernorm_bwd_scratch(rows, (int)D)}, x.options().dtype(at::kFloat));
  CHECK_RC(dpe_layernorm_bwd(bp(dy), x.data_ptr(), xb, fp(w), fp(mean), fp(rstd), dx.data_ptr(), acc ? 1 : 0, nullptr,
                             nullptr, fp(dw), fpom(db), fp(part), rows, (int)D, cur_stream()), "layernorm_bwd");
  return dx;
}

// Residual-stream form (pre-LN transformer block): dx = res_in + dLN(dy) in fp32 (a new tensor,
// res_in untouched) plus its bf16 copy for the next data/weight-grad GEMMs -- one pass instead of
// LN-bwd + add + cast.
// defer: dw / db are not touched; the third output is the [nblocks][2][D] partial scratch, finalized into
// dw / db later by layernorm_bwd_finalize_group (several LayerNorms per launch).
std::vector<Tensor> layernorm_bwd_residual(const Tensor& dy, const Tensor& x, const Tensor& w, const Tensor& mean,
                                           const Tensor& rstd, Tensor& dw, const c10::optional<Tensor>& db,
                                           const Tensor& res_in, bool defer) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_CONTIG(dy); CHECK_CONTIG(x); CHECK_F32(dw);
  CHECK_F32(res_in); CHECK_CONTIG(res_in);
  const bool xb = x.scalar_type() == at::kBFloat16;
  const int64_t D = x.size(-1), rows = x.numel() / D;
  TORCH_CHECK(res_in.numel() == x.numel(), "layernorm_bwd_residual: res_in shape mismatch");
  Tensor dx = at::empty(x.sizes(), x.options().dtype(at::kFloat));
  Tensor dxb = at::empty(x.sizes(), x.options().dtype(at::kBFloat16));
  Tensor part = at::empty({dpe_layernorm_bwd_scratch(rows, (int)D)}, x.options().dtype(at::kFloat));
  CHECK_RC(dpe_layernorm_bwd(bp(dy), x.data_ptr(), xb, fp(w), fp(mean), fp(rstd), dx.data_ptr(), 1, fp(res_in), bpm(dxb),
                             defer ? nullptr : fp(dw), defer ? nullptr : fpom(db), fp(part), rows, (int)D, cur_stream()),
           "layernorm_bwd_residual");
  if (defer) return {dx, dxb, part};
  return {dx, dxb};
}

// The deferred LayerNorm-backward finalizes: dw_i (+)= sum of part_i's dw partials (db_i likewise, when
// given), rows_i = the LayerNorm's row count; at most 8 per call.
void layernorm_bwd_finalize_group(const std::vector<Tensor>& parts, const std::vector<int64_t>& rows,
                                  const std::vector<Tensor>& dws, const std::vector<c10::optional<Tensor>>& dbs) {
  const size_t n = parts.size();
  TORCH_CHECK(n >= 1 && n <= 8 && rows.size() == n && dws.size() == n && dbs.size() == n,
              "layernorm_bwd_finalize_group: 1..8 problems, equal list lengths");
  std::vector<const float*> pp(n);
  std::vector<float*> pw(n), pb(n);
  std::vector<int> Ds(n);
  for (size_t i = 0; i < n; ++i) {
    CHECK_GPU(parts[i]); CHECK_F32(parts[i]); CHECK_F32(dws[i]); CHECK_CONTIG(dws[i]);
    const int64_t D = dws[i].numel();
    TORCH_CHECK(D > 0 && D % 8 == 0 && parts[i].numel() >= (int64_t)dpe_layernorm_bwd_nblocks(rows[i]) * 2 * D,
                "layernorm_bwd_finalize_group: partial scratch too small for rows / D");
    pp[i] = fp(parts[i]);
    pw[i] = fp(dws[i]);
    pb[i] = fpom(dbs[i]);
    if (pb[i]) TORCH_CHECK(dbs[i]->numel() == D, "layernorm_bwd_finalize_group: db size");
    Ds[i] = (int)D;
  }
  CHECK_RC(dpe_layernorm_bwd_finalize_group(pp.data(), rows.data(), Ds.data(), pw.data(), pb.data(), (int)n, cur_stream()),
           "layernorm_bwd_finalize_group");
}

// ---------------------------------------------------------------- attention
// qkv: [B, T, 3, H, D] bf16 -> out [B, T, H, D] bf16, lse [B, H, T] f32 (both optionally caller-allocated).
// doc_start / doc_end (int32 [B, T], together): the packed-document mask doc_start[b, i] <= j <= i.
// dropout_p > 0: dropout on P inside the kernels at the 8-bit rate thr / 256, thr = clamp(round(256 p), 1, 255); rng is
// the device int64[2] (seed, offset) the kernels read, stream the call site (Philox counter_lo).  0 = today's kernels.
const int64_t* drop_rng(double p, const c10::optional<Tensor>& rng, int64_t stream, const Tensor& like, uint32_t* thr) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, "attn: dropout_p must be in [0, 1), got ", p);
  TORCH_CHECK(stream >= 0 && stream <= 0xffffffffLL, "attn: stream must fit 32 bits");
  *thr = 0;
  if (p == 0.0) return nullptr;
  TORCH_CHECK(has(rng), "attn: dropout_p > 0 needs rng (device int64[2]: seed, offset)");
  TORCH_CHECK(rng->is_cuda() && rng->device() == like.device(), "attn: rng must be on qkv's device");
  TORCH_CHECK(rng->scalar_type() == at::kLong && rng->dim() == 1 && rng->numel() == 2 && rng->is_contiguous(),
              "attn: rng must be a contiguous int64[2] tensor");
  *thr = (uint32_t)std::min(255.0, std::max(1.0, std::floor(256.0 * p + 0.5)));
  return (const int64_t*)rng->data_ptr();
}

// causal = false: bidirectional attention over the first seq_len rows (0 = T); no doc_start, no dropout.
void bidir_args(const c10::optional<Tensor>& doc_start, const c10::optional<Tensor>& doc_end, double dropout_p,
                const c10::optional<Tensor>& rng, int64_t seq_len, int64_t T) {
  TORCH_CHECK(!has(doc_start) && !has(doc_end), "attn: causal=False takes no doc_start / doc_end");
  TORCH_CHECK(dropout_p == 0.0 && !has(rng), "attn: causal=False takes no dropout arguments");
  TORCH_CHECK(seq_len >= 0 && seq_len <= T, "attn: seq_len must be in [1, T] (0 = T), got ", seq_len);
}

std::vector<Tensor> attn_fwd(const Tensor& qkv, int64_t H, double scale, bool causal, const c10::optional<Tensor>& out_,
                             const c10::optional<Tensor>& lse_, const c10::optional<Tensor>& doc_start,
                             const c10::optional<Tensor>& doc_end, double dropout_p, const c10::optional<Tensor>& rng,
                             int64_t stream, int64_t seq_len) {
  CHECK_GPU(qkv); CHECK_BF16(qkv); CHECK_CONTIG(qkv);
  const int64_t B = qkv.size(0), T = qkv.size(1), D = qkv.size(-1);
  TORCH_CHECK(qkv.numel() == B * T * 3 * H * D, "attn: qkv must be [B,T,3,H,D]");
  TORCH_CHECK(D == 64, "attn: head dim 64 supported");
  Tensor out = has(out_) ? *out_ : at::empty({B, T, H, D}, qkv.options());
  Tensor lse = has(lse_) ? *lse_ : at::empty({B, H, T}, qkv.options().dtype(at::kFloat));
  CHECK_GPU(out); CHECK_BF16(out); CHECK_CONTIG(out); CHECK_GPU(lse); CHECK_F32(lse); CHECK_CONTIG(lse);
  TORCH_CHECK(out.numel() == B * T * H * D && lse.numel() == B * H * T, "attn_fwd: out is [B,T,H,D], lse [B,H,T]");
  TORCH_CHECK(has(doc_start) == has(doc_end), "attn_fwd: doc_start and doc_end go together");
  if (!causal) {
    bidir_args(doc_start, doc_end, dropout_p, rng, seq_len, T);
    CHECK_RC(dpe_attn_fwd_bidir(bp(qkv), bpm(out), fp(lse), (int)B, (int)T, (int)H, (int)D, (float)scale,
                                (int)(seq_len ? seq_len : T), cur_stream()),
             "attn_fwd (bidirectional: LDS-DMA kernels only)");
    return {out, lse};
  }
  TORCH_CHECK(seq_len == 0, "attn: seq_len goes with causal=False");
  uint32_t thr;
  if (const int64_t* rp = drop_rng(dropout_p, rng, stream, qkv, &thr)) {
    CHECK_RC(dpe_attn_fwd_drop(bp(qkv), bpm(out), fp(lse), (int)B, (int)T, (int)H, (int)D, (float)scale, causal,
                               i32_opt(doc_start, B * T, qkv, "attn_fwd: doc_start"),
                               i32_opt(doc_end, B * T, qkv, "attn_fwd: doc_end"), rp, (uint32_t)stream, thr, cur_stream()),
             "attn_fwd (dropout: LDS-DMA kernels only)");
    return {out, lse};
  }
  CHECK_RC(dpe_attn_fwd(bp(qkv), bpm(out), fp(lse), (int)B, (int)T, (int)H, (int)D, (float)scale, causal,
                        i32_opt(doc_start, B * T, qkv, "attn_fwd: doc_start"),
                        i32_opt(doc_end, B * T, qkv, "attn_fwd: doc_end"), cur_stream()),
           "attn_fwd");
  return {out, lse};
}

Tensor attn_bwd(const Tensor& qkv, const Tensor& out, const Tensor& dout, const Tensor& lse, int64_t H, double scale,
                bool causal, const c10::optional<Tensor>& dqkv_, const c10::optional<Tensor>& doc_start,
                const c10::optional<Tensor>& doc_end, double dropout_p, const c10::optional<Tensor>& rng, int64_t stream,
                int64_t seq_len) {
  CHECK_GPU(qkv); CHECK_BF16(dout); CHECK_CONTIG(dout); CHECK_CONTIG(out);
  const int64_t B = qkv.size(0), T = qkv.size(1), D = qkv.size(-1);
  Tensor dqkv = has(dqkv_) ? *dqkv_ : at::empty_like(qkv);
  CHECK_GPU(dqkv); CHECK_BF16(dqkv); CHECK_CONTIG(dqkv);
  TORCH_CHECK(dqkv.numel() == qkv.numel(), "attn_bwd: dqkv must have qkv's size");
  Tensor delta = at::empty({B, H, T}, qkv.options().dtype(at::kFloat));
  TORCH_CHECK(has(doc_start) == has(doc_end), "attn_bwd: doc_start and doc_end go together");
  if (!causal) {
    bidir_args(doc_start, doc_end, dropout_p, rng, seq_len, T);
    CHECK_RC(dpe_attn_bwd_bidir(bp(qkv), bp(out), bp(dout), fp(lse), fp(delta), bpm(dqkv), (int)B, (int)T, (int)H, (int)D,
                                (float)scale, (int)(seq_len ? seq_len : T), cur_stream()),
             "attn_bwd (bidirectional: LDS-DMA kernels only)");
    return dqkv;
  }
  TORCH_CHECK(seq_len == 0, "attn: seq_len goes with causal=False");
  uint32_t thr;
  if (const int64_t* rp = drop_rng(dropout_p, rng, stream, qkv, &thr)) {
    CHECK_RC(dpe_attn_bwd_drop(bp(qkv), bp(out), bp(dout), fp(lse), fp(delta), bpm(dqkv), (int)B, (int)T, (int)H, (int)D,
                               (float)scale, causal, i32_opt(doc_start, B * T, qkv, "attn_bwd: doc_start"),
                               i32_opt(doc_end, B * T, qkv, "attn_bwd: doc_end"), rp, (uint32_t)stream, thr, cur_stream()),
             "attn_bwd (dropout: LDS-DMA kernels only)");
    return dqkv;
  }
  CHECK_RC(dpe_attn_bwd(bp(qkv), bp(out), bp(dout), fp(lse), fp(delta), nullptr, bpm(dqkv), (int)B, (int)T, (int)H, (int)D,
                        (float)scale, causal, i32_opt(doc_start, B * T, qkv, "attn_bwd: doc_start"),
                        i32_opt(doc_end, B * T, qkv, "attn_bwd: doc_end"), cur_stream()), "attn_bwd");
  return dqkv;
}

}  // namespace

void register_ops(pybind11::module& m) {
  namespace py = pybind11;
  m.def("cross_entropy_mean", &cross_entropy_mean, py::arg("logits"), py::arg("labels"), py::arg("V"),
        py::arg("grad_bf16"), py::arg("ignore_index") = -100, py::arg("inplace") = false, py::arg("label_smoothing") = 0.0,
        py::arg("z_loss") = 0.0, py::arg("labels2") = py::none(), py::arg("mix_w") = py::none(),
        "training CE: (out4 = [sum, correct, mean, 1/n_valid], d loss_row / d logits), optionally label-smoothed / with z-loss / "
        "with a second label per row weighted by the device tensor mix_w");
  m.def("mix_draw", &mix_draw, py::arg("rng"), py::arg("stream"), py::arg("H"), py::arg("W"), py::arg("mixup_alpha"),
        py::arg("cutmix_alpha"), py::arg("prob") = 1.0, py::arg("switch_prob") = 0.5, py::arg("count") = 1,
        "mixup / cutmix decisions [count, 8] from the device rng state (not advanced)");
  m.def("mix_pack", &mix_pack, py::arg("x"), py::arg("params"), py::arg("layout"), py::arg("cpad") = 8, py::arg("out") = py::none(),
        "NCHW fp32 -> packed bf16 (0: s2d, 1: nhwc) of the batch mixed with its roll by the device row params");
  m.def("ce_grad_scale", &ce_grad_scale, py::arg("d"), py::arg("g"), py::arg("inv_n"), "d * g * inv_n (device scalars)");
  m.def("cross_entropy", &cross_entropy, py::arg("logits"), py::arg("labels"), py::arg("V"), py::arg("grad_scale"),
        py::arg("want_grad"), py::arg("grad_bf16"), py::arg("ignore_index") = -100, py::arg("inplace") = false);
  m.def("cast_bf16", &cast_bf16, py::arg("x"), py::arg("out") = py::none());
  m.def("cast_f32", &cast_f32);
  m.def("act", &act, py::arg("a"), py::arg("b") = py::none(), py::arg("op") = 0);
  m.def("dropout", &dropout);
  m.def("add", &add, py::arg("a"), py::arg("b"), py::arg("alpha") = 1.0);
  m.def("colsum", &colsum, py::arg("dy"), py::arg("db"), py::arg("accumulate") = false);
  m.def("nchw_to_s2d", &nchw_to_s2d, py::arg("x"));
  m.def("nchw_to_nhwc", &nchw_to_nhwc, py::arg("x"), py::arg("cpad") = 8);
  m.def("patchify", &patchify, py::arg("x"), py::arg("patch"),
        "fp32 NCHW -> bf16 [N, (H/p)(W/p), C p p] patch rows ordered (c, py, px)");
  m.def("embedding_fwd", &embedding_fwd, py::arg("idx"), py::arg("wte"), py::arg("wpe") = py::none(),
        py::arg("pos") = py::none());
  m.def("embedding_bwd", &embedding_bwd, py::arg("idx"), py::arg("dout"), py::arg("dwte"), py::arg("dwpe") = py::none(),
        py::arg("pos") = py::none());
  m.def("optim_step", &optim_step);
  m.def("optim_grad_norm", &optim_grad_norm, py::arg("desc"), py::arg("chunks"), py::arg("partials"), py::arg("out"),
        py::arg("max_norm"), py::arg("hp") = py::none(), py::arg("skip_nonfinite") = false);
  m.def("optim_grad_scale", &optim_grad_scale, py::arg("desc"), py::arg("chunks"), py::arg("out"));
  m.def("optim_clip_coef", &optim_clip_coef, py::arg("partials"), py::arg("nchunks"), py::arg("out"), py::arg("max_norm"),
        py::arg("hp"), py::arg("skip_nonfinite") = false);
  m.def("optim_lr_schedule", &optim_lr_schedule, py::arg("hp"), py::arg("sched"), py::arg("cur"));
  m.def("optim_sched_header", []() { return dpe_optim_sched_header(); });
  m.def("optim_trust_partials", &optim_trust_partials);
  m.def("optim_trust_ratio", &optim_trust_ratio);
  m.def("optim_trust_step", &optim_trust_step);
  m.def("optim_step_ema", &optim_step_ema);
  m.def("optim_trust_step_ema", &optim_trust_step_ema);
  m.def("optim_ema_decay", &optim_ema_decay, py::arg("hp"), py::arg("blk"), py::arg("cur"));
  m.def("optim_ema_swap", &optim_ema_swap, py::arg("desc"), py::arg("chunks"), py::arg("ema"));
  m.def("optim_chunk_size", []() { return dpe_optim_chunk_size(); });
  m.def("optim_desc_bytes", []() { return dpe_optim_desc_bytes(); });
  m.def("layernorm_bwd_residual", &layernorm_bwd_residual, py::arg("dy"), py::arg("x"), py::arg("w"), py::arg("mean"),
        py::arg("rstd"), py::arg("dw"), py::arg("db"), py::arg("res_in"), py::arg("defer") = false);
  m.def("layernorm_bwd_finalize_group", &layernorm_bwd_finalize_group, py::arg("parts"), py::arg("rows"), py::arg("dws"),
        py::arg("dbs"));
  m.def("layernorm_fwd", &layernorm_fwd, py::arg("x"), py::arg("w"), py::arg("b") = py::none(), py::arg("eps") = 1e-5);
  m.def("layernorm_bwd", &layernorm_bwd, py::arg("dy"), py::arg("x"), py::arg("w"), py::arg("mean"), py::arg("rstd"),
        py::arg("dw"), py::arg("db") = py::none(), py::arg("dx_out") = py::none());
  m.def("cu_hog", [](int64_t nblocks, int64_t threads, int64_t lds_bytes, double us, int64_t vgprs,
                     const c10::optional<Tensor>& stop, bool sleepy, int64_t mode) {
          static Tensor sink = at::empty({1024}, at::TensorOptions().dtype(at::kFloat).device(at::kCUDA));
          static Tensor buf;
          const int md = mode >= 0 ? (int)mode : (sleepy ? 1 : 0);
          if (md == 2 && (!buf.defined() || buf.numel() < dpe_cu_hog_buf_floats((int)nblocks)))
            buf = at::zeros({dpe_cu_hog_buf_floats((int)nblocks)}, at::TensorOptions().dtype(at::kFloat).device(at::kCUDA));
          const unsigned* sp = nullptr;
          if (has(stop)) {
            TORCH_CHECK(stop->is_cuda() && stop->scalar_type() == at::kInt && stop->numel() >= 1, "cu_hog: stop is an int32 GPU tensor");
            sp = (const unsigned*)stop->data_ptr();
          }
          CHECK_RC(dpe_cu_hog((int)nblocks, (int)threads, (int)lds_bytes, us, (int)vgprs, sp, (float*)sink.data_ptr(),
                              md, md == 2 ? (float*)buf.data_ptr() : nullptr, cur_stream()),
                   "cu_hog");
        }, py::arg("nblocks"), py::arg("threads") = 256, py::arg("lds_bytes") = 0, py::arg("us") = 1000.0,
        py::arg("vgprs") = 8, py::arg("stop") = py::none(), py::arg("sleepy") = false, py::arg("mode") = -1,
        "occupancy probe: nblocks workgroups holding a CU slot (threads, LDS, ~vgprs per lane) until stop[0] != 0 or `us` "
        "microseconds pass (current stream); mode 0 VALU-bound, 1 idle (= sleepy), 2 RCCL-like reduce-copy streaming");
  m.def("hog_stop", [](Tensor& stop, int64_t v) {
          TORCH_CHECK(stop.is_cuda() && stop.scalar_type() == at::kInt, "hog_stop: int32 GPU tensor");
          CHECK_RC(dpe_hog_stop((unsigned*)stop.data_ptr(), (unsigned)v, cur_stream()), "hog_stop");
        }, py::arg("stop"), py::arg("value") = 1, "set a cu_hog stop flag, ordered on the current stream");
  m.def("attn_fwd", &attn_fwd, py::arg("qkv"), py::arg("H"), py::arg("scale"), py::arg("causal") = true,
        py::arg("out") = py::none(), py::arg("lse") = py::none(), py::arg("doc_start") = py::none(),
        py::arg("doc_end") = py::none(), py::arg("dropout_p") = 0.0, py::arg("rng") = py::none(), py::arg("stream") = 0,
        py::arg("seq_len") = 0);
  m.def("attn_bwd", &attn_bwd, py::arg("qkv"), py::arg("out"), py::arg("dout"), py::arg("lse"), py::arg("H"),
        py::arg("scale"), py::arg("causal") = true, py::arg("dqkv") = py::none(), py::arg("doc_start") = py::none(),
        py::arg("doc_end") = py::none(), py::arg("dropout_p") = 0.0, py::arg("rng") = py::none(), py::arg("stream") = 0,
        py::arg("seq_len") = 0);
  m.def("dropout_add", &dropout_add, py::arg("res"), py::arg("y"), py::arg("p"), py::arg("rng"), py::arg("stream") = 0,
        py::arg("out") = py::none(), "fp32 res + dropout(y) (y bf16 or fp32); mask from the device rng state int64[2] (seed, offset) and the stream");
  m.def("dropout_cast", &dropout_cast, py::arg("g"), py::arg("p"), py::arg("rng"), py::arg("stream") = 0,
        py::arg("out") = py::none(),
        "bf16 dropout(g) of an fp32 g with dropout_add's mask (its backward)");
  m.def("set_attn_staged", [](bool on) { return dpe_set_attn_staged(on ? 1 : 0) != 0; }, py::arg("on"),
        "attention on the register-staged kernels instead of the LDS-DMA ones (test switch; default off); returns the "
        "previous setting");
  m.def("set_gemm_backend", [](int64_t mode) {
          TORCH_CHECK(mode == 1, "only the native MFMA GEMM backend exists (mode 1); the vendor-library arm was removed");
        }, "kept for API compatibility: 1 = native kernels (the only backend)");
}

}  // namespace dpe_ops
