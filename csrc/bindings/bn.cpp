// pybind11 bindings of BatchNorm, its Gram-algebra form (with the 1x1 convs that apply it on load or in their
// epilogue) and the pooling / stem-backward ops fused with it.  Checks and stream discipline as conv.cpp.
#include <algorithm>
#include <vector>

#include "../kernels/pwconv.h"
#include "gemm_plan.h"
#include "ops_common.h"

namespace dpe_ops {
namespace {

// --------------------------------------------------------------- BatchNorm
int64_t rows_of(const Tensor& x) { return x.numel() / x.size(-1); }

// returns (y, coef[4][C]); stats: optional precomputed [2][C] column sums (from conv epilogue)
std::vector<Tensor> bn_fwd_train(const Tensor& x, const c10::optional<Tensor>& gamma, const c10::optional<Tensor>& beta,
                                 const c10::optional<Tensor>& rmean, const c10::optional<Tensor>& rvar, double momentum,
                                 double eps, bool relu, const c10::optional<Tensor>& residual,
                                 const c10::optional<Tensor>& stats) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_CONTIG(x);
  const int64_t C = x.size(-1), M = rows_of(x);
  TORCH_CHECK(C % 8 == 0 && C <= 2048, "bn: C must be a multiple of 8 and <= 2048");
  auto fo = x.options().dtype(at::kFloat);
  Tensor coef = at::empty({4, C}, fo);
  hipStream_t st = cur_stream();
  if (has(stats)) {
    TORCH_CHECK(stats->dim() == 3 && stats->size(0) == 2 && stats->size(1) == C, "stats must be [2][C][nb] partials");
    CHECK_RC(dpe_bn_finalize(fp(*stats), (int)stats->size(2), (int)C, M, fpo(gamma), fpo(beta), fpom(rmean), fpom(rvar),
                             (float)momentum, (float)eps, fp(coef), st), "bn_finalize");
  } else {
    const int nb = dpe_bn_stats_nblocks(M, (int)C);
    Tensor part = at::empty({nb, 2, C}, fo);
    CHECK_RC(dpe_bn_stats(bp(x), M, (int)C, nb, fp(part), st), "bn_stats");
    CHECK_RC(dpe_bn_finalize(fp(part), nb, (int)C, M, fpo(gamma), fpo(beta), fpom(rmean), fpom(rvar), (float)momentum,
                             (float)eps, fp(coef), st), "bn_finalize");
  }
  Tensor y = at::empty_like(x);
  const uint16_t* res = nullptr;
  if (has(residual)) { CHECK_BF16((*residual)); CHECK_CONTIG((*residual)); res = bp(*residual); }
  CHECK_RC(dpe_bn_apply(bp(x), res, bpm(y), M, (int)C, fp(coef), relu ? 1 : 0, st), "bn_apply");
  return {y, coef};
}

Tensor bn_fwd_eval(const Tensor& x, const c10::optional<Tensor>& gamma, const c10::optional<Tensor>& beta,
                   const Tensor& rmean, const Tensor& rvar, double eps, bool relu, const c10::optional<Tensor>& residual) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_CONTIG(x);
  const int64_t C = x.size(-1), M = rows_of(x);
  Tensor coef = at::empty({4, C}, x.options().dtype(at::kFloat));
  hipStream_t st = cur_stream();
  CHECK_RC(dpe_bn_eval_coeff((int)C, fpo(gamma), fpo(beta), fp(rmean), fp(rvar), (float)eps, fp(coef), st), "bn_eval");
  Tensor y = at::empty_like(x);
  const uint16_t* res = nullptr;
  if (has(residual)) res = bp(*residual);
  CHECK_RC(dpe_bn_apply(bp(x), res, bpm(y), M, (int)C, fp(coef), relu ? 1 : 0, st), "bn_apply");
  return y;
}

// returns (dx, dz or empty); dgamma/dbeta accumulated (+=) if given
std::vector<Tensor> bn_bwd(const Tensor& dy, const c10::optional<Tensor>& y, const Tensor& x,
                           const c10::optional<Tensor>& gamma, const Tensor& coef, const c10::optional<Tensor>& dgamma,
                           const c10::optional<Tensor>& dbeta, bool want_dz, const c10::optional<Tensor>& y_bits) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_CONTIG(dy); CHECK_CONTIG(x);
  const int64_t C = x.size(-1), M = rows_of(x);
  const uint16_t* yp = has(y) ? bp(*y) : nullptr;
  const uint8_t* yb = nullptr;
  if (has(y_bits)) {
    // ReLU mask as bn_apply's bits (1/16 of y's bytes): y itself is not read
    CHECK_CONTIG((*y_bits));
    TORCH_CHECK(y_bits->scalar_type() == at::kByte && y_bits->numel() * 8 == x.numel() && C % 8 == 0,
                "bn_bwd: y_bits must be uint8 mask bits [.., C/8] of x's shape");
    yb = (const uint8_t*)y_bits->data_ptr();
    yp = nullptr;
  }
  hipStream_t st = cur_stream();
  auto fo = x.options().dtype(at::kFloat);
  const int nb = dpe_bn_bwd_nblocks(M, (int)C);
  Tensor part = at::empty({nb, 2, C}, fo);
  CHECK_RC(dpe_bn_bwd_reduce(bp(dy), yp, yb, bp(x), fp(coef), M, (int)C, nb, fp(part), st), "bn_bwd_reduce");
  Tensor bcoef = at::empty({3, C}, fo);
  CHECK_RC(dpe_bn_bwd_finalize(fp(part), nb, (int)C, M, fpo(gamma), fp(coef), fpom(dgamma), fpom(dbeta), fp(bcoef), st),
           "bn_bwd_finalize");
  Tensor dx = at::empty_like(x);
  Tensor dz;
  if (want_dz) dz = at::empty_like(x);
  CHECK_RC(dpe_bn_bwd_apply(bp(dy), yp, yb, bp(x), fp(bcoef), bpm(dx), want_dz ? bpm(dz) : nullptr, M, (int)C, nullptr, st),
           "bn_bwd_apply");
  return {dx, dz};
}

// ------------------------------------------------------------ BN3 by Gram algebra (bngram.hip)
// G = a'^T a' [C][C] and s = [colsum(a'), mu] [2][C] of a' = a2 - mu, a2 = relu(x * coef[0] + coef[1]) (coef: the
// BN's [4][C]) or x, centred on the pilot shift mu (bngram.hip relu_gauss_mean) of the BN coefficients
// shift_coef (default: coef; neither: mu = 0).
// stride2: x is an [N, H, W, C] image (even H, W) and the pass runs over its stride-2 subsample x[:, ::2, ::2, :],
// the input pixels of a stride-2 1x1 conv, by row addressing (no copy).
std::vector<Tensor> bn_gram(const Tensor& x, const c10::optional<Tensor>& coef, const c10::optional<Tensor>& shift_coef,
                            bool stride2) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_CONTIG(x);
  TORCH_CHECK(!stride2 || (x.dim() == 4 && x.size(1) % 2 == 0 && x.size(2) % 2 == 0), "bn_gram: stride2 needs [N, H, W, C], even H, W");
  const int64_t C = x.size(-1), M = x.numel() / C / (stride2 ? 4 : 1);
  TORCH_CHECK(C == 64 || C == 128 || C == 256, "bn_gram: C must be 64, 128 or 256");
  if (has(coef)) {
    CHECK_F32((*coef)); CHECK_CONTIG((*coef));
    TORCH_CHECK(coef->numel() >= 2 * C, "bn_gram: coef must be the BN's [4][C] coefficients");
  }
  const float* scoef = fpo(coef);
  if (scoef) TORCH_CHECK(coef->numel() == 4 * C, "bn_gram: the shift needs coef's full [4][C] (scale, shift, mean, invstd)");
  if (has(shift_coef)) {
    CHECK_F32((*shift_coef)); CHECK_CONTIG((*shift_coef));
    TORCH_CHECK(shift_coef->numel() == 4 * C, "bn_gram: shift_coef must be the BN's [4][C] coefficients");
    scoef = fp(*shift_coef);
  }
  auto fo = x.options().dtype(at::kFloat);
  Tensor ws = at::empty({dpe_gram_ws_floats(M, (int)C)}, fo);
  Tensor G = at::empty({C, C}, fo), sv = at::empty({2, C}, fo);
  CHECK_RC(dpe_gram(bp(x), fpo(coef), scoef, M, (int)C, fp(ws), fp(G), fp(sv), cur_stream(), stride2 ? (int)x.size(1) : 0,
                    stride2 ? (int)x.size(2) : 0), "bn_gram");
  return {G, sv};
}

// BN coefficients [4][Cout] of h = a2 W^T (never computed) from G, s: mean = w.s / M, E[h^2] = w^T G w / M;
// running stats updated as bn_coef.  Also returns u = W G [Cout][Cin] (fp32) for the backward.
std::vector<Tensor> bn_gram_coef(const Tensor& G, const Tensor& sv, const Tensor& w, int64_t M,
                                 const c10::optional<Tensor>& gamma, const c10::optional<Tensor>& beta,
                                 const c10::optional<Tensor>& rmean, const c10::optional<Tensor>& rvar, double momentum,
                                 double eps) {
  CHECK_GPU(G); CHECK_F32(G); CHECK_F32(sv); CHECK_BF16(w); CHECK_CONTIG(w); CHECK_CONTIG(G);
  const int64_t Cin = G.size(0), Cout = w.size(0);
  TORCH_CHECK(w.numel() == Cout * Cin && sv.numel() == 2 * Cin, "bn_gram_coef: shapes (s is bn_gram's [2][C])");
  CHECK_CONTIG(sv);
  Tensor coef = at::empty({4, Cout}, G.options()), u = at::empty({Cout, Cin}, G.options());
  CHECK_RC(dpe_gram_coef(fp(G), fp(sv), bp(w), (int)Cin, (int)Cout, M, fpo(gamma), fpo(beta), fpom(rmean), fpom(rvar),
                         (float)momentum, (float)eps, fp(coef), fp(u), cur_stream()), "bn_gram_coef");
  return {coef, u};
}

// y = relu(BN(x' W^T) + residual) of a 1x1 conv (x' = relu(x * in_coef) or x), with the BN's coefficients known
// in advance (bn_gram_coef): streaming pointwise kernel, PW_APPLY.  res_coef: the residual is the pre-BN
// output of a downsample conv, BN'd (and rounded) on the fly.  Returns (y, ReLU bits of y).
std::vector<Tensor> conv1x1_apply(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& in_coef,
                                  const Tensor& out_coef, const Tensor& residual, const c10::optional<Tensor>& res_coef) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_CONTIG(x); CHECK_BF16(w); CHECK_CONTIG(w); CHECK_F32(out_coef);
  CHECK_BF16(residual); CHECK_CONTIG(residual);
  const int64_t K = x.size(-1), M = x.numel() / K, N = w.size(0);
  TORCH_CHECK(w.numel() == N * K && out_coef.numel() == 4 * N, "conv1x1_apply: shapes");
  auto ysz = x.sizes().vec();
  ysz.back() = N;
  TORCH_CHECK(residual.sizes().vec() == ysz, "conv1x1_apply: residual must have the output's shape");
  const int rg = pw_stream_on() ? dpe_pw_rowgroups(M, N, K, dpe::PW_APPLY) : 0;
  TORCH_CHECK(rg > 0, "conv1x1_apply: outside the streaming pointwise kernel's envelope");
  Tensor y = at::empty(ysz, x.options());
  auto bsz = ysz;
  bsz.back() = N / 8;
  Tensor bits = at::empty(bsz, x.options().dtype(at::kByte));
  dpe::PwArgs pa{};
  pa.x = bp(x); pa.w = bp(w); pa.y = bpm(y);
  pa.in_coef = fpo(in_coef);
  pa.out_coef = fp(out_coef);
  pa.residual = bp(residual);
  pa.res_coef = fpo(res_coef);
  pa.out_bits = (uint8_t*)bits.data_ptr();
  pa.M = M; pa.N = N; pa.K = K; pa.rg = rg; pa.sched = dpe_gemm::sched_buffer(cur_stream());
  CHECK_RC(dpe_pw_launch(&pa, dpe::PW_APPLY, cur_stream()), "pw_stream apply");
  return {y, bits};
}

// The envelope of conv1x1_apply_next: a conv3 over h2shape [N, H, W, 64] -> cout3 == 256 on the streaming kernel whose
// pass also forms the next block's 1x1 stride-1 conv1 (256 -> c1_next in {64, 128}).  False while a CU budget is in
// force with the dynamic schedule on (no dynamic variant is built): the caller then makes the two separate calls.
bool c1_fuse_ok(const std::vector<int64_t>& h2shape, int64_t cout3, int64_t c1_next) {
  if (h2shape.size() != 4 || !pw_stream_on()) return false;
  const int64_t M = h2shape[0] * h2shape[1] * h2shape[2];
  return cout3 == 256 && h2shape[3] == 64 && (c1_next == 64 || c1_next == 128) &&
         dpe_pw_next_rowgroups(M, cout3, h2shape[3], c1_next) > 0;
}

// conv1x1_apply with the next block's conv1 in the same streaming pass: (y, bits) exactly as conv1x1_apply(x, w,
// in_coef, out_coef, residual, None) and h1 = y W_next^T [.., c1_next] (from the stored bf16 y, fp32 sums, rounded
// once) with the BatchNorm-forward partials st [2][c1_next][row groups] of the stored h1 (bn_coef's input, as
// conv_fwd's).  A BN'd residual (res_coef) is outside the envelope.  Returns (y, bits, h1, st); ``outs``: these four
// given by the caller (exact shapes and types, contiguous; row groups from a first call) instead of allocated here.
std::vector<Tensor> conv1x1_apply_next(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& in_coef,
                                       const Tensor& out_coef, const Tensor& residual, const c10::optional<Tensor>& res_coef,
                                       const Tensor& w_next, const c10::optional<std::vector<Tensor>>& outs) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_CONTIG(x); CHECK_BF16(w); CHECK_CONTIG(w); CHECK_F32(out_coef); CHECK_CONTIG(out_coef);
  CHECK_GPU(residual); CHECK_BF16(residual); CHECK_CONTIG(residual); CHECK_GPU(w_next); CHECK_BF16(w_next); CHECK_CONTIG(w_next);
  TORCH_CHECK(!has(res_coef), "conv1x1_apply_next: a BN'd residual is outside the envelope");
  TORCH_CHECK(x.dim() == 4, "conv1x1_apply_next: x must be [N, H, W, K]");
  const int64_t K = x.size(-1), M = x.numel() / K, N = w.size(0), C1 = w_next.size(0);
  TORCH_CHECK(w.numel() == N * K && out_coef.numel() == 4 * N && w_next.numel() == C1 * N, "conv1x1_apply_next: shapes");
  if (has(in_coef)) {
    CHECK_F32((*in_coef)); CHECK_CONTIG((*in_coef));
    TORCH_CHECK(in_coef->numel() >= 2 * K, "conv1x1_apply_next: in_coef must be the BN's [4][K] coefficients");
  }
  auto ysz = x.sizes().vec();
  ysz.back() = N;
  TORCH_CHECK(residual.sizes().vec() == ysz, "conv1x1_apply_next: residual must have the output's shape");
  TORCH_CHECK(c1_fuse_ok(x.sizes().vec(), N, C1), "conv1x1_apply_next: outside the envelope (c1_fuse_ok)");
  const int rg = dpe_pw_next_rowgroups(M, N, K, C1);
  Tensor y = at::empty(ysz, x.options());
  auto bsz = ysz;
  bsz.back() = N / 8;
  Tensor bits = at::empty(bsz, x.options().dtype(at::kByte));
  auto hsz = ysz;
  hsz.back() = C1;
  Tensor h1 = at::empty(hsz, x.options());
  Tensor st = at::empty({2, C1, rg}, x.options().dtype(at::kFloat));
  if (outs.has_value()) {
    TORCH_CHECK(outs->size() == 4, "conv1x1_apply_next: outs must be (y, bits, h1, st)");
    const Tensor* mine[4] = {&y, &bits, &h1, &st};
    for (int i = 0; i < 4; ++i) {
      const Tensor& o = (*outs)[i];
      TORCH_CHECK(o.is_cuda() && o.is_contiguous() && o.sizes() == mine[i]->sizes() && o.scalar_type() == mine[i]->scalar_type(),
                  "conv1x1_apply_next: outs[", i, "] has the wrong shape, type or layout");
    }
    y = (*outs)[0]; bits = (*outs)[1]; h1 = (*outs)[2]; st = (*outs)[3];
  }
  dpe::PwArgs pa{};
  pa.x = bp(x); pa.w = bp(w); pa.y = bpm(y);
  pa.in_coef = fpo(in_coef);
  pa.out_coef = fp(out_coef);
  pa.residual = bp(residual);
  pa.out_bits = (uint8_t*)bits.data_ptr();
  pa.w_next = bp(w_next); pa.y_next = bpm(h1); pa.stats_next = fp(st); pa.c1_next = (int)C1;
  pa.M = M; pa.N = N; pa.K = K; pa.rg = rg;
  CHECK_RC(dpe_pw_launch(&pa, dpe::PW_APPLY, cur_stream()), "pw_stream apply + next conv1");
  return {y, bits, h1, st};
}

// The envelope of conv1x1_apply_cat: a 1x1 stride-1 downsample conv over xshape [N, H, W, Cin] (Cin in {64, 128})
// beside a conv3 whose operand has cmid == Cin channels, both -> cout = 4 Cin.
bool down_cat_ok(const std::vector<int64_t>& xshape, int64_t cmid, int64_t cout, int64_t stride) {
  if (xshape.size() != 4 || stride != 1 || !pw_stream_on()) return false;
  const int64_t M = xshape[0] * xshape[1] * xshape[2], C = xshape[3];
  return (C == 64 || C == 128) && cmid == C && dpe_pw_cat_fwd_rowgroups(M, cout, C) > 0;
}

// y = relu(BN3(x' W^T) + BN_d(x2 W2^T)) of a downsample bottleneck's conv3 (x' = relu(x * in_coef) or x) and its
// 1x1 stride-1 downsample conv over the block input x2, as ONE streaming pass over the concatenated K = [x' | x2]
// (pwconv.hip PW_CAT): both BNs' coefficients are known in advance (bn_gram_coef), the two fp32 sums are scaled
// per output channel and rounded once; neither pre-BN tensor exists.  Returns (y, ReLU bits of y).  The dynamic
// schedule under a CU budget is built for both shapes, so the op has no fall-back of its own.
std::vector<Tensor> conv1x1_apply_cat(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& in_coef,
                                      const Tensor& out_coef, const Tensor& x2, const Tensor& w2, const Tensor& coef2) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_CONTIG(x); CHECK_BF16(w); CHECK_CONTIG(w); CHECK_F32(out_coef); CHECK_CONTIG(out_coef);
  CHECK_GPU(x2); CHECK_BF16(x2); CHECK_CONTIG(x2); CHECK_BF16(w2); CHECK_CONTIG(w2); CHECK_F32(coef2); CHECK_CONTIG(coef2);
  const int64_t K1 = x.size(-1), M = x.numel() / K1, N = w.size(0), K2 = x2.size(-1);
  TORCH_CHECK(x.dim() == 4 && K1 == K2 && x2.numel() == M * K2 && w.numel() == N * K1 && w2.numel() == N * K2 &&
                  out_coef.numel() == 4 * N && coef2.numel() == 4 * N, "conv1x1_apply_cat: shapes");
  if (has(in_coef)) {
    CHECK_F32((*in_coef)); CHECK_CONTIG((*in_coef));
    TORCH_CHECK(in_coef->numel() == 4 * K1, "conv1x1_apply_cat: in_coef must be the BN's [4][K] coefficients");
  }
  TORCH_CHECK(down_cat_ok(x2.sizes().vec(), K1, N, 1), "conv1x1_apply_cat: outside the envelope (down_cat_ok)");
  const int rg = dpe_pw_cat_fwd_rowgroups(M, N, K2);
  auto ysz = x.sizes().vec();
  ysz.back() = N;
  Tensor y = at::empty(ysz, x.options());
  auto bsz = ysz;
  bsz.back() = N / 8;
  Tensor bits = at::empty(bsz, x.options().dtype(at::kByte));
  dpe::PwArgs pa{};
  pa.x = bp(x); pa.w = bp(w); pa.y = bpm(y);
  pa.x2 = bp(x2); pa.w2 = bp(w2); pa.cat_k2 = (int)K2;
  pa.in_coef = fpo(in_coef);
  pa.out_coef = fp(out_coef);
  pa.res_coef = fp(coef2);
  pa.out_bits = (uint8_t*)bits.data_ptr();
  pa.M = M; pa.N = N; pa.K = K1 + K2; pa.rg = rg; pa.sched = dpe_gemm::sched_buffer(cur_stream());
  CHECK_RC(dpe_pw_launch(&pa, dpe::PW_CAT, cur_stream()), "pw_stream concatenated-K apply");
  return {y, bits};
}

// BN3 backward by Gram algebra: from part (row 0: sum dz partials, [2][Cout][rg]), P = dz^T a2 [Cout][Cin], W,
// u = W G, s, the forward coef: dgamma / dbeta / dw accumulate; returns the data grad's B operand
// [Cout + Cin][Cin] bf16 (= [diag(a) W ; W^T diag(b) W]) and its bias c^T W [Cin].
std::vector<Tensor> bn_gram_bwd(const Tensor& part, const Tensor& P, const Tensor& w, const Tensor& u, const Tensor& sv,
                                const Tensor& coef, const c10::optional<Tensor>& gamma, int64_t M,
                                const c10::optional<Tensor>& dgamma, const c10::optional<Tensor>& dbeta, Tensor& dw) {
  CHECK_GPU(part); CHECK_F32(part); CHECK_F32(P); CHECK_F32(u); CHECK_F32(sv); CHECK_F32(coef); CHECK_F32(dw);
  CHECK_BF16(w); CHECK_CONTIG(w); CHECK_CONTIG(P); CHECK_CONTIG(dw); CHECK_CONTIG(part);
  const int64_t Cout = w.size(0), Cin = w.numel() / Cout;
  TORCH_CHECK(part.dim() == 3 && part.size(1) == Cout && P.numel() == Cout * Cin && u.numel() == Cout * Cin &&
                  dw.numel() == Cout * Cin && sv.numel() == 2 * Cin && coef.numel() == 4 * Cout && sv.is_contiguous(),
              "bn_gram_bwd: shapes");
  auto fo = P.options();
  Tensor bcat = at::empty({Cout + Cin, Cin}, w.options()), abc = at::empty({3, Cout}, fo), e = at::empty({Cin}, fo);
  Tensor qws = at::empty({dpe_gram_bwd_ws_floats((int)Cin, (int)Cout)}, fo);
  CHECK_RC(dpe_gram_bwd(fp(part), (int)part.size(2), fp(P), bp(w), fp(u), fp(sv), fp(coef), fpo(gamma), (int)Cin,
                        (int)Cout, M, fpom(dgamma), fpom(dbeta), fp(dw), bpm(bcat), fp(abc), fp(e), fp(qws), cur_stream()),
           "bn_gram_bwd");
  return {bcat, e};
}

// da2 = [dz | a2] x bcat + e with the BN-backward partials of the BN + ReLU that produced a2 (bn_x, bn_coef):
// the concatenated-K data grad of the Gram-algebra BN3 backward (igemm AX_CAT).  a2 = relu(a2src * a2_coef)
// when a2_coef is given (a2 never materialised), else a2src itself.  Returns (da2, partials).
std::vector<Tensor> conv1x1_dgrad_cat(const Tensor& dz, const Tensor& a2src, const c10::optional<Tensor>& a2_coef,
                                      const Tensor& bcat, const Tensor& e, const Tensor& bn_x, const Tensor& bn_coef) {
  CHECK_GPU(dz); CHECK_BF16(dz); CHECK_CONTIG(dz); CHECK_BF16(a2src); CHECK_CONTIG(a2src); CHECK_BF16(bcat);
  CHECK_CONTIG(bcat); CHECK_F32(e); CHECK_BF16(bn_x); CHECK_CONTIG(bn_x); CHECK_F32(bn_coef);
  const int64_t K1 = dz.size(-1), M = dz.numel() / K1, C = a2src.size(-1);
  TORCH_CHECK(a2src.numel() == M * C && bcat.size(0) == K1 + C && bcat.size(1) == C && e.numel() == C &&
                  bn_x.sizes() == a2src.sizes() && bn_coef.numel() == 4 * C && K1 % 32 == 0 && C % 32 == 0,
              "conv1x1_dgrad_cat: shapes");
  Tensor dx = at::empty_like(bn_x);
  // a2 materialised and >= 256 channels (layer 3): the persistent GEMM's NN layout with the two A segments
  // (hgemm.hip CV = 3) and its BN-backward-partials epilogue; 156-167 us per call on the LDS-DMA kernel
  // here (416 TF, profiles/resnet50_bs512_sequence_r4.txt in git history)
  if (hgemm_conv_on() && !has(a2_coef) && C >= 256 && C % 64 == 0 && K1 % 64 == 0) {
    int pcols = 0;
    const auto pl = dpe_gemm::plan_bnb(M, C, K1 + C, 1, 0, &pcols);
    if (pl.cfg >= 0 && pl.splits == 1 && pcols > 0) {
      Tensor part = at::empty({2, C, pcols}, dz.options().dtype(at::kFloat));
      auto h = hargs();
      h.A = bp(dz); h.B = bp(bcat); h.C = dx.data_ptr();
      h.M = (int)M; h.N = (int)C; h.K = (int)(K1 + C);
      h.lda = K1; h.ldb = C; h.ldc = C;
      h.bias = fp(e);
      h.conv = 3; h.A2 = bp(a2src); h.lda2 = C; h.k1 = (int)K1;
      h.col_stats = fp(part); h.stats_ld = pcols; h.st_x = bp(bn_x); h.st_coef = fp(bn_coef);
      dpe_gemm::run_bnb(h, pl, 1, 0);
      return {dx, part};
    }
  }
  // a2 = relu(BN2(h2)) on load with h2 also the BN-backward input (layers 1-2): the streaming kernel
  // (pwconv.hip pw_cat_kernel) -- mask and h2 - mean from the h2 tile it holds, no second read of h2
  if (has(a2_coef) && a2src.data_ptr() == bn_x.data_ptr() && a2_coef->numel() == 4 * C &&
      bn_coef.data_ptr() == a2_coef->data_ptr()) {
    const int rg = dpe_pw_cat_blocks(M, K1, C);
    if (rg > 0) {
      Tensor part = at::empty({2, C, rg}, dz.options().dtype(at::kFloat));
      dpe::PwCatArgs pa{};
      pa.dz = bp(dz); pa.h2 = bp(a2src); pa.coef = fp(bn_coef); pa.bcat = bp(bcat); pa.ebias = fp(e);
      pa.y = bpm(dx); pa.stats = fp(part); pa.M = M; pa.rg = rg;
      CHECK_RC(dpe_pw_cat_launch(&pa, K1, C, cur_stream()), "pw_cat data grad");
      return {dx, part};
    }
  }
  auto a = base_args();
  a.A = bp(dz); a.B = bp(bcat); a.C = dx.data_ptr();
  a.M = (int)M; a.N = (int)C; a.K = (int)(K1 + C);
  a.lda = K1; a.ldb = C; a.ldc = C;
  a.k_split = a.K;
  a.bias = fp(e);
  a.a_mode = dpe::AX_CAT;
  a.a2 = bp(a2src); a.lda2 = C; a.k1 = (int)K1;
  a.a_coef = fpo(a2_coef);
  a.st_x = bp(bn_x); a.st_coef = fp(bn_coef);
  const int bm = 128, bn = C <= 64 ? 64 : 128;
  const int64_t tilesM = (M + bm - 1) / bm;
  Tensor part = at::empty({2, C, tilesM}, dz.options().dtype(at::kFloat));
  a.col_stats = fp(part);
  a.stats_ld = (int)tilesM;
  const int rc = dpe_igemm_dma_launch(&a, bm, bn, dpe::A_DENSE_K, dpe::B_DENSE_N, dpe::EPI_BF16_BNB, cur_stream());
  CHECK_RC(rc, "igemm_dma AX_CAT data grad");
  return {dx, part};
}

// Pilot shift for bn_gram's shift_coef when x has no producing BN (a downsample conv's block input): [4][C] =
// (1, 0, mean of a fixed sample of x's rows, 0), the degenerate BN description bngram.hip's relu_gauss_mean
// turns into the (5-bit) mean itself.
Tensor bn_gram_pilot(const Tensor& x, bool stride2) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_CONTIG(x);
  TORCH_CHECK(!stride2 || (x.dim() == 4 && x.size(1) % 2 == 0 && x.size(2) % 2 == 0), "bn_gram_pilot: stride2 needs [N, H, W, C], even H, W");
  const int64_t C = x.size(-1), M = x.numel() / C / (stride2 ? 4 : 1);
  TORCH_CHECK(C == 64 || C == 128 || C == 256, "bn_gram_pilot: C must be 64, 128 or 256");
  Tensor coef = at::empty({4, C}, x.options().dtype(at::kFloat));
  CHECK_RC(dpe_gram_pilot(bp(x), M, (int)C, fp(coef), cur_stream(), stride2 ? (int)x.size(1) : 0,
                          stride2 ? (int)x.size(2) : 0), "bn_gram_pilot");
  return coef;
}

// u = W G [Cout][Cin] (fp32) alone: bn_gram_coef's by-product without its BN coefficients / running-statistics
// update (the downsample BN's were produced by bn_coef in the forward).
Tensor bn_gram_u(const Tensor& G, const Tensor& w) {
  CHECK_GPU(G); CHECK_F32(G); CHECK_CONTIG(G); CHECK_BF16(w); CHECK_CONTIG(w);
  const int64_t Cin = G.size(0), Cout = w.size(0);
  TORCH_CHECK(G.dim() == 2 && G.size(1) == Cin && w.numel() == Cout * Cin, "bn_gram_u: shapes");
  Tensor u = at::empty({Cout, Cin}, G.options());
  CHECK_RC(dpe_gram_u(fp(G), bp(w), (int)Cin, (int)Cout, fp(u), cur_stream()), "bn_gram_u");
  return u;
}

// dx = [dz | x] x bcat + e: the concatenated-K data grad of a downsample branch whose BN runs by Gram algebra
// (x the block input, plain; no BN-backward partials).  Stride 1: streaming kernel (pwconv.hip pw_cat_kernel,
// BN = false), (K1, C) in {(256, 64), (512, 128)}.  stride2: dz is [N, H/2, W/2, K1], the second segment is the
// stride-2 subsample of x [N, H, W, C] by row addressing and the result is the compact [N, H/2, W/2, C] grid (the
// streaming conv1 data grad adds it at the even pixels): the LDS-DMA implicit GEMM's AX_CAT.  bnd_gram_ok below.
Tensor conv1x1_dgrad_cat_plain(const Tensor& dz, const Tensor& x, const Tensor& bcat, const Tensor& e, bool stride2) {
  CHECK_GPU(dz); CHECK_BF16(dz); CHECK_CONTIG(dz); CHECK_BF16(x); CHECK_CONTIG(x); CHECK_BF16(bcat); CHECK_CONTIG(bcat);
  CHECK_F32(e);
  const int64_t K1 = dz.size(-1), M = dz.numel() / K1, C = x.size(-1);
  if (stride2) {
    TORCH_CHECK(x.dim() == 4 && dz.dim() == 4 && x.size(1) == 2 * dz.size(1) && x.size(2) == 2 * dz.size(2) &&
                    x.size(0) == dz.size(0) && bcat.dim() == 2 && bcat.size(0) == K1 + C && bcat.size(1) == C &&
                    e.numel() == C && K1 % 32 == 0 && C % 32 == 0,
                "conv1x1_dgrad_cat_plain: stride-2 shapes");
    Tensor dx = at::empty({dz.size(0), dz.size(1), dz.size(2), C}, x.options());
    auto a = base_args();
    a.A = bp(dz); a.B = bp(bcat); a.C = dx.data_ptr();
    a.M = (int)M; a.N = (int)C; a.K = (int)(K1 + C);
    a.lda = K1; a.ldb = C; a.ldc = C;
    a.k_split = a.K;
    a.bias = fp(e);
    a.a_mode = dpe::AX_CAT;
    a.a2 = bp(x); a.lda2 = C; a.k1 = (int)K1;
    a.a2_h = (int)x.size(1); a.a2_w = (int)x.size(2);
    CHECK_RC(dpe_igemm_dma_launch(&a, 128, C <= 64 ? 64 : 128, dpe::A_DENSE_K, dpe::B_DENSE_N, dpe::EPI_BF16, cur_stream()),
             "igemm_dma AX_CAT data grad (stride-2 second segment)");
    return dx;
  }
  TORCH_CHECK(x.numel() == M * C && bcat.dim() == 2 && bcat.size(0) == K1 + C && bcat.size(1) == C && e.numel() == C,
              "conv1x1_dgrad_cat_plain: shapes");
  const int rg = dpe_pw_cat_blocks(M, K1, C);
  TORCH_CHECK(rg > 0, "conv1x1_dgrad_cat_plain: outside the streaming concatenated-K kernel's envelope");
  Tensor dx = at::empty_like(x);
  dpe::PwCatArgs pa{};
  pa.dz = bp(dz); pa.h2 = bp(x); pa.bcat = bp(bcat); pa.ebias = fp(e);
  pa.y = bpm(dx); pa.M = M; pa.rg = rg;
  CHECK_RC(dpe_pw_cat_launch(&pa, K1, C, cur_stream()), "pw_cat data grad (plain)");
  return dx;
}

// BatchNorm coefficients [4][C] (scale, shift, mean, invstd) from conv-epilogue
// partials WITHOUT applying them: the consumer conv applies relu(x*scale+shift)
// in its load prologue.  Updates running stats like bn_fwd_train.
Tensor bn_coef(const Tensor& stats, int64_t M, const c10::optional<Tensor>& gamma, const c10::optional<Tensor>& beta,
               const c10::optional<Tensor>& rmean, const c10::optional<Tensor>& rvar, double momentum, double eps) {
  CHECK_GPU(stats); CHECK_F32(stats);
  TORCH_CHECK(stats.dim() == 3 && stats.size(0) == 2, "stats must be [2][C][nb] partials");
  const int64_t C = stats.size(1);
  Tensor coef = at::empty({4, C}, stats.options());
  CHECK_RC(dpe_bn_finalize(fp(stats), (int)stats.size(2), (int)C, M, fpo(gamma), fpo(beta), fpom(rmean), fpom(rvar),
                           (float)momentum, (float)eps, fp(coef), cur_stream()), "bn_finalize");
  return coef;
}

// Backward of y = relu(BN(x)) given the (sum dz, sum dz*(x-mean)) partials
// [2][C][nb] produced by the dgrad epilogue that computed dy; the ReLU mask is
// recomputed from x and the forward coefficients.  dgamma/dbeta accumulate.
// relu_mask=false: dy is already dz (masked by its producer, see conv_dgrad_bn's mask).
Tensor bn_bwd_partials(const Tensor& dy, const Tensor& x, const c10::optional<Tensor>& gamma, const Tensor& coef,
                       const Tensor& partials, const c10::optional<Tensor>& dgamma, const c10::optional<Tensor>& dbeta,
                       bool relu_mask) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_CONTIG(dy); CHECK_CONTIG(x); CHECK_BF16(x);
  TORCH_CHECK(dy.sizes() == x.sizes(), "bn_bwd_partials: dy/x shape mismatch");
  const int64_t C = x.size(-1), M = rows_of(x);
  TORCH_CHECK(partials.dim() == 3 && partials.size(0) == 2 && partials.size(1) == C, "partials must be [2][C][nb]");
  hipStream_t st = cur_stream();
  Tensor bcoef = at::empty({3, C}, x.options().dtype(at::kFloat));
  CHECK_RC(dpe_bn_bwd_finalize(fp(partials), (int)partials.size(2), (int)C, M, fpo(gamma), fp(coef), fpom(dgamma),
                               fpom(dbeta), fp(bcoef), st), "bn_bwd_finalize");
  Tensor dx = at::empty_like(x);
  CHECK_RC(dpe_bn_bwd_apply(bp(dy), nullptr, nullptr, bp(x), fp(bcoef), bpm(dx), nullptr, M, (int)C, relu_mask ? fp(coef) : nullptr, st),
           "bn_bwd_apply");
  return dx;
}

// BatchNorm-backward coefficients [3][C] (dx = a*dz + b*x + c) from the (sum dz, sum dz*(x-mean))
// partials, without the apply pass (its consumer applies it on load: conv1x1_bnin_dgrad).
// dgamma/dbeta accumulate.
Tensor bn_bwd_coef(const Tensor& partials, int64_t M, const c10::optional<Tensor>& gamma, const Tensor& coef,
                   const c10::optional<Tensor>& dgamma, const c10::optional<Tensor>& dbeta) {
  CHECK_GPU(partials); CHECK_F32(partials);
  TORCH_CHECK(partials.dim() == 3 && partials.size(0) == 2, "partials must be [2][C][nb]");
  const int64_t C = partials.size(1);
  Tensor bcoef = at::empty({3, C}, partials.options());
  CHECK_RC(dpe_bn_bwd_finalize(fp(partials), (int)partials.size(2), (int)C, M, fpo(gamma), fp(coef), fpom(dgamma),
                               fpom(dbeta), fp(bcoef), cur_stream()), "bn_bwd_finalize");
  return bcoef;
}

// 1x1 stride-1 convolutions over a BatchNorm output that is never written by a pass of its own
// (igemm.h AXform): the LDS-DMA kernel computes the operand from two tensors on its fragments and
// stores it once as a by-product (x_out [+ x_bits]), so the consumer's own read of it disappears.
//
// forward: y = x . W^T,  x = relu(h * scale + shift + res)           (res_coef absent)
//                         x = relu(h * scale + shift + bf16(res * scale_d + shift_d))   (downsample identity)
// with the BN-forward partials of y when want_stats.  tile_m: 128 or 256 (N = 64 only).
std::vector<Tensor> conv1x1_bnin_fwd(const Tensor& h, const Tensor& res, const Tensor& coef,
                                     const c10::optional<Tensor>& res_coef, const Tensor& w, Tensor& x_out,
                                     Tensor& x_bits, bool want_stats, int64_t tile_m) {
  CHECK_GPU(h); CHECK_BF16(h); CHECK_BF16(res); CHECK_BF16(w); CHECK_BF16(x_out);
  CHECK_CONTIG(h); CHECK_CONTIG(res); CHECK_CONTIG(w); CHECK_CONTIG(x_out); CHECK_CONTIG(x_bits);
  CHECK_F32(coef);
  TORCH_CHECK(h.dim() == 4 && w.dim() == 4 && w.size(1) == 1 && w.size(2) == 1 && w.size(3) == h.size(3),
              "conv1x1_bnin_fwd: NHWC h / [K,1,1,C] w shape mismatch");
  TORCH_CHECK(res.sizes() == h.sizes() && x_out.sizes() == h.sizes(), "conv1x1_bnin_fwd: res / x_out must have h's shape");
  TORCH_CHECK(x_bits.scalar_type() == at::kByte && x_bits.numel() * 8 == h.numel(), "conv1x1_bnin_fwd: x_bits [.., C/8] u8");
  const int64_t C = h.size(3), K = w.size(0);
  TORCH_CHECK(coef.numel() == 4 * C && (!res_coef.has_value() || res_coef->numel() == 4 * C), "coef must be [4][C]");
  TORCH_CHECK(C % 32 == 0 && C <= 2048 && K % 8 == 0, "conv1x1_bnin_fwd: C % 32 == 0, C <= 2048");
  Tensor y = at::empty({h.size(0), h.size(1), h.size(2), K}, h.options());
  auto a = base_args();
  a.g = geom(h, w, 1, 1, 0, 0, 1, 1, h.size(1), h.size(2));
  a.A = bp(h); a.B = bp(w); a.C = y.data_ptr();
  a.M = (int)(h.numel() / C); a.N = (int)K; a.K = (int)C;
  a.lda = C; a.ldb = C; a.ldc = K;
  a.k_split = a.K;
  a.a_mode = has(res_coef) ? dpe::AX_BN_RES2 : dpe::AX_BN_RES;
  a.a2 = bp(res); a.a_coef = fp(coef); a.a_coef2 = fpo(res_coef);
  a.a_out = bpm(x_out); a.a_bits = (uint8_t*)x_bits.data_ptr();
  Tensor stats;
  if (want_stats) {  // per-128-row partials: the layout every conv path produces (BN finalize is tile-agnostic)
    stats = at::empty({2, K, (a.M + 127) / 128}, h.options().dtype(at::kFloat));
    a.col_stats = fp(stats);
  }
  const int bm = (K == 64 && tile_m == 256) ? 256 : 128, bn = K <= 64 ? 64 : 128;
  CHECK_RC(dpe_igemm_dma_launch(&a, bm, bn, dpe::A_DENSE_K, dpe::B_DENSE_K, dpe::EPI_BF16, cur_stream()),
           "conv1x1_bnin_fwd");
  return {y, stats};
}

// data grad: dx = dh . W  with  dh = a * dz + b * h + c  (BN backward applied on load, dh stored as a
// by-product for the weight grad), plus the BN-backward partials of the BN + ReLU that produced this
// conv's input (bn_x, bn_coef: ReLU mask recomputed from bn_x), as conv_dgrad_bn.
std::vector<Tensor> conv1x1_bnin_dgrad(const Tensor& dz, const Tensor& h, const Tensor& bcoef, const Tensor& w,
                                       Tensor& dh_out, const Tensor& bn_x, const Tensor& bn_coef) {
  CHECK_GPU(dz); CHECK_BF16(dz); CHECK_BF16(h); CHECK_BF16(w); CHECK_BF16(dh_out); CHECK_BF16(bn_x);
  CHECK_CONTIG(dz); CHECK_CONTIG(h); CHECK_CONTIG(w); CHECK_CONTIG(dh_out); CHECK_CONTIG(bn_x);
  CHECK_F32(bcoef); CHECK_F32(bn_coef);
  TORCH_CHECK(dz.dim() == 4 && w.dim() == 4 && w.size(1) == 1 && w.size(2) == 1 && w.size(0) == dz.size(3),
              "conv1x1_bnin_dgrad: NHWC dz / [K,1,1,C] w shape mismatch");
  TORCH_CHECK(h.sizes() == dz.sizes() && dh_out.sizes() == dz.sizes(), "conv1x1_bnin_dgrad: h / dh_out must have dz's shape");
  const int64_t K = dz.size(3), C = w.size(3);
  TORCH_CHECK(bcoef.numel() == 3 * K, "bcoef must be [3][K]");
  TORCH_CHECK(K % 32 == 0 && K <= 2048 && C % 8 == 0, "conv1x1_bnin_dgrad: K % 32 == 0, K <= 2048");
  TORCH_CHECK(bn_x.dim() == 4 && bn_x.size(0) == dz.size(0) && bn_x.size(1) == dz.size(1) && bn_x.size(2) == dz.size(2) &&
                  bn_x.size(3) == C && bn_coef.numel() == 4 * C,
              "conv1x1_bnin_dgrad: bn_x must be [N,H,W,C], bn_coef [4][C]");
  Tensor dx = at::empty_like(bn_x);
  auto a = base_args();
  a.g = geom(dx, w, 1, 1, 0, 0, 1, 1, dz.size(1), dz.size(2));
  a.A = bp(dz); a.B = bp(w); a.C = dx.data_ptr();
  a.M = (int)(dz.numel() / K); a.N = (int)C; a.K = (int)K;
  a.lda = K; a.ldb = C; a.ldc = C;
  a.k_split = a.K;
  a.a_mode = dpe::AX_BN_BWD;
  a.a2 = bp(h); a.a_coef = fp(bcoef); a.a_out = bpm(dh_out);
  a.st_x = bp(bn_x); a.st_coef = fp(bn_coef);
  const int64_t tiles_m = (a.M + 127) / 128;
  Tensor part = at::empty({2, C, tiles_m}, dz.options().dtype(at::kFloat));
  a.col_stats = fp(part);
  a.stats_ld = (int)tiles_m;
  const int bn = C <= 64 ? 64 : 128;
  CHECK_RC(dpe_igemm_dma_launch(&a, 128, bn, dpe::A_DENSE_K, dpe::B_DENSE_N, dpe::EPI_BF16_BNB, cur_stream()),
           "conv1x1_bnin_dgrad");
  return {dx, part};
}

// Two BatchNorms fed by the same dz (a downsample bottleneck: BN3 and BN_d both see dz3):
// BN3's backward from its epilogue partials, BN_d's reduce fused into BN3's apply pass
// (dz read once for both), then BN_d's apply.  Returns (dx, dx2).
std::vector<Tensor> bn_bwd_dual(const Tensor& dz, const Tensor& x, const c10::optional<Tensor>& gamma, const Tensor& coef,
                                const Tensor& partials, const c10::optional<Tensor>& dgamma,
                                const c10::optional<Tensor>& dbeta, const Tensor& x2, const c10::optional<Tensor>& gamma2,
                                const Tensor& coef2, const c10::optional<Tensor>& dgamma2, const c10::optional<Tensor>& dbeta2) {
  CHECK_GPU(dz); CHECK_BF16(dz); CHECK_CONTIG(dz); CHECK_BF16(x); CHECK_CONTIG(x); CHECK_BF16(x2); CHECK_CONTIG(x2);
  TORCH_CHECK(dz.sizes() == x.sizes() && dz.sizes() == x2.sizes(), "bn_bwd_dual: dz / x / x2 shape mismatch");
  const int64_t C = x.size(-1), M = rows_of(x);
  TORCH_CHECK(partials.dim() == 3 && partials.size(0) == 2 && partials.size(1) == C, "partials must be [2][C][nb]");
  hipStream_t st = cur_stream();
  auto fo = x.options().dtype(at::kFloat);
  Tensor bcoef = at::empty({3, C}, fo);
  CHECK_RC(dpe_bn_bwd_finalize(fp(partials), (int)partials.size(2), (int)C, M, fpo(gamma), fp(coef), fpom(dgamma),
                               fpom(dbeta), fp(bcoef), st), "bn_bwd_finalize");
  const int nb = dpe_bn_bwd_nblocks(M, (int)C);
  Tensor part2 = at::empty({2, C, nb}, fo);
  Tensor dx = at::empty_like(x);
  CHECK_RC(dpe_bn_bwd_reduce_apply(bp(dz), bp(x2), fp(coef2), bp(x), fp(bcoef), bpm(dx), M, (int)C, nb, fp(part2), st),
           "bn_bwd_reduce_apply");
  Tensor bcoef2 = at::empty({3, C}, fo);
  CHECK_RC(dpe_bn_bwd_finalize(fp(part2), nb, (int)C, M, fpo(gamma2), fp(coef2), fpom(dgamma2), fpom(dbeta2), fp(bcoef2), st),
           "bn_bwd_finalize");
  Tensor dx2 = at::empty_like(x2);
  CHECK_RC(dpe_bn_bwd_apply(bp(dz), nullptr, nullptr, bp(x2), fp(bcoef2), bpm(dx2), nullptr, M, (int)C, nullptr, st),
           "bn_bwd_apply");
  return {dx, dx2};
}

// ----------------------------------------------------------------- pooling
std::vector<Tensor> maxpool_fwd(const Tensor& x, int64_t k, int64_t s, int64_t p) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_CONTIG(x);
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int64_t OH = (H + 2 * p - k) / s + 1, OW = (W + 2 * p - k) / s + 1;
  Tensor y = at::empty({N, OH, OW, C}, x.options());
  Tensor idx = at::empty({N, OH, OW, C}, x.options().dtype(at::kByte));
  CHECK_RC(dpe_maxpool_fwd(bp(x), bpm(y), (uint8_t*)idx.data_ptr(), (int)N, (int)H, (int)W, (int)C, (int)OH, (int)OW, (int)k,
                           (int)s, (int)p, cur_stream()), "maxpool_fwd");
  return {y, idx};
}

Tensor maxpool_bwd(const Tensor& dy, const Tensor& idx, std::vector<int64_t> xshape, int64_t k, int64_t s, int64_t p) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_CONTIG(dy);
  Tensor dx = at::empty(xshape, dy.options());
  CHECK_RC(dpe_maxpool_bwd(bp(dy), (const uint8_t*)idx.data_ptr(), bpm(dx), (int)xshape[0], (int)xshape[1], (int)xshape[2],
                           (int)xshape[3], (int)dy.size(1), (int)dy.size(2), (int)k, (int)s, (int)p, cur_stream()),
           "maxpool_bwd");
  return dx;
}

// y = act(BN(x; coef) + r), r = residual (bf16) or, with residual_coef, BN(residual; residual_coef)
// computed in the same pass (bottleneck output with a BN'd downsample branch).
// want_mask: also the ReLU-mask bits of y, uint8 [.., C/8] (bit e of byte j = y[.., 8j+e] > 0).
std::vector<Tensor> bn_apply(const Tensor& x, const Tensor& coef, const c10::optional<Tensor>& residual,
                             const c10::optional<Tensor>& residual_coef, bool relu, bool want_mask) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_CONTIG(x); CHECK_F32(coef);
  const int64_t C = x.size(-1);
  TORCH_CHECK(C % 8 == 0 && coef.numel() == 4 * C, "bn_apply: coef must be [4][C], C % 8 == 0");
  const bool has_res = has(residual);
  if (has_res) {
    CHECK_BF16((*residual)); CHECK_CONTIG((*residual));
    TORCH_CHECK(residual->sizes() == x.sizes(), "bn_apply: residual shape mismatch");
  }
  Tensor y = at::empty_like(x);
  Tensor bits;
  if (want_mask) {
    auto sz = x.sizes().vec();
    sz.back() = C / 8;
    bits = at::empty(sz, x.options().dtype(at::kByte));
  }
  uint8_t* mb = want_mask ? (uint8_t*)bits.data_ptr() : nullptr;
  if (has(residual_coef)) {
    TORCH_CHECK(has_res, "bn_apply: residual_coef needs a residual");
    CHECK_F32((*residual_coef));
    TORCH_CHECK(residual_coef->numel() == 4 * C, "bn_apply: residual_coef must be [4][C]");
    CHECK_RC(dpe_bn_apply2(bp(x), fp(coef), bp(*residual), fp(*residual_coef), bpm(y), rows_of(x), (int)C, relu ? 1 : 0, mb,
                           cur_stream()), "bn_apply2");
  } else {
    CHECK_RC(dpe_bn_apply_m(bp(x), has_res ? bp(*residual) : nullptr, bpm(y), rows_of(x), (int)C, fp(coef), relu ? 1 : 0, mb,
                            cur_stream()), "bn_apply");
  }
  return {y, bits};
}

// Stem fusion: maxpool(relu(BN(h))) with BN coefficients `coef` [4][C] (bn_coef);
// the BN+ReLU output is never materialised.  Returns (pooled, argmax bytes).
std::vector<Tensor> bnrelu_maxpool_fwd(const Tensor& h, const Tensor& coef, int64_t k, int64_t s, int64_t p) {
  CHECK_GPU(h); CHECK_BF16(h); CHECK_CONTIG(h); CHECK_F32(coef);
  const int64_t N = h.size(0), H = h.size(1), W = h.size(2), C = h.size(3);
  TORCH_CHECK(coef.numel() == 4 * C, "bnrelu_maxpool_fwd: coef must be [4][C]");
  const int64_t OH = (H + 2 * p - k) / s + 1, OW = (W + 2 * p - k) / s + 1;
  Tensor y = at::empty({N, OH, OW, C}, h.options());
  Tensor idx = at::empty({N, OH, OW, C}, h.options().dtype(at::kByte));
  CHECK_RC(dpe_bnrelu_maxpool_fwd(bp(h), fp(coef), bpm(y), (uint8_t*)idx.data_ptr(), (int)N, (int)H, (int)W, (int)C, (int)OH,
                                  (int)OW, (int)k, (int)s, (int)p, cur_stream()), "bnrelu_maxpool_fwd");
  return {y, idx};
}

// Backward of the fused stem: dh = BN'(relu'(h) * maxpool'(dy)); dgamma/dbeta accumulate.
Tensor maxpool_bn_bwd(const Tensor& dy, const Tensor& idx, const Tensor& h, const c10::optional<Tensor>& gamma,
                      const Tensor& coef, const c10::optional<Tensor>& dgamma, const c10::optional<Tensor>& dbeta, int64_t k,
                      int64_t s, int64_t p) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_CONTIG(dy); CHECK_BF16(h); CHECK_CONTIG(h); CHECK_F32(coef);
  TORCH_CHECK(idx.scalar_type() == at::kByte && idx.sizes() == dy.sizes(), "maxpool_bn_bwd: idx must be uint8 of dy's shape");
  const int64_t N = h.size(0), H = h.size(1), W = h.size(2), C = h.size(3);
  TORCH_CHECK(dy.size(0) == N && dy.size(3) == C, "maxpool_bn_bwd: dy/h shape mismatch");
  const int64_t M = N * H * W;
  hipStream_t st = cur_stream();
  auto fo = h.options().dtype(at::kFloat);
  // the gather makes each row latency-heavy: ~16 rows per thread-row-phase, up to 8192 partial blocks
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(8192, M / 512));
  Tensor part = at::empty({2, C, nb}, fo);
  CHECK_RC(dpe_maxpool_bn_bwd_reduce(bp(dy), (const uint8_t*)idx.data_ptr(), bp(h), fp(coef), (int)N, (int)H, (int)W, (int)C,
                                     (int)dy.size(1), (int)dy.size(2), (int)k, (int)s, (int)p, nb, fp(part), st),
           "maxpool_bn_bwd_reduce");
  Tensor bcoef = at::empty({3, C}, fo);
  CHECK_RC(dpe_bn_bwd_finalize(fp(part), nb, (int)C, M, fpo(gamma), fp(coef), fpom(dgamma), fpom(dbeta), fp(bcoef), st),
           "bn_bwd_finalize");
  Tensor dh = at::empty_like(h);
  CHECK_RC(dpe_maxpool_bn_bwd_apply(bp(dy), (const uint8_t*)idx.data_ptr(), bp(h), fp(coef), fp(bcoef), bpm(dh), (int)N,
                                    (int)H, (int)W, (int)C, (int)dy.size(1), (int)dy.size(2), (int)k, (int)s, (int)p, st),
           "maxpool_bn_bwd_apply");
  return dh;
}

// The stem's backward without dY: BN-backward coefficients of the pooled gradient (reduce + finalize; dgamma /
// dbeta accumulate), then the stem weight grad computing dY = a dz + b h + c on the fly (stem.hip FUSED).
// dw [64, 4, 4, 16] (s2d filter layout) += dW.  No dY tensor, no apply pass.
void stem_bwd_fused(const Tensor& dy, const Tensor& idx, const Tensor& h, const Tensor& xs,
                    const c10::optional<Tensor>& gamma, const Tensor& coef, const c10::optional<Tensor>& dgamma,
                    const c10::optional<Tensor>& dbeta, Tensor& dw) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_CONTIG(dy); CHECK_BF16(h); CHECK_CONTIG(h); CHECK_F32(coef); CHECK_BF16(xs);
  CHECK_CONTIG(xs); CHECK_F32(dw); CHECK_CONTIG(dw);
  TORCH_CHECK(idx.scalar_type() == at::kByte && idx.sizes() == dy.sizes(), "stem_bwd_fused: idx must be uint8 of dy's shape");
  const int64_t N = h.size(0), H = h.size(1), W = h.size(2), C = h.size(3);
  TORCH_CHECK(C == 64 && dy.size(0) == N && dy.size(1) == H / 2 && dy.size(2) == W / 2 && dy.size(3) == C && H % 2 == 0 &&
                  W % 2 == 0 && xs.size(0) == N && xs.size(1) == H && xs.size(2) == W && xs.size(3) == 16 &&
                  dw.numel() == 64 * 256,
              "stem_bwd_fused: shapes (h [N,H,W,64], dy/idx [N,H/2,W/2,64], xs [N,H,W,16], dw [64,4,4,16])");
  const int64_t M = N * H * W;
  hipStream_t st = cur_stream();
  auto fo = h.options().dtype(at::kFloat);
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(8192, M / 512));
  Tensor part = at::empty({2, C, nb}, fo);
  CHECK_RC(dpe_maxpool_bn_bwd_reduce(bp(dy), (const uint8_t*)idx.data_ptr(), bp(h), fp(coef), (int)N, (int)H, (int)W, (int)C,
                                     (int)dy.size(1), (int)dy.size(2), 3, 2, 1, nb, fp(part), st),
           "maxpool_bn_bwd_reduce");
  Tensor bcoef = at::empty({3, C}, fo);
  CHECK_RC(dpe_bn_bwd_finalize(fp(part), nb, (int)C, M, fpo(gamma), fp(coef), fpom(dgamma), fpom(dbeta), fp(bcoef), st),
           "bn_bwd_finalize");
  auto scratch = at::empty({dpe_stem_wgrad_scratch(N, H, W)}, fo);
  CHECK_RC(dpe_stem_wgrad_launch2(bp(xs), nullptr, fp(dw), fp(scratch), (int)N, (int)H, (int)W, 1.f, bp(dy),
                                  (const uint8_t*)idx.data_ptr(), bp(h), fp(coef), fp(bcoef), st),
           "stem wgrad (fused BN / max-pool backward)");
}

Tensor gavgpool_fwd(const Tensor& x) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_CONTIG(x);
  const int64_t N = x.size(0), C = x.size(-1), HW = x.numel() / (N * C);
  Tensor y = at::empty({N, C}, x.options());
  CHECK_RC(dpe_gavgpool_fwd(bp(x), bpm(y), (int)N, (int)HW, (int)C, cur_stream()), "gavgpool_fwd");
  return y;
}

Tensor gavgpool_bwd(const Tensor& dy, std::vector<int64_t> xshape) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_CONTIG(dy);
  Tensor dx = at::empty(xshape, dy.options());
  const int64_t N = xshape[0], C = xshape.back(), HW = dx.numel() / (N * C);
  CHECK_RC(dpe_gavgpool_bwd(bp(dy), bpm(dx), (int)N, (int)HW, (int)C, cur_stream()), "gavgpool_bwd");
  return dx;
}

}  // namespace

void register_bn(pybind11::module& m) {
  namespace py = pybind11;
  m.def("gram_ok", [](std::vector<int64_t> h2shape, int64_t cout3, int64_t next_width) {
          // BN3 by Gram algebra for a bottleneck whose conv3 input is h2 [N, H, W, C2] (bngram.hip): conv3's
          // forward with the BN3 + residual + ReLU epilogue on the streaming kernel (PW_APPLY), its data
          // grad as the concatenated-K LDS-DMA GEMM, and the next block's conv1 data grad (K = next_width ->
          // cout3) emitting the sum-dz partials (PW_DSUM)
          if (h2shape.size() != 4 || !pw_stream_on()) return false;
          const int64_t M = h2shape[0] * h2shape[1] * h2shape[2], C2 = h2shape[3];
          if (C2 != 64 && C2 != 128 && C2 != 256) return false;
          if (cout3 % 128 || M % 32) return false;
          return dpe_pw_rowgroups(M, cout3, C2, dpe::PW_APPLY) > 0 &&
                 dpe_pw_rowgroups(M, cout3, next_width, dpe::PW_DSUM) > 0;
        }, py::arg("h2_shape"), py::arg("cout3"), py::arg("next_width"));
  m.def("bn_gram", &bn_gram, py::arg("x"), py::arg("coef") = py::none(), py::arg("shift_coef") = py::none(),
        py::arg("stride2") = false,
        "(G = a'^T a', s = [colsum(a'), mu]) of a' = a2 - mu, a2 = relu(x * coef[0] + coef[1]) (or x), centred on the "
        "pilot shift of shift_coef (default coef); fp32, deterministic");
  m.def("bn_gram_coef", &bn_gram_coef, py::arg("G"), py::arg("s"), py::arg("w"), py::arg("M"), py::arg("gamma"),
        py::arg("beta"), py::arg("running_mean"), py::arg("running_var"), py::arg("momentum"), py::arg("eps"),
        "BN coefficients [4][Cout] of the never-computed h = a2 W^T from (G, s), and u = W G");
  m.def("conv1x1_apply", &conv1x1_apply, py::arg("x"), py::arg("w"), py::arg("in_coef"), py::arg("out_coef"),
        py::arg("residual"), py::arg("res_coef") = py::none(),
        "y = relu(BN(x' W^T) + residual [BN_d]) and its ReLU bits (pre-BN tensor never stored)");
  m.def("conv1x1_apply_next", &conv1x1_apply_next, py::arg("x"), py::arg("w"), py::arg("in_coef"), py::arg("out_coef"),
        py::arg("residual"), py::arg("res_coef"), py::arg("w_next"), py::arg("outs") = py::none(),
        "conv1x1_apply's (y, bits) and, from the same pass, the next conv1's h1 = y W_next^T with its BN-forward partials");
  m.def("c1_fuse_ok", &c1_fuse_ok, py::arg("h2_shape"), py::arg("cout3"), py::arg("c1_next"),
        "conv1x1_apply_next's envelope: conv3 64 -> 256 beside a 1x1 stride-1 conv1 256 -> {64, 128}; no CU budget");
  m.def("conv1x1_apply_cat", &conv1x1_apply_cat, py::arg("x"), py::arg("w"), py::arg("in_coef"), py::arg("out_coef"),
        py::arg("x2"), py::arg("w2"), py::arg("coef2"),
        "y = relu(BN3(x' W^T) + BN_d(x2 W2^T)) over the concatenated K and its ReLU bits (no pre-BN tensors)");
  m.def("down_cat_ok", &down_cat_ok, py::arg("xshape"), py::arg("cmid"), py::arg("cout"), py::arg("stride"),
        "conv1x1_apply_cat's envelope: 1x1 stride-1 downsample conv, Cin == cmid in {64, 128}, cout == 4 Cin");
  m.def("bn_gram_bwd", &bn_gram_bwd, py::arg("part"), py::arg("P"), py::arg("w"), py::arg("u"), py::arg("s"),
        py::arg("coef"), py::arg("gamma"), py::arg("M"), py::arg("dgamma"), py::arg("dbeta"), py::arg("dw"),
        "BN3 backward from (sum dz partials, P = dz^T a2): dgamma/dbeta/dw +=, returns (B_cat bf16, bias)");
  m.def("conv1x1_dgrad_cat", &conv1x1_dgrad_cat, py::arg("dz"), py::arg("a2src"), py::arg("a2_coef"), py::arg("bcat"),
        py::arg("e"), py::arg("bn_x"), py::arg("bn_coef"),
        "[dz | a2] x bcat + e with the BN2-backward partials (concatenated-K data grad)");
  m.def("bn_gram_pilot", &bn_gram_pilot, py::arg("x"), py::arg("stride2") = false,
        "pilot shift [4][C] for bn_gram's shift_coef from a sample of x's rows (x without a producing BN)");
  m.def("bn_gram_u", &bn_gram_u, py::arg("G"), py::arg("w"), "u = W G (fp32) alone: no coefficients, no running stats");
  m.def("conv1x1_dgrad_cat_plain", &conv1x1_dgrad_cat_plain, py::arg("dz"), py::arg("x"), py::arg("bcat"), py::arg("e"),
        py::arg("stride2") = false,
        "[dz | x] x bcat + e (concatenated-K data grad of a Gram-path downsample branch, no partials)");
  m.def("bnd_gram_ok", [](std::vector<int64_t> xshape, int64_t cout, std::vector<int64_t> stride) {
          // the downsample BN by Gram algebra for a 1x1 stride-1 downsample conv over x [N, H, W, Cin]: the Gram
          // pass over x, the deterministic LDS-DMA weight grad P_d = dz3^T x, and the streaming concatenated-K
          // data grad (Cin -> 4 Cin, Cin in {64, 128})
          // stride 2 (layer2.0: 256 -> 512 over the even pixels): the Gram pass and the data grad's second segment
          // address the subsample of x by rows (LDS-DMA kernels), and P_d runs on the persistent GEMM's
          // implicit-im2col weight grad (fixed-order slabs), whose envelope is tested here
          if (xshape.size() != 4 || stride.size() != 2 || stride[0] != stride[1] || !igemm_dma_on()) return false;
          const int64_t M = xshape[0] * xshape[1] * xshape[2], C = xshape[3];
          // (stride 1: P_d's LDS-DMA weight grad needs Cout, C % 8 and M Cout 2 B < 2^31 -- the channel test and
          // dpe_pw_cat_blocks' own size limit imply both)
          if (stride[0] == 1) return (C == 64 || C == 128) && cout == 4 * C && dpe_pw_cat_blocks(M, cout, C) > 0;
          if (stride[0] != 2 || xshape[1] % 2 || xshape[2] % 2) return false;
          static const bool gdma = env_on("DPE_GRAM_DMA", true);
          const int64_t Mo = M / 4, lim = (1ll << 31) - 4096;
          return gdma && (C == 64 || C == 128 || C == 256) && cout >= 256 && cout % 32 == 0 && hgemm_conv_on() &&
                 hgemm_conv_wgrad_on() && Mo % 64 == 0 && Mo < (1 << 24) && M * C * 2 < lim && Mo * cout * 2 < lim;
        }, py::arg("xshape"), py::arg("cout"), py::arg("stride"));
  m.def("bn_bwd_coef", &bn_bwd_coef, py::arg("partials"), py::arg("M"), py::arg("gamma"), py::arg("coef"),
        py::arg("dgamma") = py::none(), py::arg("dbeta") = py::none(),
        "BN-backward coefficients [3][C] from the dgrad-epilogue partials (no apply pass); dgamma/dbeta +=");
  m.def("conv1x1_bnin_fwd", &conv1x1_bnin_fwd, py::arg("h"), py::arg("res"), py::arg("coef"), py::arg("res_coef"),
        py::arg("w"), py::arg("x_out"), py::arg("x_bits"), py::arg("want_stats") = true, py::arg("tile_m") = 128,
        "1x1 conv over x = relu(BN(h) + res [BN_d]) computed on load; x (+ ReLU bits) stored as a by-product");
  m.def("conv1x1_bnin_dgrad", &conv1x1_bnin_dgrad, py::arg("dz"), py::arg("h"), py::arg("bcoef"), py::arg("w"),
        py::arg("dh_out"), py::arg("bn_x"), py::arg("bn_coef"),
        "1x1 data grad over dh = a*dz + b*h + c computed on load (dh stored as a by-product) + BN-backward partials");
  m.def("bn_coef", &bn_coef, py::arg("stats"), py::arg("M"), py::arg("gamma"), py::arg("beta"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("momentum"), py::arg("eps"));
  m.def("bn_apply", &bn_apply, py::arg("x"), py::arg("coef"), py::arg("residual") = py::none(),
        py::arg("residual_coef") = py::none(), py::arg("relu") = true, py::arg("want_mask") = false);
  m.def("bnrelu_maxpool_fwd", &bnrelu_maxpool_fwd, py::arg("h"), py::arg("coef"), py::arg("k"), py::arg("s"), py::arg("p"));
  m.def("set_pool_legacy", [](bool on) { dpe_set_pool_legacy(on ? 1 : 0); },
        "test hook: the stem max-pool on the reference (per-tap compare) kernel instead of the key-max one");
  m.def("stem_bwd_fused", &stem_bwd_fused, py::arg("dy"), py::arg("idx"), py::arg("h"), py::arg("xs"), py::arg("gamma"),
        py::arg("coef"), py::arg("dgamma"), py::arg("dbeta"), py::arg("dw"),
        "stem backward without dY: BN-backward coefficients of the pooled gradient, then the stem weight grad "
        "(s2d filter layout) computing dY on the fly");
  m.def("maxpool_bn_bwd", &maxpool_bn_bwd, py::arg("dy"), py::arg("idx"), py::arg("h"), py::arg("gamma"), py::arg("coef"),
        py::arg("dgamma"), py::arg("dbeta"), py::arg("k"), py::arg("s"), py::arg("p"));
  m.def("bn_bwd_partials", &bn_bwd_partials, py::arg("dy"), py::arg("x"), py::arg("gamma"), py::arg("coef"),
        py::arg("partials"), py::arg("dgamma") = py::none(), py::arg("dbeta") = py::none(), py::arg("relu_mask") = true);
  m.def("bn_fwd_train", &bn_fwd_train, py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("rmean"), py::arg("rvar"),
        py::arg("momentum"), py::arg("eps"), py::arg("relu"), py::arg("residual") = py::none(), py::arg("stats") = py::none());
  m.def("bn_fwd_eval", &bn_fwd_eval, py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("rmean"), py::arg("rvar"),
        py::arg("eps"), py::arg("relu"), py::arg("residual") = py::none());
  m.def("bn_bwd_dual", &bn_bwd_dual, py::arg("dz"), py::arg("x"), py::arg("gamma"), py::arg("coef"), py::arg("partials"),
        py::arg("dgamma"), py::arg("dbeta"), py::arg("x2"), py::arg("gamma2"), py::arg("coef2"), py::arg("dgamma2"),
        py::arg("dbeta2"), "backward of two BatchNorms fed by one dz (BN3 + downsample BN): dz read once for both");
  m.def("bn_bwd", &bn_bwd, py::arg("dy"), py::arg("y"), py::arg("x"), py::arg("gamma"), py::arg("coef"), py::arg("dgamma"),
        py::arg("dbeta"), py::arg("want_dz") = false, py::arg("y_bits") = py::none());
  m.def("maxpool_fwd", &maxpool_fwd);
  m.def("maxpool_bwd", &maxpool_bwd);
  m.def("gavgpool_fwd", &gavgpool_fwd);
  m.def("gavgpool_bwd", &gavgpool_bwd);
}

}  // namespace dpe_ops
