// Bindings of the generation kernels (csrc/kernels/decode.hip): attn_decode, linear_skinny, sample_logits.
#include "ops_common.h"

namespace dpe_ops {
namespace {

bool aligned16(const Tensor& t) { return ((uintptr_t)t.data_ptr() & 15) == 0; }

// qkv_step [B, 3, H, 64] bf16, kc / vc [B, H, Tmax, 64] bf16 (updated in place at row len[b]), len int32 [B]
Tensor attn_decode(const Tensor& qkv_step, Tensor& kc, Tensor& vc, const Tensor& len, double scale, int64_t splits,
                   const c10::optional<Tensor>& out_opt) {
  CHECK_GPU(qkv_step); CHECK_BF16(qkv_step); CHECK_CONTIG(qkv_step);
  CHECK_GPU(kc); CHECK_BF16(kc); CHECK_CONTIG(kc);
  CHECK_GPU(vc); CHECK_BF16(vc); CHECK_CONTIG(vc);
  CHECK_GPU(len); CHECK_CONTIG(len);
  TORCH_CHECK(qkv_step.dim() == 4 && qkv_step.size(1) == 3 && qkv_step.size(3) == 64, "attn_decode: qkv_step must be [B, 3, H, 64]");
  const int64_t B = qkv_step.size(0), H = qkv_step.size(2);
  TORCH_CHECK(kc.dim() == 4 && kc.size(0) == B && kc.size(1) == H && kc.size(3) == 64 && kc.sizes() == vc.sizes(),
              "attn_decode: the cache must be [B, H, Tmax, 64] twice");
  TORCH_CHECK(len.scalar_type() == at::kInt && len.numel() == B, "attn_decode: len must be int32 [B]");
  TORCH_CHECK(aligned16(qkv_step) && aligned16(kc) && aligned16(vc), "attn_decode: 16-byte aligned tensors");
  const int64_t Tmax = kc.size(2);
  const int S = splits > 0 ? (int)splits : dpe_attn_decode_splits((int)(B * H), (int)Tmax);
  TORCH_CHECK(S >= 1 && S <= 1024, "attn_decode: splits out of range");
  Tensor out;
  if (has(out_opt)) {
    out = *out_opt;
    CHECK_GPU(out); CHECK_BF16(out); CHECK_CONTIG(out);
    TORCH_CHECK(out.numel() == B * H * 64, "attn_decode: out must be [B, H * 64]");
  } else {
    out = at::empty({B, H * 64}, qkv_step.options());
  }
  Tensor ws;
  if (S > 1) ws = at::empty({dpe_attn_decode_ws_floats((int)(B * H), S)}, qkv_step.options().dtype(at::kFloat));
  CHECK_RC(dpe_attn_decode(bp(qkv_step), bpm(kc), bpm(vc), (const int32_t*)len.data_ptr(), (int)B, (int)H, (int)Tmax, S,
                           (float)scale, S > 1 ? fp(ws) : nullptr, bpm(out), cur_stream()),
           "attn_decode");
  return out;
}

int64_t attn_decode_splits(int64_t BH, int64_t Tmax) { return dpe_attn_decode_splits((int)BH, (int)Tmax); }

int resolve_ksplit(int64_t M, int64_t N, int64_t K, int64_t ksplit) {
  return ksplit > 0 ? (int)ksplit : dpe_linear_skinny_ksplit((int)M, (int)N, (int)K);
}

bool linear_skinny_ok(int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldw) {
  return dpe_linear_skinny_ok((int)M, (int)N, (int)K, ldx, ldw) != 0;
}

// the number of K partials added per output: the waves of a block times the blocks along K
int64_t linear_skinny_splits(int64_t M, int64_t N, int64_t K, int64_t ksplit) {
  return (int64_t)dpe_linear_skinny_waves() * resolve_ksplit(M, N, K, ksplit);
}

// x [M, K] bf16 (row stride a multiple of 8), w [N, K] bf16 -> y [M, N]: bf16 (bias, GELU) or fp32 (bias, residual);
// ``out``: the fp32 destination, which may be the residual itself
Tensor linear_skinny(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias, bool gelu, bool out_f32,
                     const c10::optional<Tensor>& residual, const c10::optional<Tensor>& out, int64_t ksplit) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_GPU(w); CHECK_BF16(w);
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1), "linear_skinny: x [M, K], w [N, K]");
  TORCH_CHECK(x.stride(1) == 1 && w.stride(1) == 1, "linear_skinny: K-contiguous operands");
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  const int64_t ldx = M > 1 ? x.stride(0) : K, ldw = N > 1 ? w.stride(0) : K;
  TORCH_CHECK(linear_skinny_ok(M, N, K, ldx, ldw),
              "linear_skinny: outside the envelope (M <= 16, K % 32 == 0, N % 16 == 0, row strides % 8 == 0): M=", M, " N=", N,
              " K=", K, " ldx=", ldx, " ldw=", ldw);
  TORCH_CHECK(aligned16(x) && aligned16(w), "linear_skinny: 16-byte aligned operands");
  TORCH_CHECK(!(gelu && out_f32), "linear_skinny: GELU is a bf16 epilogue");
  TORCH_CHECK(!has(residual) || out_f32, "linear_skinny: the residual is an fp32 epilogue");
  if (has(bias)) { CHECK_GPU(*bias); CHECK_F32(*bias); CHECK_CONTIG(*bias); TORCH_CHECK(bias->numel() == N, "linear_skinny: bias [N]"); }
  int64_t ldr = 0;
  if (has(residual)) {
    CHECK_GPU(*residual); CHECK_F32(*residual); CHECK_CONTIG(*residual);
    TORCH_CHECK(residual->numel() == M * N, "linear_skinny: residual [M, N]");
    ldr = N;
  }
  Tensor y;
  if (has(out)) {
    y = *out;
    CHECK_GPU(y); CHECK_CONTIG(y);
    TORCH_CHECK(y.numel() == M * N && y.scalar_type() == (out_f32 ? at::kFloat : at::kBFloat16), "linear_skinny: out [M, N]");
  } else {
    y = at::empty({M, N}, x.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
  }
  const int ks = resolve_ksplit(M, N, K, ksplit);
  TORCH_CHECK(ks >= 1 && ks <= K / 32, "linear_skinny: ksplit out of range");
  Tensor ws;
  if (ks > 1) ws = at::empty({(int64_t)ks * M * N}, x.options().dtype(at::kFloat));
  CHECK_RC(dpe_linear_skinny(bp(x), ldx, bp(w), ldw, (int)M, (int)N, (int)K, fpo(bias), gelu ? 1 : 0, out_f32 ? 1 : 0,
                             fpo(residual), ldr, y.data_ptr(), N, ks, ks > 1 ? fp(ws) : nullptr, cur_stream()),
           "linear_skinny");
  return y;
}

// logits [B, ld] bf16 / fp32 (row stride a multiple of 8, >= V rounded up to 8), rng int64 [2], done int32 [B] -> int64 [B]
Tensor sample_logits(const Tensor& logits, int64_t V, double temperature, int64_t top_k, double top_p, const Tensor& rng,
                     int64_t stream, int64_t eos_id, const c10::optional<Tensor>& done) {
  CHECK_GPU(logits); CHECK_GPU(rng); CHECK_CONTIG(rng);
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1, "sample_logits: logits [B, ld]");
  const bool bf = logits.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf || logits.scalar_type() == at::kFloat, "sample_logits: bf16 or fp32 logits");
  TORCH_CHECK(rng.scalar_type() == at::kLong && rng.numel() == 2, "sample_logits: rng must be int64 [2]");
  const int64_t B = logits.size(0), ld = B > 1 ? logits.stride(0) : logits.size(1);
  TORCH_CHECK(V >= 1 && V <= logits.size(1) && V <= 65536, "sample_logits: V out of range");
  TORCH_CHECK(ld % 8 == 0 && logits.size(1) >= (V + 7) / 8 * 8 && aligned16(logits),
              "sample_logits: rows must be 16-byte aligned and padded to a multiple of 8 columns");
  TORCH_CHECK(temperature >= 0.0 && top_k >= 0 && top_p > 0.0 && top_p <= 1.0, "sample_logits: temperature >= 0, top_k >= 0, 0 < top_p <= 1");
  int32_t* dn = nullptr;
  if (has(done)) {
    CHECK_GPU(*done); CHECK_CONTIG(*done);
    TORCH_CHECK(done->scalar_type() == at::kInt && done->numel() == B, "sample_logits: done must be int32 [B]");
    dn = (int32_t*)done->data_ptr();
  }
  Tensor out = at::empty({B}, logits.options().dtype(at::kLong));
  CHECK_RC(dpe_sample_logits(logits.data_ptr(), bf ? 1 : 0, (int)B, (int)V, ld, (float)temperature, (int)top_k, (float)top_p,
                             (const int64_t*)rng.data_ptr(), (uint32_t)stream, (int)eos_id, dn, (int64_t*)out.data_ptr(),
                             cur_stream()),
           "sample_logits");
  return out;
}

}  // namespace

void register_decode(pybind11::module& m) {
  namespace py = pybind11;
  m.def("attn_decode", &attn_decode, py::arg("qkv_step"), py::arg("kc"), py::arg("vc"), py::arg("len"), py::arg("scale"),
        py::arg("splits") = 0, py::arg("out") = py::none(), "single-query attention against the KV cache; stores the step's K/V at row len[b]");
  m.def("attn_decode_splits", &attn_decode_splits, py::arg("BH"), py::arg("Tmax"));
  m.def("linear_skinny", &linear_skinny, py::arg("x"), py::arg("w"), py::arg("bias") = py::none(), py::arg("gelu") = false,
        py::arg("out_f32") = false, py::arg("residual") = py::none(), py::arg("out") = py::none(), py::arg("ksplit") = 0,
        "y = x w^T for M <= 16 rows (weight streaming)");
  m.def("linear_skinny_ok", &linear_skinny_ok, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("ldx"), py::arg("ldw"));
  m.def("linear_skinny_splits", &linear_skinny_splits, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("ksplit") = 0,
        "K partials added per output");
  m.def("sample_logits", &sample_logits, py::arg("logits"), py::arg("V"), py::arg("temperature"), py::arg("top_k"),
        py::arg("top_p"), py::arg("rng"), py::arg("stream") = 0, py::arg("eos_id") = -1, py::arg("done") = py::none(),
        "one token per row (temperature, top-k, top-p, Gumbel-max) on the device");
}
}  // namespace dpe_ops
