// Bindings of the depthwise 7x7 kernels (csrc/kernels/dwconv.hip): dwconv7_fwd, dwconv7_dgrad, dwconv7_wgrad.
#include "ops_common.h"

namespace dpe_ops {
namespace {

bool aligned16(const Tensor& t) { return ((uintptr_t)t.data_ptr() & 15) == 0; }

// x [N, H, W, C] bf16 or fp32, contiguous, C % 8 == 0; w49 [49, C] bf16
void check_operands(const Tensor& x, const Tensor& w49, const char* what) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_GPU(w49); CHECK_BF16(w49); CHECK_CONTIG(w49);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat, what, ": x must be bfloat16 or float32");
  TORCH_CHECK(x.dim() == 4 && x.numel() > 0, what, ": x must be a non-empty [N, H, W, C]");
  const int64_t C = x.size(3);
  TORCH_CHECK(C % 8 == 0, what, ": C must be a multiple of 8, got ", C);
  TORCH_CHECK(w49.dim() == 2 && w49.size(0) == 49 && w49.size(1) == C, what, ": the filter must be [49, C] tap-major");
  TORCH_CHECK(x.size(0) <= 65535 && x.size(1) < (1 << 24) && x.size(2) < (1 << 24) && C < (1 << 24), what, ": shape out of range");
  TORCH_CHECK(aligned16(x) && aligned16(w49), what, ": 16-byte aligned tensors");
}

Tensor rows(const Tensor& x, const Tensor& w49, const c10::optional<Tensor>& bias, const char* what) {
  check_operands(x, w49, what);
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  if (has(bias)) {
    CHECK_GPU(*bias); CHECK_F32(*bias); CHECK_CONTIG(*bias);
    TORCH_CHECK(bias->numel() == C, what, ": bias [C]");
  }
  Tensor y = at::empty({N, H, W, C}, x.options().dtype(at::kBFloat16));
  CHECK_RC(dpe_dwconv7_fwd(x.data_ptr(), x.scalar_type() == at::kFloat, bp(w49), fpo(bias), bpm(y), (int)N, (int)H, (int)W,
                           (int)C, cur_stream()),
           "dwconv7_rows");
  return y;
}

Tensor dwconv7_fwd(const Tensor& x, const Tensor& w49, const c10::optional<Tensor>& bias) {
  return rows(x, w49, bias, "dwconv7_fwd");
}

// w49_flipped: the taps in reverse order (the filter rotated by 180 degrees)
Tensor dwconv7_dgrad(const Tensor& dy, const Tensor& w49_flipped) {
  CHECK_BF16(dy);
  return rows(dy, w49_flipped, c10::nullopt, "dwconv7_dgrad");
}

// dw [C, 1, 7, 7] fp32 and db [C] fp32 (optional): written, or added to with ``accumulate``
void dwconv7_wgrad(const Tensor& dy, const Tensor& x, Tensor& dw, const c10::optional<Tensor>& db, bool accumulate) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_CONTIG(dy); CHECK_GPU(x); CHECK_CONTIG(x);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat, "dwconv7_wgrad: x must be bfloat16 or float32");
  TORCH_CHECK(x.dim() == 4 && x.numel() > 0 && dy.sizes() == x.sizes(), "dwconv7_wgrad: dy and x must be the same non-empty [N, H, W, C]");
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  TORCH_CHECK(C % 8 == 0, "dwconv7_wgrad: C must be a multiple of 8, got ", C);
  TORCH_CHECK(N <= 65535 && H < (1 << 24) && W < (1 << 24) && C < (1 << 24), "dwconv7_wgrad: shape out of range");
  TORCH_CHECK(aligned16(x) && aligned16(dy), "dwconv7_wgrad: 16-byte aligned tensors");
  CHECK_GPU(dw); CHECK_F32(dw); CHECK_CONTIG(dw);
  TORCH_CHECK(dw.numel() == C * 49 && dw.size(0) == C, "dwconv7_wgrad: dw must be [C, 1, 7, 7]");
  if (has(db)) {
    CHECK_GPU(*db); CHECK_F32(*db); CHECK_CONTIG(*db);
    TORCH_CHECK(db->numel() == C, "dwconv7_wgrad: db [C]");
  }
  const int64_t nb = dpe_dwconv7_wgrad_blocks((int)N, (int)H, (int)W, (int)C);
  TORCH_CHECK(nb > 0 && nb <= INT32_MAX, "dwconv7_wgrad: shape outside the envelope");
  Tensor part = at::empty({nb, C, 50}, x.options().dtype(at::kFloat));
  CHECK_RC(dpe_dwconv7_wgrad(bp(dy), x.data_ptr(), x.scalar_type() == at::kFloat, fp(part), fp(dw), fpom(db), accumulate,
                             (int)N, (int)H, (int)W, (int)C, cur_stream()),
           "dwconv7_wgrad");
}

}  // namespace

void register_dwconv(pybind11::module& m) {
  namespace py = pybind11;
  m.def("dwconv7_fwd", &dwconv7_fwd, py::arg("x"), py::arg("w49"), py::arg("bias") = py::none());
  m.def("dwconv7_dgrad", &dwconv7_dgrad, py::arg("dy"), py::arg("w49_flipped"));
  m.def("dwconv7_wgrad", &dwconv7_wgrad, py::arg("dy"), py::arg("x"), py::arg("dw"), py::arg("db") = py::none(),
        py::arg("accumulate") = false);
}
}  // namespace dpe_ops
