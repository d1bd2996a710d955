// Shared by the op bindings (conv.cpp, bn.cpp, ops.cpp, gemm.cpp); internal to csrc/bindings.  Nothing here holds
// state (a variable in a header exists once per translation unit): every switch and cache is defined in one .cpp
// and reached from the others through a function declared below.
#pragma once
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "../kernels/hgemm.h"
#include "../kernels/igemm.h"
#include "../kernels/launch.h"

#define CHECK_GPU(t) TORCH_CHECK((t).is_cuda(), #t " must be a GPU tensor")
#define CHECK_CONTIG(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")
#define CHECK_BF16(t) TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bfloat16")
#define CHECK_F32(t) TORCH_CHECK((t).scalar_type() == at::kFloat, #t " must be float32")
#define CHECK_RC(rc, what)                                                                          \
  do {                                                                                              \
    const int rc_ = (rc);                                                                           \
    const hipError_t e_ = hipGetLastError();                                                        \
    TORCH_CHECK(rc_ == 0 && e_ == hipSuccess, "dpe kernel launch failed: " what " rc=", rc_, " hip=", \
                hipGetErrorString(e_));                                                             \
  } while (0)

namespace dpe_ops {
using at::Tensor;

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }
// an optional tensor argument that was passed and is not an undefined tensor
inline bool has(const c10::optional<Tensor>& t) { return t.has_value() && t->defined(); }
inline const uint16_t* bp(const Tensor& t) { return (const uint16_t*)t.data_ptr(); }
inline uint16_t* bpm(const Tensor& t) { return (uint16_t*)t.data_ptr(); }
inline float* fp(const Tensor& t) { return (float*)t.data_ptr(); }
inline const float* fpo(const c10::optional<Tensor>& t) { return has(t) ? (const float*)t->data_ptr() : nullptr; }
inline float* fpom(const c10::optional<Tensor>& t) { return has(t) ? (float*)t->data_ptr() : nullptr; }

// An on/off environment switch.  Default on: only a value starting with '0' turns it off; default off: only '1' on.
inline bool env_on(const char* name, bool dflt) {
  const char* e = getenv(name);
  return dflt ? !(e && e[0] == '0') : (e && e[0] == '1');
}

// A default-on switch with a test hook: read from its environment variable at the first on() unless set() came
// first; set() overrides from then on.  Define each one in exactly one .cpp.
class Toggle {
  const char* env_;
  int v_ = -1;  // -1: not read yet
 public:
  constexpr explicit Toggle(const char* env) : env_(env) {}
  bool on() {
    if (v_ < 0) v_ = env_on(env_, true) ? 1 : 0;
    return v_ == 1;
  }
  void set(bool on) { v_ = on ? 1 : 0; }
};

// ---- defined in conv.cpp, also called by bn.cpp
dpe::IgemmArgs base_args();  // zeroed, alpha = 1
dpe::HgemmArgs hargs();      // zeroed, alpha = 1, splits = 1
dpe::ConvGeom geom(const Tensor& x, const Tensor& w, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw,
                   int64_t OH, int64_t OW);
bool igemm_dma_on();         // DPE_IGEMM_DMA
bool pw_stream_on();         // DPE_PW_STREAM / set_pw_stream
bool hgemm_conv_on();        // DPE_HGEMM_CONV / set_hgemm_conv
bool hgemm_conv_wgrad_on();  // DPE_HGEMM_CONV_WGRAD

void register_conv(pybind11::module& m);  // conv.cpp
void register_bn(pybind11::module& m);    // bn.cpp
void register_ops(pybind11::module& m);   // ops.cpp
void register_decode(pybind11::module& m);  // decode.cpp
}  // namespace dpe_ops
