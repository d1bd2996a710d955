// Fused multi-tensor optimizers: ONE launch updates every parameter of a
// model (replacing the reference's foreach-Adam chain of _foreach_lerp_ /
// mul / addcmul / sqrt / div / add / addcdiv launches).
//
// Each parameter is split into CHUNK-element pieces; the launch grid is the
// list of (tensor, chunk) pairs, prepared once on the host and kept on the
// device.  Per element the kernel reads p, g, state(s) and writes p,
// state(s) and (optionally) the bf16 compute shadow of p that the MFMA
// kernels consume -- so no separate fp32->bf16 cast pass per step.
//
// Hyper-parameters (lr etc.) live in a small device array so a captured
// hipGraph can replay the step while the host edits the learning rate.
#include "common.h"

namespace dpe {

struct TensorDesc {
  float* p;
  const float* g;
  float* s1;        // exp_avg (Adam) / momentum_buffer (SGD)
  float* s2;        // exp_avg_sq (Adam)
  uint16_t* shadow;  // bf16 copy of p (may be null)
  int64_t n;
  int group;
  int step_idx;  // index into steps[] (per-parameter step counters)
};

// Per group, 12 floats: lr, beta1/momentum, beta2/dampening, eps, weight_decay,
// flags(bitfield: 1 nesterov, 2 maximize, 4 decoupled wd), grad_scale, clip coef, step ok, pad...
// The host initialises coef and ok to 1.0; grad_clip_coef_kernel overwrites them when clipping is on.
constexpr int HP = 12;
constexpr int HP_COEF = 7, HP_OK = 8;
// 16K elements per block: 256 lanes x 4 (one 16-B access per operand) x 16
// iterations.  Small enough that a 25M-parameter model spreads over ~1.6k
// blocks (>6 per CU, so the streaming loads of several waves overlap), large
// enough that the per-block descriptor fetch is noise.
constexpr int CHUNK = 16384;

// Per-element update rules (shared by the 16-B vector body and the scalar tail).
struct AdamRule {
  float lr, b1, b2, eps, wd, step_size, bc2_sqrt;
  bool maximize, decoupled;
  float gscale;
  DPE_DEVICE AdamRule(const float* h, float step) {
    lr = h[0]; b1 = h[1]; b2 = h[2]; eps = h[3]; wd = h[4];
    const int flags = (int)h[5];
    gscale = h[6] * h[HP_COEF];
    maximize = flags & 2; decoupled = flags & 4;
    step_size = lr / (1.f - powf(b1, step));
    bc2_sqrt = sqrtf(1.f - powf(b2, step));
  }
  DPE_DEVICE void operator()(float& p, float g, float& m, float& v) const {
    g *= gscale;
    if (maximize) g = -g;
    if (wd != 0.f) {
      if (decoupled) p *= (1.f - lr * wd);
      else g += wd * p;
    }
    m = m + (1.f - b1) * (g - m);  // lerp, as torch
    v = b2 * v + (1.f - b2) * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p -= step_size * (m / denom);
  }
};

struct SgdRule {
  float lr, mom, damp, wd, gscale;
  bool nesterov, maximize, first;
  DPE_DEVICE SgdRule(const float* h, float step) {
    lr = h[0]; mom = h[1]; damp = h[2]; wd = h[4];
    const int flags = (int)h[5];
    gscale = h[6] * h[HP_COEF];
    nesterov = flags & 1; maximize = flags & 2;
    first = step <= 1.f;
  }
  DPE_DEVICE void operator()(float& p, float g, float& b, float&) const {
    g *= gscale;
    if (maximize) g = -g;  // as torch: negate before weight decay and momentum
    if (wd != 0.f) g += wd * p;
    if (mom != 0.f) {
      b = first ? g : mom * b + (1.f - damp) * g;
      g = nesterov ? g + mom * b : b;
    }
    p -= lr * g;
  }
};

// One (tensor, chunk) per block.  When every operand of the tensor is 16-B
// aligned (8-B for the bf16 shadow) -- always the case for parameters and for
// bucket-view gradients of 4-multiple sizes -- each lane moves 4 elements per
// operand per iteration with dwordx4 loads/stores; otherwise (or for the
// ragged tail) one element.  `s2` is only touched by rules that use it.
template <class Rule, bool TWO_STATES>
DPE_DEVICE void optim_chunk(const TensorDesc& d, const Rule& rule, int chunk) {
  const int64_t beg = (int64_t)chunk * CHUNK;
  const int64_t end = min(d.n, beg + CHUNK);
  const bool has_s1 = d.s1 != nullptr;
  const uintptr_t align = (uintptr_t)d.p | (uintptr_t)d.g | (uintptr_t)d.s1 | (TWO_STATES ? (uintptr_t)d.s2 : 0);
  const bool vec = (align & 15) == 0 && ((uintptr_t)d.shadow & 7) == 0;
  int64_t i = beg;
  if (vec) {
    // Software-pipelined one 1024-element step ahead: the next step's loads are issued before this step's
    // stores, so the wait for them counts past those stores (loads and stores share vmcnt: loaded after the
    // stores, every step waited for its predecessor's stores to complete).  Every load and store goes through
    // a buffer resource and is issued unconditionally -- an absent state or shadow is a 0-byte resource
    // (loads read 0, stores are dropped) and the last step's look-ahead re-reads its own elements -- so the
    // compiler's waits stay counted instead of vmcnt(0) (common.h buf_rsrc).
    const int64_t vend = beg + ((end - beg) & ~(int64_t)1023);
    const int nsteps = (int)((vend - beg) >> 10);
    const uint32_t bytes = (uint32_t)((vend - beg) * 4);  // <= 64 KiB (CHUNK)
    const __amdgpu_buffer_rsrc_t prs = buf_rsrc(d.p + beg, bytes), grs = buf_rsrc(d.g + beg, bytes);
    const __amdgpu_buffer_rsrc_t mrs = buf_rsrc(has_s1 ? d.s1 + beg : nullptr, has_s1 ? bytes : 0u);
    const __amdgpu_buffer_rsrc_t vrs = buf_rsrc(TWO_STATES ? d.s2 + beg : nullptr, TWO_STATES ? bytes : 0u);
    const __amdgpu_buffer_rsrc_t srs = buf_rsrc(d.shadow ? d.shadow + beg : nullptr, d.shadow ? bytes / 2 : 0u);
    auto ld = [](__amdgpu_buffer_rsrc_t r, uint32_t o) {
      return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o, 0, 0));
    };
    const uint32_t lo = threadIdx.x * 16u;  // the lane's 16 B of a 4-KiB step
    f32x4 pn = ld(prs, lo), gn = ld(grs, lo), mn = ld(mrs, lo), vn = ld(vrs, lo);
    for (int k = 0; k < nsteps; ++k) {
      f32x4 p = pn, m = mn, v = vn;
      const f32x4 g = gn;
      const uint32_t o = lo + (uint32_t)k * 4096u, on = k + 1 < nsteps ? o + 4096u : o;
      pn = ld(prs, on);
      gn = ld(grs, on);
      mn = ld(mrs, on);
      vn = ld(vrs, on);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        rule(pe, g[e], me, ve);
        p[e] = pe; m[e] = me; v[e] = ve;
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, p), prs, o, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, m), mrs, o, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), vrs, o, 0, 0);
      u32x2 sh;
      sh[0] = pack_bf2(p[0], p[1]);
      sh[1] = pack_bf2(p[2], p[3]);
      __builtin_amdgcn_raw_buffer_store_b64(sh, srs, o >> 1, 0, 0);
    }
    i = vend;
  }
  for (int64_t j = i + threadIdx.x; j < end; j += 256) {
    float p = d.p[j], m = has_s1 ? d.s1[j] : 0.f, v = TWO_STATES ? d.s2[j] : 0.f;
    rule(p, d.g[j], m, v);
    d.p[j] = p;
    if (has_s1) d.s1[j] = m;
    if (TWO_STATES) d.s2[j] = v;
    if (d.shadow) d.shadow[j] = f2bf(p);
  }
}

__global__ __launch_bounds__(256) void adam_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                   const float* __restrict__ hp, const float* __restrict__ steps) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const float* h = hp + d.group * HP;
  if (h[HP_OK] == 0.f) return;  // skipped step (non-finite gradient norm): uniform over the grid
  optim_chunk<AdamRule, true>(d, AdamRule(h, steps[d.step_idx]), ck.y);
}

__global__ __launch_bounds__(256) void sgd_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                  const float* __restrict__ hp, const float* __restrict__ steps) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const float* h = hp + d.group * HP;
  if (h[HP_OK] == 0.f) return;  // skipped step (non-finite gradient norm): uniform over the grid
  optim_chunk<SgdRule, false>(d, SgdRule(h, steps[d.step_idx]), ck.y);
}

// ------------------------------------------------------- global-norm gradient clipping
// The norm is produced on the device and consumed by the update kernels through the hp rows (HP_COEF,
// HP_OK), so a clipped step reads the gradients once more, writes nothing back and never touches the
// host.  No atomics anywhere: every sum has a fixed order, so the norm (and with it the coef every DDP
// rank derives from the same averaged buckets) is bitwise reproducible.
//
// Clip block `out`: [0] total_norm, [1] coef, [2] ok (1 finite / 0 not), [3] skipped steps.
constexpr int CLIP_STEPS = CHUNK / 1024;

// The lane's part of one chunk's 16-B steps, all issued back to back: the resource covers the chunk's
// whole 16-B groups only, so every load is entirely inside or entirely outside it (outside reads 0).
DPE_DEVICE void chunk_loads(__amdgpu_buffer_rsrc_t rs, f32x4* v) {
  const uint32_t lo = threadIdx.x * 16u;
#pragma unroll
  for (int k = 0; k < CLIP_STEPS; ++k)
    v[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, lo + (uint32_t)k * 4096u, 0, 0));
}

// Byte offset of the lane's element of the chunk's ragged end (the < 4 elements past the last whole
// 16-B group), read through a resource of the chunk's real byte count; other lanes read past it.
DPE_DEVICE uint32_t tail_offset(int n4) { return threadIdx.x < 4 ? (uint32_t)(n4 + (int)threadIdx.x) * 4u : BUF_OOB; }

// partials[b] = sum of squares of the gradient elements of table entry b (same grid as the update).
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                          float* __restrict__ partials) {
  __shared__ float sh[4];
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const int64_t beg = (int64_t)ck.y * CHUNK;
  const int n = (int)max((int64_t)0, min((int64_t)CHUNK, d.n - beg));
  const float* g = d.g + beg;
  float s;
  if (((uintptr_t)d.g & 15) == 0) {  // beg is a multiple of 16 B
    const int n4 = n & ~3;
    f32x4 v[CLIP_STEPS];
    chunk_loads(buf_rsrc(g, (uint32_t)n4 * 4u), v);
    const float t = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(buf_rsrc(g, (uint32_t)n * 4u), tail_offset(n4), 0, 0));
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;  // 8 independent accumulators of <= 8 squares each
#pragma unroll
    for (int k = 0; k < CLIP_STEPS; k += 2) {
      a0 += v[k] * v[k];
      a1 += v[k + 1] * v[k + 1];
    }
    a0 += a1;
    s = ((a0[0] + a0[1]) + (a0[2] + a0[3])) + t * t;
  } else {
    float a0 = 0.f, a1 = 0.f;
    int j = threadIdx.x;
    for (; j + 256 < n; j += 512) {
      const float x = g[j], y = g[j + 256];
      a0 += x * x;
      a1 += y * y;
    }
    if (j < n) a0 += g[j] * g[j];
    s = a0 + a1;
  }
  s = warp_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// One block: fixed-order fp64 sum of the partials -> total_norm, coef = min(1, max_norm / (norm + 1e-6))
// (torch.nn.utils.clip_grad_norm_'s formula; NaN stays NaN), ok.  With `hp` the coef goes into every
// group's row; the ok slot gets the real flag only in skip mode, else 1.0 (non-finite values propagate
// through the update as they do through torch's).
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const float* __restrict__ partials, int n, float* __restrict__ out,
                                                             const float* __restrict__ max_norm, float* __restrict__ hp,
                                                             int ngroups, int skip) {
  __shared__ double sh[256];
  __shared__ float res[2];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += (double)partials[i];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float tn = (float)sqrt(sh[0]);
    const float c = max_norm[0] / (tn + 1e-6f);
    const float coef = c > 1.f ? 1.f : c;
    const float ok = fabsf(tn) < INFINITY ? 1.f : 0.f;
    out[0] = tn;
    out[1] = coef;
    out[2] = ok;
    if (skip) out[3] += 1.f - ok;
    res[0] = coef;
    res[1] = skip ? ok : 1.f;
  }
  __syncthreads();
  if (hp != nullptr)
    for (int gi = threadIdx.x; gi < ngroups; gi += 256) {
      hp[gi * HP + HP_COEF] = res[0];
      hp[gi * HP + HP_OK] = res[1];
    }
}

// In-place g *= out[1] over the table (optim.clip_grad_norm_, for loops that keep torch's call).
__global__ __launch_bounds__(256) void grad_scale_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                         const float* __restrict__ out) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const float coef = out[1];
  const int64_t beg = (int64_t)ck.y * CHUNK;
  const int n = (int)max((int64_t)0, min((int64_t)CHUNK, d.n - beg));
  float* g = const_cast<float*>(d.g) + beg;
  if (((uintptr_t)d.g & 15) == 0) {
    const int n4 = n & ~3;
    const __amdgpu_buffer_rsrc_t rs = buf_rsrc(g, (uint32_t)n4 * 4u), trs = buf_rsrc(g, (uint32_t)n * 4u);
    f32x4 v[CLIP_STEPS];
    chunk_loads(rs, v);
    const uint32_t to = tail_offset(n4), lo = threadIdx.x * 16u;
    const float t = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(trs, to, 0, 0));
#pragma unroll
    for (int k = 0; k < CLIP_STEPS; ++k)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v[k] * coef), rs, lo + (uint32_t)k * 4096u, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(t * coef), trs, to, 0, 0);
  } else {
    for (int j = threadIdx.x; j < n; j += 256) g[j] *= coef;
  }
}

}  // namespace dpe

using namespace dpe;

extern "C" int dpe_optim_chunk_size() { return CHUNK; }
extern "C" int dpe_optim_desc_bytes() { return (int)sizeof(TensorDesc); }

// kind: 0 adam/adamw, 1 sgd
extern "C" int dpe_optim_step(int kind, const void* desc, const void* chunks, int nchunks, const float* hp, const float* steps,
                              hipStream_t st) {
  if (nchunks <= 0) return 0;
  if (kind == 0)
    hipLaunchKernelGGL(adam_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks, hp, steps);
  else
    hipLaunchKernelGGL(sgd_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks, hp, steps);
  return 0;
}

// Global gradient norm over the table: partials[nchunks] -> out (see the clip block above).  `hp` may be
// null (free-function use: no optimizer rows to fill).
extern "C" int dpe_optim_grad_norm(const void* desc, const void* chunks, int nchunks, float* partials, float* out,
                                   const float* max_norm, float* hp, int ngroups, int skip, hipStream_t st) {
  if (nchunks > 0)
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks,
                       partials);
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, st, (const float*)partials, nchunks > 0 ? nchunks : 0, out,
                     max_norm, hp, ngroups, skip);
  return 0;
}

extern "C" int dpe_optim_grad_scale(const void* desc, const void* chunks, int nchunks, const float* out, hipStream_t st) {
  if (nchunks <= 0) return 0;
  hipLaunchKernelGGL(grad_scale_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks, out);
  return 0;
}
