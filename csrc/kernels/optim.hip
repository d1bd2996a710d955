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
#include "launch.h"

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
// flags(bitfield: 1 nesterov, 2 maximize, 4 decoupled wd), grad_scale, clip coef, step ok,
// trust_coefficient (LARS) / trust ratio on-off (LAMB), trust_eps, pad.
// The host initialises coef and ok to 1.0; grad_clip_coef_kernel overwrites them when clipping is on.
constexpr int HP = 12;
constexpr int HP_COEF = 7, HP_OK = 8;
constexpr int HP_EMA = 11;  // 1 - d_n of the weight EMA (ema_decay_kernel; the EMA kernels alone read it)
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

// The weight-EMA operand of a 16-B walk (optim_chunk, lamb_chunk): its own resource, the look-ahead register and
// ema += ew * (p_new - ema), ew = 1 - d_n.  With ew == 1 (the first update, ema == 0) that is 0 + 1 * (p - 0): p
// bit for bit.  The EMA = false arm is empty, so the kernels without the average are what they were before it.
template <bool EMA>
struct EmaArm {
  DPE_DEVICE EmaArm(const float*, uint32_t, float) {}
  DPE_DEVICE void load(uint32_t) {}
  DPE_DEVICE void take() {}
  DPE_DEVICE void update(int, float) {}
  DPE_DEVICE void store(uint32_t) const {}
};

template <>
struct EmaArm<true> {
  __amdgpu_buffer_rsrc_t rs;
  float ew;
  f32x4 next, cur;
  DPE_DEVICE EmaArm(const float* base, uint32_t bytes, float ew_) : rs(buf_rsrc(base, bytes)), ew(ew_) {}
  DPE_DEVICE void load(uint32_t o) { next = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0)); }
  DPE_DEVICE void take() { cur = next; }
  DPE_DEVICE void update(int e, float p) { cur[e] = cur[e] + ew * (p - cur[e]); }
  DPE_DEVICE void store(uint32_t o) const { __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, cur), rs, o, 0, 0); }
};

// The same for lamb_chunk's one-element-per-lane end.
template <bool EMA>
struct EmaTail {
  DPE_DEVICE EmaTail(const float*, uint32_t, float) {}
  DPE_DEVICE void load(uint32_t) {}
  DPE_DEVICE void store(uint32_t, float) const {}
};

template <>
struct EmaTail<true> {
  __amdgpu_buffer_rsrc_t rs;
  float ew, a;
  DPE_DEVICE EmaTail(const float* base, uint32_t bytes, float ew_) : rs(buf_rsrc(base, bytes)), ew(ew_), a(0.f) {}
  DPE_DEVICE void load(uint32_t o) { a = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0)); }
  DPE_DEVICE void store(uint32_t o, float p) const {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(a + ew * (p - a)), rs, o, 0, 0);
  }
};

// One (tensor, chunk) per block.  When every operand of the tensor is 16-B
// aligned (8-B for the bf16 shadow) -- always the case for parameters and for
// bucket-view gradients of 4-multiple sizes -- each lane moves 4 elements per
// operand per iteration with dwordx4 loads/stores; otherwise (or for the
// ragged tail) one element.  `s2` is only touched by rules that use it.
//
// EMA: the weight average rides along, ema += ew * (p_new - ema) with ew = 1 - d_n (ew == 1 on the first
// update: 0 + 1 * (p - 0) is p bit for bit).  One more operand of the same walk -- its load joins the
// look-ahead loads and its store the stores, both unconditional through a resource of its own.  `ema` is
// the tensor's fp32 average (never null when EMA); the EMA = false instantiations do not see either argument.
template <class Rule, bool TWO_STATES, bool EMA = false>
DPE_DEVICE void optim_chunk(const TensorDesc& d, const Rule& rule, int chunk, float* ema = nullptr, float ew = 0.f) {
  const int64_t beg = (int64_t)chunk * CHUNK;
  const int64_t end = min(d.n, beg + CHUNK);
  const bool has_s1 = d.s1 != nullptr;
  const uintptr_t align = (uintptr_t)d.p | (uintptr_t)d.g | (uintptr_t)d.s1 | (TWO_STATES ? (uintptr_t)d.s2 : 0) |
                          (EMA ? (uintptr_t)ema : 0);
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
    EmaArm<EMA> arm(ema + beg, bytes, ew);
    arm.load(lo);
    for (int k = 0; k < nsteps; ++k) {
      f32x4 p = pn, m = mn, v = vn;
      const f32x4 g = gn;
      arm.take();
      const uint32_t o = lo + (uint32_t)k * 4096u, on = k + 1 < nsteps ? o + 4096u : o;
      pn = ld(prs, on);
      gn = ld(grs, on);
      mn = ld(mrs, on);
      vn = ld(vrs, on);
      arm.load(on);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        rule(pe, g[e], me, ve);
        p[e] = pe; m[e] = me; v[e] = ve;
        arm.update(e, pe);
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, p), prs, o, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, m), mrs, o, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), vrs, o, 0, 0);
      arm.store(o);
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
    if (EMA) {
      const float a = ema[j];
      ema[j] = a + ew * (p - a);
    }
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

// The same updates with the weight EMA arm.  `ema[ti]` is tensor ti's average: a device array of its own, so
// TensorDesc and the kernels above are what they were without it.
__global__ __launch_bounds__(256) void adam_ema_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                       const float* __restrict__ hp, const float* __restrict__ steps,
                                                       float* const* __restrict__ ema) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const float* h = hp + d.group * HP;
  if (h[HP_OK] == 0.f) return;  // skipped step: the average stays too
  optim_chunk<AdamRule, true, true>(d, AdamRule(h, steps[d.step_idx]), ck.y, ema[ck.x], h[HP_EMA]);
}

__global__ __launch_bounds__(256) void sgd_ema_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                      const float* __restrict__ hp, const float* __restrict__ steps,
                                                      float* const* __restrict__ ema) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const float* h = hp + d.group * HP;
  if (h[HP_OK] == 0.f) return;
  optim_chunk<SgdRule, false, true>(d, SgdRule(h, steps[d.step_idx]), ck.y, ema[ck.x], h[HP_EMA]);
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

// The lane's share of the sum of squares of x[0, n) (n <= CHUNK; `al16`: x is 16-B aligned).  Shared by every
// kernel that takes a chunk's norm, so they all sum in the same order.
DPE_DEVICE float lane_sqsum(const float* x, bool al16, int n) {
  float s;
  if (al16) {
    const int n4 = n & ~3;
    f32x4 v[CLIP_STEPS];
    chunk_loads(buf_rsrc(x, (uint32_t)n4 * 4u), v);
    const float t = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(buf_rsrc(x, (uint32_t)n * 4u), tail_offset(n4), 0, 0));
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
      const float x0 = x[j], x1 = x[j + 256];
      a0 += x0 * x0;
      a1 += x1 * x1;
    }
    if (j < n) a0 += x[j] * x[j];
    s = a0 + a1;
  }
  return s;
}

// partials[b] = sum of squares of the gradient elements of table entry b (same grid as the update).
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                          float* __restrict__ partials) {
  __shared__ float sh[4];
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const int64_t beg = (int64_t)ck.y * CHUNK;
  const int n = (int)max((int64_t)0, min((int64_t)CHUNK, d.n - beg));
  float s = lane_sqsum(d.g + beg, ((uintptr_t)d.g & 15) == 0, n);  // beg is a multiple of 16 B
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

// ------------------------------------------------------- learning-rate schedule
// The lr of every group for this step, computed on the device from a device step counter and written into
// the hp rows the update kernels read -- like the clip coefficient, so the host copies nothing per step and
// a captured step replays with an advancing lr.  Schedule block `sched` (fp64):
//   [0] s, the scheduled steps already taken   [1] kind (0 constant, 1 linear, 2 cosine, 3 poly)
//   [2] W warm-up steps   [3] T total steps   [4] r = min_ratio   [5] power   [6 + g] base lr of group g
//   f(s) = (s + 1) / W                                             s < W
//        = 1 | 1 - (1 - r) t | r + (1 - r) (1 + cos(pi t)) / 2 | r + (1 - r) (1 - t)^power,
//          t = min(1, (s - W) / max(1, T - W))                      otherwise
// A thread per group evaluates f in fp64 and rounds base * f once; cur[g] keeps the lr the step uses.  The
// counter then advances by this step's ok flag (final by now: the clip kernel runs first), so a step skipped
// for a non-finite gradient norm consumes no schedule step.
constexpr int SCHED_HDR = 6;

__global__ __launch_bounds__(64) void lr_schedule_kernel(float* __restrict__ hp, int ngroups, double* __restrict__ sched,
                                                         float* __restrict__ cur) {
  const double s = sched[0], W = sched[2], T = sched[3], r = sched[4], pw = sched[5];
  const int kind = (int)sched[1];
  const float ok = hp[HP_OK];  // the same in every row
  double f;
  if (s < W) {
    f = (s + 1.0) / W;
  } else {
    const double t = fmin(1.0, (s - W) / fmax(1.0, T - W));
    if (kind == 1) f = 1.0 - (1.0 - r) * t;
    else if (kind == 2) f = r + (1.0 - r) * (0.5 * (1.0 + cos(3.14159265358979323846 * t)));
    else if (kind == 3) f = r + (1.0 - r) * pow(1.0 - t, pw);
    else f = 1.0;
  }
  for (int g = threadIdx.x; g < ngroups; g += 64) {
    const float lr = (float)(sched[SCHED_HDR + g] * f);
    hp[g * HP] = lr;
    cur[g] = lr;
  }
  __syncthreads();  // every thread has read s
  if (threadIdx.x == 0) sched[0] = s + (double)ok;
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

// ------------------------------------------------------- layer-wise trust ratios (LARS / LAMB)
// Every tensor's update is scaled by a ratio of two per-tensor 2-norms.  The norms reuse the clip machinery:
// one partial per (tensor, chunk) block, no atomics, then a fixed-order fp64 sum -- here per tensor, over
// the tensor's contiguous run of table entries [first_chunk[ti], first_chunk[ti + 1]).
//   LARS: partials of (w, g)      -> ratio -> SGD update of ratio * (g' + wd * w)
//   LAMB: phase 1 writes m, v and the partials of (w, u) -> ratio -> phase 2 recomputes u and writes w
// hp slots: 9 trust_coefficient (LARS) / trust ratio on-off (LAMB), 10 trust_eps.
// stats[ti] = (wn, gn or un, ratio), fp32.
constexpr int HP_TRUST = 9, HP_TEPS = 10;

// a * b that the compiler may not contract into a neighbouring add
DPE_DEVICE float mul_nofuse(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// Thread 0 writes the block's two sums (fixed order: lane, wave butterfly, 4 waves).
DPE_DEVICE void block_write2(float a, float b, float* __restrict__ pa, float* __restrict__ pb) {
  __shared__ float sh[8];
  a = warp_sum(a);
  b = warp_sum(b);
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6] = a;
    sh[4 + (threadIdx.x >> 6)] = b;
  }
  lds_barrier();  // LDS only: __syncthreads() would also wait for the block's last m / v stores
  if (threadIdx.x == 0) {
    pa[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    pb[blockIdx.x] = (sh[4] + sh[5]) + (sh[6] + sh[7]);
  }
}

// part_w[b] = sum p^2, part_g[b] = sum g^2 (the latter exactly grad_sqnorm_kernel's value: with clipping on,
// grad_clip_coef_kernel runs on part_g and the gradients are read once for both norms).
__global__ __launch_bounds__(256) void lars_sqnorm_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                          float* __restrict__ part_w, float* __restrict__ part_g) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const int64_t beg = (int64_t)ck.y * CHUNK;
  const int n = (int)max((int64_t)0, min((int64_t)CHUNK, d.n - beg));
  const float sw = lane_sqsum(d.p + beg, ((uintptr_t)d.p & 15) == 0, n);
  const float sg = lane_sqsum(d.g + beg, ((uintptr_t)d.g & 15) == 0, n);
  block_write2(sw, sg, part_w, part_g);
}

// SGD on d = ratio * (g' + wd * w), weight decay 0 afterwards.  Written as SgdRule plus one multiply that
// stays a multiply, so ratio == 1 (trust_coefficient 0) is bit for bit sgd_kernel's update.
struct LarsRule {
  SgdRule r;
  float ratio;
  DPE_DEVICE LarsRule(const float* h, float step, float ratio_) : r(h, step), ratio(ratio_) {}
  DPE_DEVICE void operator()(float& p, float g, float& b, float&) const {
    g *= r.gscale;
    if (r.maximize) g = -g;
    if (r.wd != 0.f) g += r.wd * p;
    g = mul_nofuse(ratio, g);
    if (r.mom != 0.f) {
      b = r.first ? g : r.mom * b + (1.f - r.damp) * g;
      g = r.nesterov ? g + r.mom * b : b;
    }
    p -= r.lr * g;
  }
};

__global__ __launch_bounds__(256) void lars_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                   const float* __restrict__ hp, const float* __restrict__ steps,
                                                   const float* __restrict__ stats) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const float* h = hp + d.group * HP;
  if (h[HP_OK] == 0.f) return;  // skipped step: uniform over the grid
  optim_chunk<LarsRule, false>(d, LarsRule(h, steps[d.step_idx], stats[ck.x * 3 + 2]), ck.y);
}

__global__ __launch_bounds__(256) void lars_ema_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                       const float* __restrict__ hp, const float* __restrict__ steps,
                                                       const float* __restrict__ stats, float* const* __restrict__ ema) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const float* h = hp + d.group * HP;
  if (h[HP_OK] == 0.f) return;
  optim_chunk<LarsRule, false, true>(d, LarsRule(h, steps[d.step_idx], stats[ck.x * 3 + 2]), ck.y, ema[ck.x], h[HP_EMA]);
}

struct LambRule {
  float lr, b1, b2, eps, wd, gscale, rbc1, rbc2;
  bool maximize;
  DPE_DEVICE LambRule(const float* h, float step) {
    lr = h[0]; b1 = h[1]; b2 = h[2]; eps = h[3]; wd = h[4];
    maximize = (int)h[5] & 2;
    gscale = h[6] * h[HP_COEF];
    // 1 - b^t to a few ulp of the result: 1 - powf(b2, t) carries powf's absolute error (~6e-8 near 1)
    // into a value of ~1e-3 * t, a relative 6e-5 / t that the update norm |u| would inherit whole.
    rbc1 = -1.f / expm1f(step * log1pf(b1 - 1.f));
    rbc2 = -1.f / expm1f(step * log1pf(b2 - 1.f));
  }
  DPE_DEVICE void moments(float g, float& m, float& v) const {
    g *= gscale;
    if (maximize) g = -g;
    m = m + (1.f - b1) * (g - m);  // lerp, as torch
    v = b2 * v + (1.f - b2) * g * g;
  }
  // The Adam update with the (coupled) weight decay inside.  Both phases call this on the same p, m, v;
  // nothing in it is contracted with the caller's arithmetic, so both get the same bits.  It runs twice per
  // element, so the bias corrections are multiplies by per-block reciprocals and the root and the quotient are
  // the 1-ulp v_sqrt_f32 / v_rcp_f32: with IEEE divides and root the two phases spent ~70 VALU instructions per
  // element, 40 % of the machine's issue rate at the streaming rate; a few 6e-8 roundings against the 1e-5
  // the optimizers are held to.
  DPE_DEVICE float update(float p, float m, float v) const {
#pragma clang fp contract(off)
    return (m * rbc1) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v * rbc2) + eps) + wd * p;
  }
};

// One (tensor, chunk) of LAMB.  PHASE 1: m, v <- g; sw += p^2, su += u^2 (the lane's share).  PHASE 2:
// p -= lr_ratio * u, bf16 shadow.  The walk is optim_chunk's: 16-B steps pipelined one ahead through buffer
// resources; the ragged end (or a whole chunk of a tensor that is not 16-B aligned) goes one element per
// lane through resources clamped to the chunk, so no load or store is predicated there either.  EMA (phase 2
// only): the weight average as in optim_chunk, one more operand of both walks.
template <int PHASE, bool EMA = false>
DPE_DEVICE void lamb_chunk(const TensorDesc& d, const LambRule& rule, int chunk, float lr_ratio, float& sw, float& su,
                           float* ema = nullptr, float ew = 0.f) {
  static_assert(!EMA || PHASE == 2, "the average follows the weights phase 2 writes");
  const int64_t beg = (int64_t)chunk * CHUNK;
  const int64_t end = min(d.n, beg + CHUNK);
  const uintptr_t align = (uintptr_t)d.p | (uintptr_t)d.s1 | (uintptr_t)d.s2 | (PHASE == 1 ? (uintptr_t)d.g : 0) |
                          (EMA ? (uintptr_t)ema : 0);
  const bool vec = (align & 15) == 0 && (PHASE == 1 || ((uintptr_t)d.shadow & 7) == 0);
  const bool has_sh = PHASE == 2 && d.shadow != nullptr;
  f32x4 aw = {0.f, 0.f, 0.f, 0.f}, au = aw;
  int64_t i = beg;
  if (vec) {
    const int64_t vend = beg + ((end - beg) & ~(int64_t)1023);
    const int nsteps = (int)((vend - beg) >> 10);
    const uint32_t bytes = (uint32_t)((vend - beg) * 4);  // <= 64 KiB (CHUNK)
    const __amdgpu_buffer_rsrc_t prs = buf_rsrc(d.p + beg, bytes), mrs = buf_rsrc(d.s1 + beg, bytes);
    const __amdgpu_buffer_rsrc_t vrs = buf_rsrc(d.s2 + beg, bytes);
    const __amdgpu_buffer_rsrc_t grs = buf_rsrc(PHASE == 1 ? d.g + beg : nullptr, PHASE == 1 ? bytes : 0u);
    const __amdgpu_buffer_rsrc_t srs = buf_rsrc(has_sh ? d.shadow + beg : nullptr, has_sh ? bytes / 2 : 0u);
    auto ld = [](__amdgpu_buffer_rsrc_t r, uint32_t o) {
      return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o, 0, 0));
    };
    const uint32_t lo = threadIdx.x * 16u;
    f32x4 pn = ld(prs, lo), mn = ld(mrs, lo), vn = ld(vrs, lo), gn = pn;
    if (PHASE == 1) gn = ld(grs, lo);
    EmaArm<EMA> arm(ema + beg, bytes, ew);
    arm.load(lo);
    for (int k = 0; k < nsteps; ++k) {
      f32x4 p = pn, m = mn, v = vn;
      const f32x4 g = gn;
      arm.take();
      const uint32_t o = lo + (uint32_t)k * 4096u, on = k + 1 < nsteps ? o + 4096u : o;
      pn = ld(prs, on);
      if (PHASE == 1) gn = ld(grs, on);
      mn = ld(mrs, on);
      vn = ld(vrs, on);
      arm.load(on);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float me = m[e], ve = v[e];
        if (PHASE == 1) rule.moments(g[e], me, ve);
        const float u = rule.update(p[e], me, ve);
        if (PHASE == 1) {
          m[e] = me; v[e] = ve;
          aw[e] += p[e] * p[e];
          au[e] += u * u;
        } else {
          p[e] -= lr_ratio * u;
          arm.update(e, p[e]);
        }
      }
      if (PHASE == 1) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, m), mrs, o, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), vrs, o, 0, 0);
      } else {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, p), prs, o, 0, 0);
        u32x2 sh;
        sh[0] = pack_bf2(p[0], p[1]);
        sh[1] = pack_bf2(p[2], p[3]);
        __builtin_amdgcn_raw_buffer_store_b64(sh, srs, o >> 1, 0, 0);
        arm.store(o);
      }
    }
    i = vend;
  }
  const uint32_t tb = (uint32_t)((end - i) * 4);  // <= 64 KiB
  const int nt = (int)((end - i + 255) >> 8);
  const __amdgpu_buffer_rsrc_t prs = buf_rsrc(d.p + i, tb), mrs = buf_rsrc(d.s1 + i, tb), vrs = buf_rsrc(d.s2 + i, tb);
  const __amdgpu_buffer_rsrc_t grs = buf_rsrc(PHASE == 1 ? d.g + i : nullptr, PHASE == 1 ? tb : 0u);
  const __amdgpu_buffer_rsrc_t srs = buf_rsrc(has_sh ? d.shadow + i : nullptr, has_sh ? tb / 2 : 0u);
  EmaTail<EMA> tail(ema + i, tb, ew);
  auto ld1 = [](__amdgpu_buffer_rsrc_t r, uint32_t o) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, o, 0, 0));
  };
  float tw = 0.f, tu = 0.f;
  for (int k = 0; k < nt; ++k) {
    const uint32_t o = ((uint32_t)k * 256u + threadIdx.x) * 4u;  // past tb: reads 0, the stores are dropped
    float p = ld1(prs, o), m = ld1(mrs, o), v = ld1(vrs, o);
    tail.load(o);
    if (PHASE == 1) {
      rule.moments(ld1(grs, o), m, v);
      const float u = rule.update(p, m, v);
      tw += p * p;
      tu += o < tb ? u * u : 0.f;  // (0 / (0 + eps) is NaN at eps == 0)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m), mrs, o, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), vrs, o, 0, 0);
    } else {
      p -= lr_ratio * rule.update(p, m, v);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(p), prs, o, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b16(f2bf(p), srs, o >> 1, 0, 0);
      tail.store(o, p);
    }
  }
  sw = ((aw[0] + aw[1]) + (aw[2] + aw[3])) + tw;
  su = ((au[0] + au[1]) + (au[2] + au[3])) + tu;
}

__global__ __launch_bounds__(256) void lamb_phase1_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                          const float* __restrict__ hp, const float* __restrict__ steps,
                                                          float* __restrict__ part_w, float* __restrict__ part_u) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const float* h = hp + d.group * HP;
  if (h[HP_OK] == 0.f) return;  // skipped step: m and v stay as they are (uniform over the grid)
  float sw, su;
  lamb_chunk<1>(d, LambRule(h, steps[d.step_idx]), ck.y, 0.f, sw, su);
  block_write2(sw, su, part_w, part_u);
}

__global__ __launch_bounds__(256) void lamb_phase2_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                          const float* __restrict__ hp, const float* __restrict__ steps,
                                                          const float* __restrict__ stats) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const float* h = hp + d.group * HP;
  if (h[HP_OK] == 0.f) return;
  float sw, su;
  lamb_chunk<2>(d, LambRule(h, steps[d.step_idx]), ck.y, h[0] * stats[ck.x * 3 + 2], sw, su);
}

__global__ __launch_bounds__(256) void lamb_phase2_ema_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                              const float* __restrict__ hp, const float* __restrict__ steps,
                                                              const float* __restrict__ stats, float* const* __restrict__ ema) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  const float* h = hp + d.group * HP;
  if (h[HP_OK] == 0.f) return;
  float sw, su;
  lamb_chunk<2, true>(d, LambRule(h, steps[d.step_idx]), ck.y, h[0] * stats[ck.x * 3 + 2], sw, su, ema[ck.x], h[HP_EMA]);
}

// One wave per tensor: lane l sums partials first + l, first + l + 64, ... in fp64, then a butterfly.  Of
// ResNet-50's 161 tensors the largest has 144 chunks and of GPT-2-small's 148 all but the embedding (2356)
// have at most 144, most a handful: a 256-lane block would keep three waves idle behind a barrier, and the
// launch is a latency-bound grid of ~150 waves either way.
template <bool LAMB>
__global__ __launch_bounds__(64) void trust_ratio_kernel(const TensorDesc* __restrict__ td, const int* __restrict__ first_chunk,
                                                         int nchunks, const float* __restrict__ part_w,
                                                         const float* __restrict__ part_x, const float* __restrict__ hp,
                                                         float* __restrict__ stats) {
  const int ti = blockIdx.x;
  const float* h = hp + td[ti].group * HP;
  if (h[HP_OK] == 0.f) return;  // skipped step: the stats of the last real step stay
  const int c0 = max(first_chunk[ti], 0), c1 = min(first_chunk[ti + 1], nchunks);
  double a = 0.0, b = 0.0;
  for (int c = c0 + (int)threadIdx.x; c < c1; c += 64) {
    a += (double)part_w[c];
    b += (double)part_x[c];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  if (threadIdx.x == 0) {
    const float wn = (float)sqrt(a);
    float xn = (float)sqrt(b), ratio = 1.f;
    if (LAMB) {
      if (h[HP_TRUST] != 0.f && wn > 0.f && xn > 0.f) ratio = wn / xn;
    } else {
      xn *= h[6] * h[HP_COEF];  // the norm of the clipped gradient
      const float tc = h[HP_TRUST];
      if (tc > 0.f && wn > 0.f && xn > 0.f) ratio = tc * wn / (xn + h[4] * wn + h[HP_TEPS]);
    }
    stats[ti * 3 + 0] = wn;
    stats[ti * 3 + 1] = xn;
    stats[ti * 3 + 2] = ratio;
  }
}

// ------------------------------------------------------- weight EMA: this step's decay, and the swap
// EMA block `blk` (fp64): [0] n, the updates already done   [1] decay   [2] warm-up on / off.
//   d_0 = 0 (the first update copies),  d_n = warm-up ? min(decay, (1 + n) / (10 + n)) : decay
// 1 - d_n, evaluated in fp64 and rounded once, goes into every group's hp row (HP_EMA) and d_n into cur[0]; the
// counter then advances by the step's ok flag (final by now, as for lr_schedule_kernel), so a skipped step
// makes no update and consumes no warm-up step.
__global__ __launch_bounds__(64) void ema_decay_kernel(float* __restrict__ hp, int ngroups, double* __restrict__ blk,
                                                       float* __restrict__ cur) {
  const double n = blk[0], decay = blk[1];
  const float ok = hp[HP_OK];  // the same in every row
  double dn = 0.0;
  if (n >= 1.0) dn = blk[2] != 0.0 ? fmin(decay, (1.0 + n) / (10.0 + n)) : decay;
  const float ew = (float)(1.0 - dn);
  for (int g = threadIdx.x; g < ngroups; g += 64) hp[g * HP + HP_EMA] = ew;
  __syncthreads();  // every thread has read n
  if (threadIdx.x == 0) {
    cur[0] = (float)dn;
    blk[0] = n + (double)ok;
  }
}

// w <-> ema element for element over the table, and the bf16 shadow of the new w (optimizer.swap_ema()).
// Not on the training path: plain 16-B accesses where the three pointers allow, else one element per lane.
__global__ __launch_bounds__(256) void ema_swap_kernel(const TensorDesc* __restrict__ td, const int2* __restrict__ chunks,
                                                       float* const* __restrict__ ema) {
  const int2 ck = chunks[blockIdx.x];
  const TensorDesc d = td[ck.x];
  float* a = ema[ck.x];
  const int64_t beg = (int64_t)ck.y * CHUNK;
  const int64_t end = min(d.n, beg + CHUNK);
  int64_t i = beg;
  if ((((uintptr_t)d.p | (uintptr_t)a) & 15) == 0 && ((uintptr_t)d.shadow & 7) == 0) {  // beg is a multiple of 16 B
    const int64_t vend = beg + ((end - beg) & ~(int64_t)3);
    for (int64_t j = beg + (int64_t)threadIdx.x * 4; j < vend; j += 1024) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(d.p + j), e = *reinterpret_cast<const f32x4*>(a + j);
      *reinterpret_cast<f32x4*>(d.p + j) = e;
      *reinterpret_cast<f32x4*>(a + j) = w;
      if (d.shadow) {
        u32x2 sh;
        sh[0] = pack_bf2(e[0], e[1]);
        sh[1] = pack_bf2(e[2], e[3]);
        *reinterpret_cast<u32x2*>(d.shadow + j) = sh;
      }
    }
    i = vend;
  }
  for (int64_t j = i + threadIdx.x; j < end; j += 256) {
    const float w = d.p[j], e = a[j];
    d.p[j] = e;
    a[j] = w;
    if (d.shadow) d.shadow[j] = f2bf(e);
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

// The same step with the weight EMA: ema = device array of one fp32 pointer per tensor of the table.
extern "C" int dpe_optim_step_ema(int kind, const void* desc, const void* chunks, int nchunks, const float* hp,
                                  const float* steps, const void* ema, hipStream_t st) {
  if (nchunks <= 0) return 0;
  if (kind == 0)
    hipLaunchKernelGGL(adam_ema_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks, hp, steps,
                       (float* const*)ema);
  else
    hipLaunchKernelGGL(sgd_ema_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks, hp, steps,
                       (float* const*)ema);
  return 0;
}

// 1 - d_n into hp[g * HP + 11] and d_n into cur[0], then the counter in blk[0] advances by hp[HP_OK].
// blk holds 3 doubles (see ema_decay_kernel).
extern "C" int dpe_optim_ema_decay(float* hp, int ngroups, double* blk, float* cur, hipStream_t st) {
  if (ngroups <= 0) return 0;
  hipLaunchKernelGGL(ema_decay_kernel, dim3(1), dim3(64), 0, st, hp, ngroups, blk, cur);
  return 0;
}

extern "C" int dpe_optim_ema_swap(const void* desc, const void* chunks, int nchunks, const void* ema, hipStream_t st) {
  if (nchunks <= 0) return 0;
  hipLaunchKernelGGL(ema_swap_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks,
                     (float* const*)ema);
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

// The one-block finishing kernel alone, on partials something else produced (LARS: its own partials kernel).
extern "C" int dpe_optim_clip_coef(const float* partials, int nchunks, float* out, const float* max_norm, float* hp,
                                   int ngroups, int skip, hipStream_t st) {
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, st, partials, nchunks > 0 ? nchunks : 0, out, max_norm, hp,
                     ngroups, skip);
  return 0;
}

// This step's lr into hp[g * HP + 0] and cur[g], then the counter in sched[0] advances by hp[HP_OK].
// sched holds SCHED_HDR + ngroups doubles (see lr_schedule_kernel).
extern "C" int dpe_optim_sched_header() { return SCHED_HDR; }
extern "C" int dpe_optim_lr_schedule(float* hp, int ngroups, double* sched, float* cur, hipStream_t st) {
  if (ngroups <= 0) return 0;
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(64), 0, st, hp, ngroups, sched, cur);
  return 0;
}

// Trust-ratio steps.  kind: 0 LARS, 1 LAMB.
// partials: LARS part_w = sum p^2, part_x = sum g^2; LAMB phase 1 (writes m, v; part_x = sum u^2).
extern "C" int dpe_optim_trust_partials(int kind, const void* desc, const void* chunks, int nchunks, const float* hp,
                                        const float* steps, float* part_w, float* part_x, hipStream_t st) {
  if (nchunks <= 0) return 0;
  if (kind == 0)
    hipLaunchKernelGGL(lars_sqnorm_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks,
                       part_w, part_x);
  else
    hipLaunchKernelGGL(lamb_phase1_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks, hp,
                       steps, part_w, part_x);
  return 0;
}

extern "C" int dpe_optim_trust_ratio(int kind, const void* desc, int ntensors, const int* first_chunk, int nchunks,
                                     const float* part_w, const float* part_x, const float* hp, float* stats, hipStream_t st) {
  if (ntensors <= 0) return 0;
  if (kind == 0)
    hipLaunchKernelGGL(trust_ratio_kernel<false>, dim3(ntensors), dim3(64), 0, st, (const TensorDesc*)desc, first_chunk, nchunks,
                       part_w, part_x, hp, stats);
  else
    hipLaunchKernelGGL(trust_ratio_kernel<true>, dim3(ntensors), dim3(64), 0, st, (const TensorDesc*)desc, first_chunk, nchunks,
                       part_w, part_x, hp, stats);
  return 0;
}

// The update: LARS's SGD on ratio * (g' + wd * w), or LAMB phase 2.
extern "C" int dpe_optim_trust_step(int kind, const void* desc, const void* chunks, int nchunks, const float* hp,
                                    const float* steps, const float* stats, hipStream_t st) {
  if (nchunks <= 0) return 0;
  if (kind == 0)
    hipLaunchKernelGGL(lars_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks, hp, steps,
                       stats);
  else
    hipLaunchKernelGGL(lamb_phase2_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks, hp,
                       steps, stats);
  return 0;
}

extern "C" int dpe_optim_trust_step_ema(int kind, const void* desc, const void* chunks, int nchunks, const float* hp,
                                        const float* steps, const float* stats, const void* ema, hipStream_t st) {
  if (nchunks <= 0) return 0;
  if (kind == 0)
    hipLaunchKernelGGL(lars_ema_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks, hp, steps,
                       stats, (float* const*)ema);
  else
    hipLaunchKernelGGL(lamb_phase2_ema_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks, hp,
                       steps, stats, (float* const*)ema);
  return 0;
}

extern "C" int dpe_optim_grad_scale(const void* desc, const void* chunks, int nchunks, const float* out, hipStream_t st) {
  if (nchunks <= 0) return 0;
  hipLaunchKernelGGL(grad_scale_kernel, dim3(nchunks), dim3(256), 0, st, (const TensorDesc*)desc, (const int2*)chunks, out);
  return 0;
}
