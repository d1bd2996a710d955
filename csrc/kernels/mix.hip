// Mixup / CutMix (README, "Batch mixing"): one mixing decision per batch, drawn on the device, and the mix
// itself inside the pass that packs the NCHW fp32 batch for the stem.
//
// The decision is a float32[8] row   [w_pix, w_lab, x1, y1, x2, y2, mode, lam_raw]
//   mode 0 none:   w_pix = w_lab = 1, empty box
//   mode 1 mixup:  w_pix = w_lab = lam, empty box
//   mode 2 cutmix: w_pix = 1, box [y1:y2, x1:x2] (torchvision's), w_lab = 1 - box area / (H W)
// with lam ~ Beta(alpha, alpha) of the mode's alpha.  The partner of image n is image (n - 1) mod N
// (x.roll(1, 0)).  Pixel rule: inside the box the partner's pixel, outside w_pix x + (1 - w_pix) x_partner in
// fp32, then one RNE rounding to bf16.
//
// mix_draw_kernel: row i of a launch uses the Philox-4x32-10 blocks (key = seed, counter = (stream, offset + i, k))
// -- k is the fourth counter word, which philox4x32() of common.h fixes at 0x9E3779B9: no block here is one of a
// dropout kernel's, whatever the seeds and streams.  Words of block k:
//   k = 0                 w0: apply (u < prob)   w1: cutmix (u < switch_prob)   w2: r_x = mulhi(w2, W)   w3: r_y = mulhi(w3, H)
//   k = 1 + 13 g + t      trip t < 12 of Gamma draw g (0, 1): w0, w1 Box-Muller normal, w2 the acceptance uniform
//   k = 1 + 13 g + 12     w0: the boost uniform of Gamma draw g (alpha < 1)
// u = ((w >> 8) + 0.5) 2^-24, in (0, 1).  lam = G0 / (G0 + G1), G ~ Gamma(alpha) by Marsaglia-Tsang (2000):
// d = a' - 1/3, c = 1 / sqrt(9 d), v = (1 + c n)^3, accept iff v > 0 and ln u < n^2 / 2 + d - d v + d ln v; then
// G = d v, with a' = alpha for alpha >= 1 and a' = alpha + 1, G *= u_boost^(1 / alpha) below 1.  Everything is
// carried as ln G, so a small alpha underflows nothing: lam = 1 / (1 + exp(ln G1 - ln G0)).
// The method accepts a trip with probability >= 0.95 for every a' >= 1 (0.9516 at a' = 1, rising with a'), so T
// trips all reject with probability <= 0.05^T and a row (two Gamma draws) needs 2 x 0.05^T < 1e-12: T >= 10.
// MIX_TRIPS = 12 (5e-16 per row; still below 1e-12 if the rate were only 0.906).  All 12 trips are always
// computed and the first accepted one is taken, so no loop's length depends on data; if none accepts, the draw
// falls back to v = 1, i.e. G = d.
#include "common.h"
#include "launch.h"

namespace dpe {

constexpr int MIX_TRIPS = 12;

DPE_DEVICE u32x4 mix_philox(uint64_t seed, uint64_t row, uint32_t stream, uint32_t k) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t c0 = stream, c1 = (uint32_t)row, c2 = (uint32_t)(row >> 32), c3 = k;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  u32x4 r;
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
  return r;
}

DPE_DEVICE float mix_u01(uint32_t w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-8f; }

// ln of a Gamma(alpha, 1) variate, alpha > 0
DPE_DEVICE float mix_log_gamma(uint64_t seed, uint64_t row, uint32_t stream, int g, float alpha) {
  const uint32_t kb = 1u + (uint32_t)g * (MIX_TRIPS + 1);
  const float a1 = alpha < 1.f ? alpha + 1.f : alpha;
  const float d = a1 - (1.f / 3.f);
  const float c = 1.f / sqrtf(9.f * d);
  float lg = logf(d);  // the fallback: v = 1
  bool done = false;
#pragma unroll 1
  for (int t = 0; t < MIX_TRIPS; ++t) {
    const u32x4 r = mix_philox(seed, row, stream, kb + (uint32_t)t);
    const float n = sqrtf(-2.f * logf(mix_u01(r[0]))) * cosf(6.283185307179586f * mix_u01(r[1]));
    const float t1 = 1.f + c * n;
    const float v = t1 * t1 * t1;
    const float lv = logf(fmaxf(v, 1e-37f));
    const bool ok = v > 0.f && logf(mix_u01(r[2])) < 0.5f * n * n + d - d * v + d * lv;
    if (ok && !done) {
      lg = logf(d) + lv;
      done = true;
    }
  }
  if (alpha < 1.f) lg += logf(mix_u01(mix_philox(seed, row, stream, kb + MIX_TRIPS)[0])) / alpha;
  return lg;
}

// One block; thread t takes rows t, t + blockDim.x, ...  The caller advances rng[1] by count afterwards.
__global__ __launch_bounds__(256) void mix_draw_kernel(const int64_t* __restrict__ rng, uint32_t stream, int H, int W,
                                                       float mixup_alpha, float cutmix_alpha, float prob, float switch_prob,
                                                       int count, float* __restrict__ out) {
  const uint64_t seed = (uint64_t)rng[0], offset = (uint64_t)rng[1];
  for (int i = threadIdx.x; i < count; i += blockDim.x) {
    const uint64_t row = offset + (uint64_t)i;
    const u32x4 r = mix_philox(seed, row, stream, 0u);
    int mode = 0;
    if (mixup_alpha > 0.f && cutmix_alpha > 0.f) mode = mix_u01(r[1]) < switch_prob ? 2 : 1;
    else if (mixup_alpha > 0.f) mode = 1;
    else if (cutmix_alpha > 0.f) mode = 2;
    float lam = 1.f;
    if (mode != 0) {
      const float alpha = mode == 2 ? cutmix_alpha : mixup_alpha;
      const float l0 = mix_log_gamma(seed, row, stream, 0, alpha), l1 = mix_log_gamma(seed, row, stream, 1, alpha);
      lam = 1.f / (1.f + expf(l1 - l0));
    }
    if (!(mix_u01(r[0]) < prob)) mode = 0;
    float w_pix = 1.f, w_lab = 1.f;
    int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    if (mode == 1) {
      w_pix = w_lab = lam;
    } else if (mode == 2) {
      const int rx = (int)(((uint64_t)r[2] * (uint64_t)W) >> 32), ry = (int)(((uint64_t)r[3] * (uint64_t)H) >> 32);
      const float hr = 0.5f * sqrtf(fmaxf(1.f - lam, 0.f));
      const int hw = (int)(hr * (float)W), hh = (int)(hr * (float)H);
      x1 = max(rx - hw, 0); y1 = max(ry - hh, 0);
      x2 = min(rx + hw, W); y2 = min(ry + hh, H);
      const double hwd = (double)H * (double)W;
      w_lab = (float)((hwd - (double)(x2 - x1) * (double)(y2 - y1)) / hwd);
    }
    float* o = out + (int64_t)i * 8;
    o[0] = w_pix; o[1] = w_lab;
    o[2] = (float)x1; o[3] = (float)y1; o[4] = (float)x2; o[5] = (float)y2;
    o[6] = (float)mode; o[7] = lam;
  }
}

// The row as the pack kernels use it: the box clamped into [0, W] x [0, H] (a NaN clamps to 0), so no value of the
// row reaches an address -- it only chooses between the two in-range pixels and weighs them.
struct MixRow {
  float w;
  int x1, y1, x2, y2;
  bool blend;  // w != 1: a pixel outside the box needs the partner too
};
DPE_DEVICE MixRow mix_row(const float* __restrict__ prm, int H, int W) {
  MixRow m;
  m.w = prm[0];
  m.x1 = (int)fminf(fmaxf(prm[2], 0.f), (float)W);
  m.y1 = (int)fminf(fmaxf(prm[3], 0.f), (float)H);
  m.x2 = (int)fminf(fmaxf(prm[4], 0.f), (float)W);
  m.y2 = (int)fminf(fmaxf(prm[5], 0.f), (float)H);
  m.blend = !(m.w == 1.f);
  return m;
}
DPE_DEVICE float mix_px(const MixRow& m, bool inside, float a, float b) {
  return inside ? b : (m.blend ? m.w * a + (1.f - m.w) * b : a);
}

// nchw_to_s2d_kernel (eltwise.hip) with the mix: x NCHW f32 [N,C<=4,H,W] -> [N,H/2,W/2,16] bf16.  A pair of
// horizontal neighbours is read from the image itself unless both lie inside the box, and from the partner only
// if one lies inside or the row blends: cutmix reads one source per pixel (both for the pairs a box edge splits),
// mixup two.
__global__ __launch_bounds__(256) void mix_pack_s2d_kernel(const float* __restrict__ x, const float* __restrict__ prm,
                                                           uint16_t* __restrict__ y, int N, int C, int H, int W) {
  const MixRow m = mix_row(prm, H, W);
  const int Ho = H / 2, Wo = W / 2;
  const int64_t total = (int64_t)N * Ho * Wo;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int p = (int)(i % Wo);
    const int64_t t = i / Wo;
    const int q = (int)(t % Ho);
    const int n = (int)(t / Ho);
    const int pn = n == 0 ? N - 1 : n - 1;
    const bool in0 = 2 * p >= m.x1 && 2 * p < m.x2, in1 = 2 * p + 1 >= m.x1 && 2 * p + 1 < m.x2;
    float v[16];
#pragma unroll
    for (int ay = 0; ay < 2; ++ay) {
      const int r = 2 * q + ay;
      const bool iny = r >= m.y1 && r < m.y2;
      const bool i0 = iny && in0, i1 = iny && in1;
      const bool own = !(i0 && i1), other = i0 || i1 || m.blend;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float2 a = float2{0.f, 0.f}, b = float2{0.f, 0.f};
        if (c < C) {
          if (own) a = *(const float2*)(x + (((int64_t)n * C + c) * H + r) * W + 2 * p);
          if (other) b = *(const float2*)(x + (((int64_t)pn * C + c) * H + r) * W + 2 * p);
        }
        v[ay * 8 + c] = mix_px(m, i0, a.x, b.x);  // j = c + 4 ax + 8 ay
        v[ay * 8 + 4 + c] = mix_px(m, i1, a.y, b.y);
      }
    }
    u32x4* o = (u32x4*)(y + i * 16);
    o[0] = pack8(v);
    o[1] = pack8(v + 8);
  }
}

// nchw_to_nhwc_kernel (eltwise.hip) with the mix: x NCHW f32 -> NHWC bf16, channels padded to Cp with zeros
__global__ __launch_bounds__(256) void mix_pack_nhwc_kernel(const float* __restrict__ x, const float* __restrict__ prm,
                                                            uint16_t* __restrict__ y, int N, int C, int H, int W, int Cp) {
  const MixRow m = mix_row(prm, H, W);
  const int HW = H * W;
  const int64_t total = (int64_t)N * HW;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int n = (int)(i / HW), hw = (int)(i % HW);
    const int r = hw / W, col = hw % W;
    const int pn = n == 0 ? N - 1 : n - 1;
    const bool inside = r >= m.y1 && r < m.y2 && col >= m.x1 && col < m.x2;
    for (int c = 0; c < Cp; ++c) {
      float o = 0.f;
      if (c < C) {
        const float a = inside ? 0.f : x[((int64_t)n * C + c) * HW + hw];
        const float b = (inside || m.blend) ? x[((int64_t)pn * C + c) * HW + hw] : 0.f;
        o = mix_px(m, inside, a, b);
      }
      y[i * Cp + c] = c < C ? f2bf(o) : (uint16_t)0;
    }
  }
}

}  // namespace dpe

using namespace dpe;

static inline int mix_grid(int64_t work) {
  const int64_t g = (work + 255) / 256;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

// out: count rows of 8 floats.  rng: device int64[2] (seed, offset), not advanced here.
extern "C" int dpe_mix_draw(const int64_t* rng, uint32_t stream, int H, int W, float mixup_alpha, float cutmix_alpha,
                            float prob, float switch_prob, int count, float* out, hipStream_t st) {
  if (!rng || !out || H <= 0 || W <= 0 || H > 65536 || W > 65536 || count <= 0) return -1;
  if (!(mixup_alpha >= 0.f) || !(cutmix_alpha >= 0.f) || !(prob >= 0.f && prob <= 1.f) ||
      !(switch_prob >= 0.f && switch_prob <= 1.f))
    return -1;
  const int threads = count >= 256 ? 256 : ((count + 63) / 64) * 64;
  hipLaunchKernelGGL(mix_draw_kernel, dim3(1), dim3(threads), 0, st, rng, stream, H, W, mixup_alpha, cutmix_alpha, prob,
                     switch_prob, count, out);
  return (int)hipGetLastError();
}

// layout 0: space-to-depth [N,H/2,W/2,16] (C <= 4, even H and W); 1: NHWC [N,H,W,Cp], Cp >= C.  x and y 16-B aligned.
extern "C" int dpe_mix_pack(const float* x, const float* prm, uint16_t* y, int N, int C, int H, int W, int layout, int Cp,
                            hipStream_t st) {
  if (!x || !prm || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffffLL) return -1;
  if (layout == 0) {
    if (C > 4 || (H & 1) || (W & 1) || ((uintptr_t)x % 8) || ((uintptr_t)y % 16)) return -1;
    hipLaunchKernelGGL(mix_pack_s2d_kernel, dim3(mix_grid((int64_t)N * (H / 2) * (W / 2))), dim3(256), 0, st, x, prm, y, N, C,
                       H, W);
  } else if (layout == 1) {
    if (Cp < C) return -1;
    hipLaunchKernelGGL(mix_pack_nhwc_kernel, dim3(mix_grid((int64_t)N * H * W)), dim3(256), 0, st, x, prm, y, N, C, H, W, Cp);
  } else {
    return -1;
  }
  return (int)hipGetLastError();
}
