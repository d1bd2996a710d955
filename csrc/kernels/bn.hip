// BatchNorm2d training/eval kernels for NHWC bf16 activations (x viewed as
// [M = N*H*W][C], C % 8 == 0).  Memory-bound: every pass moves 16 B per lane.
//
//  stats_partial : per-block partial (sum, sumsq) over a row range  -> [nb][2][C]
//  finalize      : reduce partials in fp64, update running stats, emit
//                  per-channel (scale, shift, mean, invstd)          -> [4][C]
//  apply         : y = act(x*scale + shift [+ residual])
//  bwd_reduce    : partial (sum dz, sum dz*(x-mean)), dz = dy * relu'(y)
//  bwd_finalize  : dgamma/dbeta + the affine dx = a*dz + b*x + c coefficients
//  bwd_apply     : dx = a*dz + b*x + c   [+ write dz for a residual branch]
//
// When a GEMM epilogue already accumulated the column (sum, sumsq) for this
// BN (igemm col_stats), `finalize` is called with nb = 1 on that buffer and
// the stats pass is skipped entirely.
#include <cstdlib>
#include "common.h"
#include "launch.h"

namespace dpe {

constexpr int BN_T = 256;

DPE_DEVICE uint8_t mask_byte(const u32x4& pk) { return relu_mask_byte(pk); }

// Thread layout for a [rows][C] pass: chunk c = tid % CPR (8 channels), row phase tid / CPR.
__global__ __launch_bounds__(BN_T) void bn_stats_partial_kernel(const uint16_t* __restrict__ x, int64_t M, int C,
                                                                int64_t rows_per_block, float* __restrict__ part) {
  const int CPR = C >> 3;
  const int tid = threadIdx.x;
  const int RPI = BN_T / CPR;  // rows per iteration (CPR <= 256)
  const int c = tid % CPR, r = tid / CPR;
  const int64_t rb = blockIdx.x * rows_per_block;
  const int64_t re = min(M, rb + rows_per_block);
  float s[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
  if (r < RPI) {
    for (int64_t row = rb + r; row < re; row += RPI) {
      float f[8];
      unpack8(*(const u32x4*)(x + row * C + c * 8), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[e] += f[e]; q[e] += f[e] * f[e]; }
    }
  }
  __shared__ float red[2][BN_T][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[0][tid][e] = s[e]; red[1][tid][e] = q[e]; }
  __syncthreads();
  // each of the first C threads sums its channel over RPI row-phases
  for (int ch = tid; ch < C; ch += BN_T) {
    const int cc = ch >> 3, e = ch & 7;
    float a = 0.f, b = 0.f;
    for (int rr = 0; rr < RPI; ++rr) { a += red[0][rr * CPR + cc][e]; b += red[1][rr * CPR + cc][e]; }
    part[(int64_t)ch * gridDim.x + blockIdx.x] = a;
    part[(int64_t)(C + ch) * gridDim.x + blockIdx.x] = b;
  }
}

// Sum channel ch's nb partials (layout [2][C][nb]) with the whole NTHR-thread
// block (the conv-epilogue partials number M/BM -- 12,544 per channel for the
// first stage at batch 512 -- so a narrow block was latency-bound): four
// independent fp64 accumulator pairs per thread keep 8 loads in flight.
// Result valid in thread 0.
template <int NTHR>
DPE_DEVICE void block_sum2(const float* __restrict__ part, int nb, int C, int ch, double& s, double& q) {
  constexpr int NW = NTHR / 64;
  __shared__ double red[2][NW];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
  const float* ps = part + (int64_t)ch * nb;
  const float* pq = part + (int64_t)(C + ch) * nb;
  int i = threadIdx.x;
  for (; i + 3 * NTHR < nb; i += 4 * NTHR) {
    const float x0 = ps[i], x1 = ps[i + NTHR], x2 = ps[i + 2 * NTHR], x3 = ps[i + 3 * NTHR];
    const float y0 = pq[i], y1 = pq[i + NTHR], y2 = pq[i + 2 * NTHR], y3 = pq[i + 3 * NTHR];
    a0 += x0; a1 += x1; a2 += x2; a3 += x3;
    b0 += y0; b1 += y1; b2 += y2; b3 += y3;
  }
  for (; i < nb; i += NTHR) { a0 += ps[i]; b0 += pq[i]; }
  double a = (a0 + a1) + (a2 + a3), b = (b0 + b1) + (b2 + b3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
  if (lane == 0) { red[0][wid] = a; red[1][wid] = b; }
  __syncthreads();
  s = 0.0; q = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w) { s += red[0][w]; q += red[1][w]; }
}

// out: [4][C] = scale, shift, mean, invstd
template <int NTHR>
__global__ __launch_bounds__(NTHR) void bn_finalize_kernel(const float* __restrict__ part, int nb, int C, int64_t M,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ rmean, float* __restrict__ rvar,
                                                           float momentum, float eps, float* __restrict__ out) {
  const int ch = blockIdx.x;
  double s, q;
  block_sum2<NTHR>(part, nb, C, ch, s, q);
  if (threadIdx.x != 0) return;
  const double mean = s / (double)M;
  double var = q / (double)M - mean * mean;
  if (var < 0) var = 0;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float g = gamma ? gamma[ch] : 1.f, bt = beta ? beta[ch] : 0.f;
  const float sc = g * invstd;
  out[ch] = sc;
  out[C + ch] = bt - (float)mean * sc;
  out[2 * C + ch] = (float)mean;
  out[3 * C + ch] = invstd;
  if (rmean) {
    const double unbiased = M > 1 ? var * (double)M / (double)(M - 1) : var;
    rmean[ch] = (1.f - momentum) * rmean[ch] + momentum * (float)mean;
    rvar[ch] = (1.f - momentum) * rvar[ch] + momentum * (float)unbiased;
  }
}

// eval-mode coefficients from running stats
__global__ void bn_eval_coeff_kernel(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                                     float eps, float* out) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= C) return;
  const float invstd = rsqrtf(rvar[ch] + eps);
  const float sc = (gamma ? gamma[ch] : 1.f) * invstd;
  out[ch] = sc;
  out[C + ch] = (beta ? beta[ch] : 0.f) - rmean[ch] * sc;
  out[2 * C + ch] = rmean[ch];
  out[3 * C + ch] = invstd;
}

// Elementwise BN passes: one 16-B chunk per thread over a grid that covers the tensor exactly.
// Measured on MI355X (scripts/stream_probe.hip, 2 reads + 1 write of bf16): 5.9-6.0 TB/s for this
// form vs 4.4-5.3 TB/s for a 4096-block grid-stride loop with 4 chunks in flight per thread
// (the previous form of these passes; 822 MB tensors 566 -> 411 us), 5.4-5.7 with 2-8 chunks per
// thread, and plain loads >= non-temporal ones.  The per-channel coefficients come from a tiny
// L2-resident table; a block's 256 chunks share one channel phase when C/8 divides 256.

template <int NCOEF>
struct Coef8 {
  float v[NCOEF][8];
  DPE_DEVICE void load(const float* __restrict__ base, int C, int c8) {
#pragma unroll
    for (int k = 0; k < NCOEF; ++k) {
      const f32x4 a = *(const f32x4*)(base + k * C + c8), b = *(const f32x4*)(base + k * C + c8 + 4);
      v[k][0] = a[0]; v[k][1] = a[1]; v[k][2] = a[2]; v[k][3] = a[3];
      v[k][4] = b[0]; v[k][5] = b[1]; v[k][6] = b[2]; v[k][7] = b[3];
    }
  }
};

// A block covers U*256 consecutive chunks; thread t takes chunks base + u*256 + t (u < U), which
// share one channel whenever C/8 divides 256, so the coefficients are loaded once per thread.
template <typename I, int U>
struct Chunks {
  I base;
  int c8;
  bool same;  // every u of this thread is one channel
  DPE_DEVICE Chunks(int C) {
    const int CPR = C >> 3;
    base = (I)blockIdx.x * (BN_T * U) + threadIdx.x;
    same = (BN_T % CPR) == 0;
    c8 = (int)(base % (I)CPR) * 8;
  }
  DPE_DEVICE I at(int u) const { return base + (I)(u * BN_T); }
  DPE_DEVICE int chan(int u, int C) const { return same ? c8 : (int)(at(u) % (I)(C >> 3)) * 8; }
};

// y = act(x*scale + shift [+ res])
template <typename I, int U>
__global__ __launch_bounds__(BN_T) void bn_apply_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ res,
                                                        uint16_t* __restrict__ y, int64_t nchunks, int C,
                                                        const float* __restrict__ coef, int relu,
                                                        uint8_t* __restrict__ mbits) {
  const Chunks<I, U> ch(C);
  u32x4 xr[U], rr[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const I i = min(ch.at(u), (I)(nchunks - 1));
    xr[u] = *(const u32x4*)(x + (size_t)i * 8);
    if (res) rr[u] = *(const u32x4*)(res + (size_t)i * 8);
  }
  Coef8<2> cf;
  cf.load(coef, C, ch.c8);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const I i = ch.at(u);
    if ((int64_t)i >= nchunks) break;
    if (!ch.same) cf.load(coef, C, ch.chan(u, C));
    float f[8], g[8];
    unpack8(xr[u], f);
    if (res) unpack8(rr[u], g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = fmaf(f[e], cf.v[0][e], cf.v[1][e]);
      if (res) v += g[e];
      if (relu) v = fmaxf(v, 0.f);
      f[e] = v;
    }
    const u32x4 pk = pack8(f);
    *(u32x4*)(y + (size_t)i * 8) = pk;
    if (mbits) mbits[i] = mask_byte(pk);
  }
}

// y = act(x*scale + shift + x2*scale2 + shift2): a bottleneck's BN3 output plus its
// BN'd downsample branch in one pass (the downsample BN output is never stored).
template <typename I, int U>
__global__ __launch_bounds__(BN_T) void bn_apply2_kernel(const uint16_t* __restrict__ x, const float* __restrict__ coef,
                                                         const uint16_t* __restrict__ x2, const float* __restrict__ coef2,
                                                         uint16_t* __restrict__ y, int64_t nchunks, int C, int relu,
                                                         uint8_t* __restrict__ mbits) {
  const Chunks<I, U> ch(C);
  u32x4 xr[U], x2r[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const I i = min(ch.at(u), (I)(nchunks - 1));
    xr[u] = *(const u32x4*)(x + (size_t)i * 8);
    x2r[u] = *(const u32x4*)(x2 + (size_t)i * 8);
  }
  Coef8<2> cf, cf2;
  cf.load(coef, C, ch.c8);
  cf2.load(coef2, C, ch.c8);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const I i = ch.at(u);
    if ((int64_t)i >= nchunks) break;
    if (!ch.same) {
      cf.load(coef, C, ch.chan(u, C));
      cf2.load(coef2, C, ch.chan(u, C));
    }
    float f[8], g[8];
    unpack8(xr[u], f);
    unpack8(x2r[u], g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      // the residual is rounded to bf16 first, as when it is materialised
      const float r = bf2f(f2bf(fmaf(g[e], cf2.v[0][e], cf2.v[1][e])));
      float v = fmaf(f[e], cf.v[0][e], cf.v[1][e]) + r;
      if (relu) v = fmaxf(v, 0.f);
      f[e] = v;
    }
    const u32x4 pk = pack8(f);
    *(u32x4*)(y + (size_t)i * 8) = pk;
    if (mbits) mbits[i] = mask_byte(pk);
  }
}

// partial sums of dz and dz*(x-mean), dz = dy * (y > 0 if relu)
// ybits: the ReLU mask as bits of y (one byte per 8 columns, bn_apply's want_mask) instead of y itself
// With adx: the same pass also applies ANOTHER BatchNorm's backward to the same dz,
// adx = a*dz + b*ax + c (abcoef [3][C]) -- a bottleneck's BN3 apply fused with its
// downsample BN's reduce (both are functions of dz3): dz3 is read once.
// RELU (compile-time: 0 none, 1 y > 0, 2 ybits) and ADX select the operands, so no load sits under a
// run-time branch, and the row tail is clamped (loads always issued, the rows past the end masked out of
// the sums and their adx stores dropped by the buffer unit): a load or store under a lane-divergent test
// made the compiler drain every load in flight, 7 full vmcnt(0) per trip (the layer-3/4 reduces ran at
// 2.6-4.1 TB/s, 182 VGPRs for the union of the variants' operands).
constexpr uint32_t BN_OOB = 0x80000000u;
template <int U, int RELU, bool ADX>
__global__ __launch_bounds__(BN_T) void bn_bwd_reduce_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
                                                             const uint8_t* __restrict__ ybits,
                                                             const uint16_t* __restrict__ x, const float* __restrict__ coef,
                                                             int64_t M, int C, int64_t rows_per_block, float* __restrict__ part,
                                                             const uint16_t* __restrict__ ax, const float* __restrict__ abcoef,
                                                             uint16_t* __restrict__ adx) {
  const int CPR = C >> 3;
  const int tid = threadIdx.x;
  const int RPI = BN_T / CPR;
  const int c = tid % CPR, r = tid / CPR;
  const int64_t rb = blockIdx.x * rows_per_block;
  const int64_t re = min(M, rb + rows_per_block);
  float s[8], q[8], mean[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; mean[e] = coef[2 * C + c * 8 + e]; }
  Coef8<3> ac;
  if constexpr (ADX) ac.load(abcoef, C, c * 8);
  // adx stores through a buffer resource: a tail row's offset is out of range and the store is dropped
  const __amdgpu_buffer_rsrc_t adr = __builtin_amdgcn_make_buffer_rsrc(
      ADX ? (void*)adx : (void*)part, (short)0, ADX ? (int)min<int64_t>(M * C * 2, 0x7fffffffll) : 0, 0x00020000);
  if (r < RPI && rb < re) {
    // U rows per thread per iteration, all of their loads issued before the first use
    for (int64_t row0 = rb + r; row0 < re; row0 += (int64_t)U * RPI) {
      u32x4 rd[U], rx[U], ra[ADX ? U : 1], ry[RELU == 1 ? U : 1];
      uint32_t mbits[RELU == 2 ? U : 1];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t row = min(row0 + (int64_t)u * RPI, re - 1);
        const int64_t off = row * C + c * 8;
        rd[u] = *(const u32x4*)(dy + off);
        rx[u] = *(const u32x4*)(x + off);
        if constexpr (ADX) ra[u] = *(const u32x4*)(ax + off);
        if constexpr (RELU == 2) mbits[u] = ybits[off >> 3];
        if constexpr (RELU == 1) ry[u] = *(const u32x4*)(y + off);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t row = row0 + (int64_t)u * RPI;
        const bool ok = row < re;
        const int64_t off = row * C + c * 8;
        float d[8], xv[8];
        unpack8(rd[u], d);
        unpack8(rx[u], xv);
        if constexpr (ADX) {
          float av[8], o[8];
          unpack8(ra[u], av);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = fmaf(ac.v[0][e], d[e], fmaf(ac.v[1][e], av[e], ac.v[2][e]));
          __builtin_amdgcn_raw_buffer_store_b128(pack8(o), adr, ok ? (uint32_t)(off * 2) : BN_OOB, 0, 0);
        }
        if constexpr (RELU == 2) {
          const uint32_t mb = ok ? mbits[u] : 0u;
#pragma unroll
          for (int e = 0; e < 8; ++e) d[e] = ((mb >> e) & 1u) ? d[e] : 0.f;
        } else {
          float yv[8];
          if constexpr (RELU == 1) unpack8(ry[u], yv);
#pragma unroll
          for (int e = 0; e < 8; ++e) d[e] = (ok && (RELU == 0 || yv[e] > 0.f)) ? d[e] : 0.f;
        }
#pragma unroll
        // (explicit fma: every RELU / ADX instantiation rounds the same way -- the compiler's own contraction
        // choice differed between them, and the y / ybits paths must agree bit for bit)
        for (int e = 0; e < 8; ++e) { s[e] += d[e]; q[e] = fmaf(d[e], xv[e] - mean[e], q[e]); }
      }
    }
  }
  __shared__ float red[2][BN_T][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[0][tid][e] = s[e]; red[1][tid][e] = q[e]; }
  __syncthreads();
  for (int ch = tid; ch < C; ch += BN_T) {
    const int cc = ch >> 3, e = ch & 7;
    float a = 0.f, b = 0.f;
    for (int rr = 0; rr < RPI; ++rr) { a += red[0][rr * CPR + cc][e]; b += red[1][rr * CPR + cc][e]; }
    part[(int64_t)ch * gridDim.x + blockIdx.x] = a;
    part[(int64_t)(C + ch) * gridDim.x + blockIdx.x] = b;
  }
}

// bcoef: [3][C] = a, b, c  for dx = a*dz + b*x + c ; dgamma/dbeta accumulated (+=) into fp32 grads
template <int NTHR>
__global__ __launch_bounds__(NTHR) void bn_bwd_finalize_kernel(const float* __restrict__ part, int nb, int C, int64_t M,
                                                               const float* __restrict__ gamma, const float* __restrict__ coef,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                               float* __restrict__ bcoef) {
  const int ch = blockIdx.x;
  double s, q;
  block_sum2<NTHR>(part, nb, C, ch, s, q);
  if (threadIdx.x != 0) return;
  const float mean = coef[2 * C + ch], invstd = coef[3 * C + ch];
  const float g = gamma ? gamma[ch] : 1.f;
  if (dgamma) dgamma[ch] += (float)(q * invstd);
  if (dbeta) dbeta[ch] += (float)s;
  const float k1 = g * invstd;
  const float invM = 1.f / (float)M;
  const float a = k1;
  const float b = -k1 * invstd * invstd * (float)q * invM;
  const float c = -k1 * (float)s * invM - b * mean;
  bcoef[ch] = a;
  bcoef[C + ch] = b;
  bcoef[2 * C + ch] = c;
}

// ReLU mask: from y (y > 0) when y is given, else from the pre-BN input and the
// forward coefficients (x*scale + shift > 0) when mcoef is given (the BN output
// was never materialised: it was applied in the consumer's load prologue).
template <typename I, int U>
__global__ __launch_bounds__(BN_T) void bn_bwd_apply_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
                                                            const uint8_t* __restrict__ ybits,
                                                            const uint16_t* __restrict__ x, const float* __restrict__ bcoef,
                                                            uint16_t* __restrict__ dx, uint16_t* __restrict__ dz_out,
                                                            int64_t nchunks, int C, const float* __restrict__ mcoef) {
  const Chunks<I, U> ch(C);
  u32x4 dr[U], xr[U], yr[U];
  uint32_t mb[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const I i = min(ch.at(u), (I)(nchunks - 1));
    dr[u] = *(const u32x4*)(dy + (size_t)i * 8);
    xr[u] = *(const u32x4*)(x + (size_t)i * 8);
    if (ybits) mb[u] = ybits[i];
    else if (y) yr[u] = *(const u32x4*)(y + (size_t)i * 8);
  }
  Coef8<3> bc;
  Coef8<2> mc;
  bc.load(bcoef, C, ch.c8);
  if (mcoef) mc.load(mcoef, C, ch.c8);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const I i = ch.at(u);
    if ((int64_t)i >= nchunks) break;
    if (!ch.same) {
      bc.load(bcoef, C, ch.chan(u, C));
      if (mcoef) mc.load(mcoef, C, ch.chan(u, C));
    }
    float d[8], xv[8];
    unpack8(dr[u], d);
    unpack8(xr[u], xv);
    if (ybits) {
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = ((mb[u] >> e) & 1u) ? d[e] : 0.f;
    } else if (y) {
      float yv[8];
      unpack8(yr[u], yv);
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = yv[e] > 0.f ? d[e] : 0.f;
    } else if (mcoef) {
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = fmaf(xv[e], mc.v[0][e], mc.v[1][e]) > 0.f ? d[e] : 0.f;
    }
    if (dz_out) *(u32x4*)(dz_out + (size_t)i * 8) = pack8(d);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaf(bc.v[0][e], d[e], fmaf(bc.v[1][e], xv[e], bc.v[2][e]));
    *(u32x4*)(dx + (size_t)i * 8) = pack8(o);
  }
}

// bn_apply_kernel with the residual and the mask-bits store compile-time, one channel per thread, tail
// clamped (a chunk of the last row recomputed and stored again): no load or store under a run-time test.
template <typename I, int U, bool RES, bool MB>
__global__ __launch_bounds__(BN_T) void bn_apply_lean_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ res,
                                                             uint16_t* __restrict__ y, int64_t nchunks, int C,
                                                             const float* __restrict__ coef, int relu,
                                                             uint8_t* __restrict__ mbits) {
  const Chunks<I, U> ch(C);
  u32x4 xr[U], rr[RES ? U : 1];
  I idx[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    // past the end: the last row's chunk of this thread's own channel (nchunks is a multiple of C / 8), so
    // the recomputed chunk uses the coefficients it was computed with and stores the same bytes
    const I i = min(ch.at(u), (I)(nchunks - (C >> 3) + (ch.c8 >> 3)));
    idx[u] = i;
    xr[u] = *(const u32x4*)(x + (size_t)i * 8);
    if constexpr (RES) rr[u] = *(const u32x4*)(res + (size_t)i * 8);
  }
  Coef8<2> cf;
  cf.load(coef, C, ch.c8);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float f[8], g[8];
    unpack8(xr[u], f);
    if constexpr (RES) unpack8(rr[u], g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = fmaf(f[e], cf.v[0][e], cf.v[1][e]);
      if constexpr (RES) v += g[e];
      if (relu) v = fmaxf(v, 0.f);
      f[e] = v;
    }
    const u32x4 pk = pack8(f);
    *(u32x4*)(y + (size_t)idx[u] * 8) = pk;
    if constexpr (MB) mbits[idx[u]] = mask_byte(pk);
  }
}

// bn_bwd_apply_kernel with the mask source (MODE 0 none, 1 y > 0, 2 ybits, 3 mcoef) and the dz store
// compile-time, one channel per thread (C / 8 divides the block), and the tail clamped rather than cut: a
// thread past the end recomputes a chunk of the last row and stores the same bytes again, so no load or store sits
// under a run-time or lane-divergent test (the generic kernel: 7 full vmcnt drains, loads and stores
// serialised; 34 launches and 2.2 ms of the ResNet-50 step).
template <typename I, int U, int MODE, bool DZ>
__global__ __launch_bounds__(BN_T) void bn_bwd_apply_lean_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
                                                                 const uint8_t* __restrict__ ybits,
                                                                 const uint16_t* __restrict__ x, const float* __restrict__ bcoef,
                                                                 uint16_t* __restrict__ dx, uint16_t* __restrict__ dz_out,
                                                                 int64_t nchunks, int C, const float* __restrict__ mcoef) {
  const Chunks<I, U> ch(C);
  u32x4 dr[U], xr[U], yr[MODE == 1 ? U : 1];
  uint32_t mb[MODE == 2 ? U : 1];
  I idx[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    // past the end: the last row's chunk of this thread's own channel (nchunks is a multiple of C / 8), so
    // the recomputed chunk uses the coefficients it was computed with and stores the same bytes
    const I i = min(ch.at(u), (I)(nchunks - (C >> 3) + (ch.c8 >> 3)));
    idx[u] = i;
    dr[u] = *(const u32x4*)(dy + (size_t)i * 8);
    xr[u] = *(const u32x4*)(x + (size_t)i * 8);
    if constexpr (MODE == 2) mb[u] = ybits[i];
    if constexpr (MODE == 1) yr[u] = *(const u32x4*)(y + (size_t)i * 8);
  }
  Coef8<3> bc;
  Coef8<MODE == 3 ? 2 : 1> mc;
  bc.load(bcoef, C, ch.c8);
  if constexpr (MODE == 3) mc.load(mcoef, C, ch.c8);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const I i = idx[u];
    float d[8], xv[8];
    unpack8(dr[u], d);
    unpack8(xr[u], xv);
    if constexpr (MODE == 2) {
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = ((mb[u] >> e) & 1u) ? d[e] : 0.f;
    } else if constexpr (MODE == 1) {
      float yv[8];
      unpack8(yr[u], yv);
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = yv[e] > 0.f ? d[e] : 0.f;
    } else if constexpr (MODE == 3) {
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = fmaf(xv[e], mc.v[0][e], mc.v[1][e]) > 0.f ? d[e] : 0.f;
    }
    if constexpr (DZ) *(u32x4*)(dz_out + (size_t)i * 8) = pack8(d);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaf(bc.v[0][e], d[e], fmaf(bc.v[1][e], xv[e], bc.v[2][e]));
    *(u32x4*)(dx + (size_t)i * 8) = pack8(o);
  }
}

}  // namespace dpe

using namespace dpe;

template <int U>
static unsigned grid_for(int64_t nchunks) {  // exact cover: U 16-B chunks per thread
  const int64_t g = (nchunks + BN_T * U - 1) / (BN_T * U);
  return (unsigned)(g < 1 ? 1 : g);
}
#define BN_LAUNCH_U(KERN, I, UV, nch, ...)                                                                          \
  switch (UV) {                                                                                                     \
    case 1: hipLaunchKernelGGL((KERN<I, 1>), dim3(grid_for<1>(nch)), dim3(BN_T), 0, __VA_ARGS__); break;           \
    case 2: hipLaunchKernelGGL((KERN<I, 2>), dim3(grid_for<2>(nch)), dim3(BN_T), 0, __VA_ARGS__); break;           \
    default: hipLaunchKernelGGL((KERN<I, 4>), dim3(grid_for<4>(nch)), dim3(BN_T), 0, __VA_ARGS__); break;          \
  }

extern "C" int dpe_bn_stats_nblocks(int64_t M, int C) {
  // target ~1024 partial blocks but at least 64 rows each (1024 / 2048 / 4096: same step time)
  int64_t nb = M / 64;
  if (nb > 1024) nb = 1024;
  if (nb < 1) nb = 1;
  (void)C;
  return (int)nb;
}

// Blocks of the BN-backward reduce: as dpe_bn_stats_nblocks, but at >= 1024 channels (layers 3-4: a block row
// is one or two pixels) at least DPE_BNR_ROWS (default 64) rows per block, up to 2048 blocks
extern "C" int dpe_bn_bwd_nblocks(int64_t M, int C) {
  static const int rows = [] { const char* e = getenv("DPE_BNR_ROWS"); return e ? std::max(4, atoi(e)) : 64; }();
  if (C < 1024) return dpe_bn_stats_nblocks(M, C);
  int64_t nb = M / rows;
  if (nb > 2048) nb = 2048;
  if (nb < 1) nb = 1;
  return (int)nb;
}

extern "C" int dpe_bn_stats(const uint16_t* x, int64_t M, int C, int nb, float* part, hipStream_t st) {
  if (C % 8 || C / 8 > BN_T) return -1;
  const int64_t rpb = (M + nb - 1) / nb;
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(nb), dim3(BN_T), 0, st, x, M, C, rpb, part);
  return 0;
}

extern "C" int dpe_bn_finalize(const float* part, int nb, int C, int64_t M, const float* gamma, const float* beta,
                               float* rmean, float* rvar, float momentum, float eps, float* coef, hipStream_t st) {
  if (nb > 2048) {
    hipLaunchKernelGGL(bn_finalize_kernel<1024>, dim3(C), dim3(1024), 0, st, part, nb, C, M, gamma, beta, rmean, rvar,
                       momentum, eps, coef);
    return 0;
  }
  hipLaunchKernelGGL(bn_finalize_kernel<256>, dim3(C), dim3(256), 0, st, part, nb, C, M, gamma, beta, rmean, rvar,
                     momentum, eps, coef);
  return 0;
}

extern "C" int dpe_bn_eval_coeff(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                                 float eps, float* coef, hipStream_t st) {
  hipLaunchKernelGGL(bn_eval_coeff_kernel, dim3((C + 255) / 256), dim3(256), 0, st, C, gamma, beta, rmean, rvar, eps, coef);
  return 0;
}

extern "C" int dpe_bn_apply_m(const uint16_t* x, const uint16_t* res, uint16_t* y, int64_t M, int C, const float* coef,
                              int relu, uint8_t* mbits, hipStream_t st) {
  const int64_t nch = M * C / 8;
  // 2 chunks per thread (A/B, ResNet-50 step: 1 / 2 / 4 within noise for the forward applies)
  constexpr int U = 2;
  static const bool lean = [] { const char* e = getenv("DPE_BN_BWD_LEAN"); return !(e && e[0] == '0'); }();
  if (lean && nch < (1ll << 31) && C % 8 == 0 && BN_T % (C / 8) == 0) {
#define DPE_BAL(R_, M_)                                                                                           \
  if ((res != nullptr) == R_ && (mbits != nullptr) == M_) {                                                       \
    hipLaunchKernelGGL((bn_apply_lean_kernel<uint32_t, U, R_, M_>), dim3(grid_for<U>(nch)), dim3(BN_T), 0, st, x, res, y, \
                       nch, C, coef, relu, mbits);                                                                \
    return 0;                                                                                                     \
  }
    DPE_BAL(false, false) DPE_BAL(false, true) DPE_BAL(true, false) DPE_BAL(true, true)
#undef DPE_BAL
  }
  if (nch < (1ll << 31)) {
    BN_LAUNCH_U(bn_apply_kernel, uint32_t, U, nch, st, x, res, y, nch, C, coef, relu, mbits)
  } else {
    BN_LAUNCH_U(bn_apply_kernel, int64_t, U, nch, st, x, res, y, nch, C, coef, relu, mbits)
  }
  return 0;
}

extern "C" int dpe_bn_apply(const uint16_t* x, const uint16_t* res, uint16_t* y, int64_t M, int C, const float* coef,
                            int relu, hipStream_t st) {
  return dpe_bn_apply_m(x, res, y, M, C, coef, relu, nullptr, st);
}

extern "C" int dpe_bn_apply2(const uint16_t* x, const float* coef, const uint16_t* x2, const float* coef2, uint16_t* y,
                             int64_t M, int C, int relu, uint8_t* mbits, hipStream_t st) {
  const int64_t nch = M * C / 8;
  constexpr int U = 2;
  if (nch < (1ll << 31)) {
    BN_LAUNCH_U(bn_apply2_kernel, uint32_t, U, nch, st, x, coef, x2, coef2, y, nch, C, relu, mbits)
  } else {
    BN_LAUNCH_U(bn_apply2_kernel, int64_t, U, nch, st, x, coef, x2, coef2, y, nch, C, relu, mbits)
  }
  return 0;
}

extern "C" int dpe_bn_bwd_reduce(const uint16_t* dy, const uint16_t* y, const uint8_t* ybits, const uint16_t* x,
                                 const float* coef, int64_t M, int C, int nb, float* part, hipStream_t st) {
  if (C % 8 || C / 8 > BN_T) return -1;
  const int64_t rpb = (M + nb - 1) / nb;
#define DPE_BNR(RELU_)                                                                                          \
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<4, RELU_, false>), dim3(nb), dim3(BN_T), 0, st, dy, y, ybits, x, coef, M, C, \
                     rpb, part, (const uint16_t*)nullptr, (const float*)nullptr, (uint16_t*)nullptr)
  if (ybits) DPE_BNR(2);
  else if (y) DPE_BNR(1);
  else DPE_BNR(0);
#undef DPE_BNR
  return 0;
}

// reduce (dz, x; coef) for one BatchNorm + apply adx = a*dz + b*ax + c for another, one pass
extern "C" int dpe_bn_bwd_reduce_apply(const uint16_t* dz, const uint16_t* x, const float* coef, const uint16_t* ax,
                                       const float* abcoef, uint16_t* adx, int64_t M, int C, int nb, float* part,
                                       hipStream_t st) {
  if (C % 8 || C / 8 > BN_T) return -1;
  const int64_t rpb = (M + nb - 1) / nb;
  if ((int64_t)M * C * 2 >= 0x7fffffffll) return -1;  // 32-bit buffer offsets of the adx stores
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<4, 0, true>), dim3(nb), dim3(BN_T), 0, st, dz, (const uint16_t*)nullptr,
                     (const uint8_t*)nullptr, x, coef, M, C, rpb, part, ax, abcoef, adx);
  return 0;
}

extern "C" int dpe_bn_bwd_finalize(const float* part, int nb, int C, int64_t M, const float* gamma, const float* coef,
                                   float* dgamma, float* dbeta, float* bcoef, hipStream_t st) {
  if (nb > 2048) {
    hipLaunchKernelGGL(bn_bwd_finalize_kernel<1024>, dim3(C), dim3(1024), 0, st, part, nb, C, M, gamma, coef, dgamma, dbeta,
                       bcoef);
    return 0;
  }
  hipLaunchKernelGGL(bn_bwd_finalize_kernel<256>, dim3(C), dim3(256), 0, st, part, nb, C, M, gamma, coef, dgamma,
                     dbeta, bcoef);
  return 0;
}

extern "C" int dpe_bn_bwd_apply(const uint16_t* dy, const uint16_t* y, const uint8_t* ybits, const uint16_t* x,
                                const float* bcoef, uint16_t* dx, uint16_t* dz_out, int64_t M, int C, const float* mcoef,
                                hipStream_t st) {
  const int64_t nch = M * C / 8;
  // three coefficient tables per thread: 2 chunks (4 at C >= 1024, where a block spans one row)
  // amortise them; ResNet-50 step 43.5 ms (1 chunk) -> 42.8 ms (2 chunks)
  const int U = C >= 1024 ? 4 : 2;
  static const bool lean = [] { const char* e = getenv("DPE_BN_BWD_LEAN"); return !(e && e[0] == '0'); }();
  if (lean && nch < (1ll << 31) && C % 8 == 0 && BN_T % (C / 8) == 0) {
    const int mode = ybits ? 2 : y ? 1 : mcoef ? 3 : 0;
#define DPE_BWL(U_, M_, DZ_)                                                                                     \
  if (U == U_ && mode == M_ && (dz_out != nullptr) == DZ_) {                                                     \
    hipLaunchKernelGGL((bn_bwd_apply_lean_kernel<uint32_t, U_, M_, DZ_>), dim3(grid_for<U_>(nch)), dim3(BN_T), 0, st, \
                       dy, y, ybits, x, bcoef, dx, dz_out, nch, C, mcoef);                                        \
    return 0;                                                                                                    \
  }
#define DPE_BWL_M(U_) DPE_BWL(U_, 0, false) DPE_BWL(U_, 1, false) DPE_BWL(U_, 2, false) DPE_BWL(U_, 3, false) \
                      DPE_BWL(U_, 0, true) DPE_BWL(U_, 1, true) DPE_BWL(U_, 2, true) DPE_BWL(U_, 3, true)
    DPE_BWL_M(2)
    DPE_BWL_M(4)
#undef DPE_BWL_M
#undef DPE_BWL
  }
  if (nch < (1ll << 31)) {
    BN_LAUNCH_U(bn_bwd_apply_kernel, uint32_t, U, nch, st, dy, y, ybits, x, bcoef, dx, dz_out, nch, C, mcoef)
  } else {
    BN_LAUNCH_U(bn_bwd_apply_kernel, int64_t, U, nch, st, dy, y, ybits, x, bcoef, dx, dz_out, nch, C, mcoef)
  }
  return 0;
}
