// BatchNorm-after-1x1-conv by Gram algebra (the ResNet bottleneck's conv3 -> BN3; SURVEY §7.4 hard
// part #3: BatchNorm bytes dominate once the GEMMs are fast).
//
// h3 = a2 W3^T is linear in a2 (the conv's input, [M][Cin], Cin = Cout / 4), so every per-channel
// reduction BN3 needs over h3's M rows is a reduction over a2 through two small matrices:
//   G = a2^T a2  [Cin][Cin],   s = colsum(a2)  [Cin]
//   forward:   sum_r h3[r,k]   = w_k . s            sum_r h3[r,k]^2 = w_k^T G w_k
//   backward:  P = dz3^T a2 (the weight-grad GEMM of dz3 -- the same cost as today's dh3^T a2)
//              sum_r dz3[r,k] h3[r,k] = w_k . P[k,:]
//              dW3 = sum_r dh3^T a2 = diag(a) P + diag(b) (W3 G) + c s^T          (dh3 = a dz3 + b h3 + c)
//              da2 = dh3 W3 = dz3 (diag(a) W3) + a2 (W3^T diag(b) W3) + c^T W3  -- one GEMM over the
//                    concatenated K = [dz3 | a2] x [diag(a) W3 ; Q]               (igemm AX_CAT)
// So BN3's statistics are known BEFORE conv3 runs (its epilogue writes relu(BN3(h3) + idn) directly:
// no h3 tensor, no bn_apply pass), and BN3's backward needs neither h3 nor a dh3 tensor (no
// bn_bwd_apply pass, no h3 re-read in the next block's data-grad epilogue).  The price is one read of
// a2 (a quarter of the block width) for G plus 2 M Cin^2 MFMA FLOPs, and Cin more K in the data grad.
//
// Kernels here: the Gram pass (partials per block + fixed-order reduction: deterministic), the forward
// coefficient kernel (BN3 scale / shift / mean / invstd + running stats, and u = W3 G for the
// backward), and the two backward coefficient kernels (BN3 parameter grads, the dW3 correction, the
// data grad's concatenated B operand and bias).
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "common.h"
#include "launch.h"

namespace dpe {
namespace gram {

constexpr int TR = 32;           // rows per tile (= the MFMA's K)
constexpr int TS = TR * 2 + 16;  // LDS bytes per channel row of the transposed tile (16 B pad: conflict-free b128 reads)

// Pilot shift of a = relu(z), z = x * scale + shift the BN output ([4][C] coefficients: scale, shift, mean,
// invstd of x): z ~ N(beta, sigma^2) with beta = shift + mean * scale, sigma = |scale| / invstd, so
// E[a] ~ beta Phi(beta / sigma) + sigma phi(beta / sigma).  Only an estimate is needed: any mu within
// O(std) of the true mean removes the cancellation.  mu is rounded to 5 significant bits: then for every
// bf16 a in [mu / 2, 8 mu] (and a = 0, the ReLU's zeros) bf16(a - mu) is EXACT -- mu's lowest bit is no
// finer than a's ulp -- so the once-more-rounded MFMA operand carries no error where the data sit, and no
// bias from mu's own low bits anywhere (what remains, a in (0, mu / 2), rounds a's varying low bits).
__device__ inline float relu_gauss_mean(const float* sc, int C, int c) {
  const float scale = sc[c], sh = sc[C + c], mean = sc[2 * C + c], invstd = sc[3 * C + c];
  const float beta = fmaf(mean, scale, sh);
  const float sigma = invstd > 0.f ? fabsf(scale) / invstd : 0.f;
  float mu = fmaxf(beta, 0.f);
  if (sigma > 0.f && isfinite(sigma)) {
    const float t = beta / sigma;
    mu = beta * 0.5f * (1.f + erff(t * 0.70710678f)) + sigma * 0.39894228f * expf(-0.5f * t * t);
  }
  if (!isfinite(mu)) return 0.f;
  const uint32_t b = (__float_as_uint(mu) + (1u << 18)) & ~((1u << 19) - 1u);  // 4 explicit mantissa bits
  return __uint_as_float(b);
}

// Partial Gram matrix and column sums of x' = relu(x * coef[c] + coef[C + c]) (coef != nullptr) or x,
// CENTRED on the pilot shift mu (relu_gauss_mean of scoef; 0 without scoef), over rows
// [blockIdx.x * rpb, +rpb): gp[block][C][C] (full, symmetric), sp[block][C] of x' - mu; block 0 also
// writes mu.  x' is rounded to bf16 exactly as the on-load BN transform of the conv kernels rounds their
// MFMA operand, so G + (mu terms) is the Gram matrix of the operand conv3 actually multiplies; x' - mu is
// exact in fp32 and rounded to bf16 once more for the MFMA (exact whenever it cancels, i.e. whenever
// precision matters).  Without the shift, E[h^2] - mean^2 cancels catastrophically once a channel's
// |mean| / std reaches ~30 (post-ReLU operands are non-negative): tests/test_bn3_gram_robust_gpu.py.
//
// A 32-row tile is loaded as 16-B row chunks: load slot (wave w, instruction i) covers rows
// 16 (slot % 2) + [0, 16) x chunks 4 (slot / 2) + [0, 4) (lane: row l / 4, chunk l % 4), and stored
// TRANSPOSED in LDS ([channel][32 rows], TS bytes per channel) so that an MFMA operand -- 8 consecutive
// rows of one channel -- is one ds_read_b128.  Lanes l and l + 4 hold rows r, r + 1 of the same
// channels: one swaps half its chunk with the other so each writes whole row-pair dwords (4 ds_write_b32
// instead of 8 ds_write_b16; the 16-row x 4-chunk slot spreads a store over 32 banks, 2-way).
template <int C, int NT = (C == 256 ? 512 : 256)>
__global__ __launch_bounds__(NT) void gram_partial_kernel(const uint16_t* __restrict__ x, const float* __restrict__ coef,
                                                           const float* __restrict__ scoef, int64_t M, int rpb,
                                                           float* __restrict__ gp, float* __restrict__ sp,
                                                           float* __restrict__ mu_out) {
  constexpr int NW = NT / 64;  // (C = 256: 8 waves, so each holds 17 accumulator fragments, not 34)
  constexpr int NB = C / 16, NF = NB * (NB + 1) / 2, FPW = (NF + NW - 1) / NW;
  constexpr int CPR = C / 8;          // 16-B chunks per row
  constexpr int CPT = TR * CPR / NT;  // load slots per wave per tile
  static_assert(CPT >= 1 && CPT * NT == TR * CPR && CPR % 4 == 0, "tile split");
  __shared__ __attribute__((aligned(16))) char tile[2][C * TS];
  __shared__ __attribute__((aligned(16))) float cf[2 * C];  // [scale | shift] of the on-load BN
  __shared__ __attribute__((aligned(16))) float mus[C];     // pilot shift

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = min<int64_t>(M, r0 + rpb);
  const int ntile = r0 < r1 ? (int)((r1 - r0 + TR - 1) / TR) : 0;
  const bool odd = (lane >> 2) & 1;  // row r + 1 of its pair
  if (coef)
    for (int i = tid; i < 2 * C; i += NT) cf[i] = coef[i];
  for (int c = tid; c < C; c += NT) {
    const float m = scoef ? relu_gauss_mean(scoef, C, c) : 0.f;
    mus[c] = m;
    if (blockIdx.x == 0) mu_out[c] = m;
  }

  int srow[CPT], scc[CPT];
  float csum[CPT][8];
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int slot = wid + NW * i;
    srow[i] = 16 * (slot & 1) + (lane >> 2);
    scc[i] = 4 * (slot >> 1) + (lane & 3);
#pragma unroll
    for (int e = 0; e < 8; ++e) csum[i][e] = 0.f;
  }
  __syncthreads();

  // fragments (I <= J) of wave wid: f = wid + NW i
  int fi[FPW], fj[FPW];
#pragma unroll
  for (int i = 0; i < FPW; ++i) {
    int f = wid + NW * i, I = 0;
    if (f >= NF) f = NF - 1;  // (padding slot: recomputes a valid fragment, never stored)
    while (f >= NB - I) { f -= NB - I; ++I; }
    fi[i] = I;
    fj[i] = I + f;
  }
  f32x4 acc[FPW];
#pragma unroll
  for (int i = 0; i < FPW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // register ring: the loads of the next U tiles are in flight while a tile is transposed and multiplied
  // (one tile ahead left the pass latency-bound: ~1.5 TB/s at C = 64)
  constexpr int U = CPT == 1 ? 8 : (NT == 256 ? 4 : 1);  // (C = 256 has no registers for a deeper ring)
  u32x4 ring[U][CPT];
  auto load = [&](int t, u32x4 (&ld)[CPT]) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int64_t m = r0 + (int64_t)t * TR + srow[i];
      ld[i] = (t < ntile && m < r1) ? *(const u32x4*)(x + m * C + 8 * scc[i]) : u32x4{0u, 0u, 0u, 0u};
    }
  };
#pragma unroll
  for (int u = 0; u < U; ++u) load(u, ring[u]);
  for (int t0 = 0; t0 < ntile; t0 += U)
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int t = t0 + u;
    if (t >= ntile) break;
    char* T = tile[t & 1];
    u32x4 (&ld)[CPT] = ring[u];
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const bool valid = r0 + (int64_t)t * TR + srow[i] < r1;
      float f[8];
      unpack8(ld[i], f);
      if (coef) {
        const f32x4* cs = (const f32x4*)(cf + 8 * scc[i]);
        const f32x4* ch = (const f32x4*)(cf + C + 8 * scc[i]);
        const f32x4 s0 = cs[0], s1 = cs[1], h0 = ch[0], h1 = ch[1];
        const float sc8[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
        const float sh8[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = valid ? fmaxf(fmaf(f[e], sc8[e], sh8[e]), 0.f) : 0.f;
        const u32x4 pr = pack8(f);
        unpack8(pr, f);  // the rounded operand
      }
      {
        const f32x4* cm = (const f32x4*)(mus + 8 * scc[i]);
        const f32x4 m0 = cm[0], m1 = cm[1];
        const float mu8[8] = {m0[0], m0[1], m0[2], m0[3], m1[0], m1[1], m1[2], m1[3]};
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = valid ? f[e] - mu8[e] : 0.f;  // (pad rows stay 0, not -mu)
      }
      const u32x4 pk = pack8(f);
      unpack8(pk, f);  // the centred MFMA operand
#pragma unroll
      for (int e = 0; e < 8; ++e) csum[i][e] += f[e];
      // even lane keeps channels 0-3 of its chunk and takes the odd partner's rows for them; the odd
      // lane keeps channels 4-7
      const uint32_t s0 = odd ? pk[0] : pk[2], s1 = odd ? pk[1] : pk[3];
      const uint32_t q0 = (uint32_t)__shfl_xor((int)s0, 4, 64), q1 = (uint32_t)__shfl_xor((int)s1, 4, 64);
      const uint32_t o0 = odd ? pk[2] : pk[0], o1 = odd ? pk[3] : pk[1];
      const int cb = 8 * scc[i] + (odd ? 4 : 0), p = srow[i] >> 1;
      const uint32_t own[2] = {o0, o1}, oth[2] = {q0, q1};
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        // (row r, row r + 1) halves: even lane = own is row r; odd lane = own is row r + 1
        const uint32_t rlo = odd ? oth[u] : own[u], rhi = odd ? own[u] : oth[u];
        *(uint32_t*)(T + (cb + 2 * u) * TS + p * 4) = (rlo & 0xffffu) | (rhi << 16);
        *(uint32_t*)(T + (cb + 2 * u + 1) * TS + p * 4) = (rlo >> 16) | (rhi & 0xffff0000u);
      }
    }
    load(t + U, ld);  // refill this ring slot (in flight across the next U - 1 tiles)
    __syncthreads();
    const int g = lane >> 4, li = lane & 15;
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
      const bf16x8 a = __builtin_bit_cast(bf16x8, *(const u32x4*)(T + (16 * fi[i] + li) * TS + g * 16));
      const bf16x8 b = __builtin_bit_cast(bf16x8, *(const u32x4*)(T + (16 * fj[i] + li) * TS + g * 16));
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[i], 0, 0, 0);
    }
    // (the next tile writes the other buffer; this one is rewritten two tiles on, after the barrier
    // above has been passed by every wave that read it)
  }
  // partial G: lane holds D[4 (lane / 16) + e][lane % 16] of fragment (I, J); mirrored below the diagonal
  float* G = gp + (int64_t)blockIdx.x * C * C;
  {
    const int g = lane >> 4, li = lane & 15;
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
      if (wid + NW * i >= NF) continue;
      const int I = fi[i], J = fj[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 16 * I + 4 * g + e, c = 16 * J + li;
        G[(int64_t)r * C + c] = acc[i][e];
        if (I != J) G[(int64_t)c * C + r] = acc[i][e];
      }
    }
  }
  // column sums: slot (wave, i) x lane -> chunk scc; fixed-order LDS reduction over the 32 (slot, lane)
  // pairs holding each chunk (2 row halves x 16 lanes)
  __syncthreads();
  float* rs = (float*)tile[0];  // [slot][64 lanes][8]
#pragma unroll
  for (int i = 0; i < CPT; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) rs[((wid + NW * i) * 64 + lane) * 8 + e] = csum[i][e];
  __syncthreads();
  for (int c8 = tid; c8 < CPR; c8 += NT) {  // chunk c8: slots 2 (c8 / 4) + {0, 1}, lanes = c8 % 4 (mod 4)
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    for (int h = 0; h < 2; ++h)
      for (int l = c8 % 4; l < 64; l += 4)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += rs[((2 * (c8 / 4) + h) * 64 + l) * 8 + e];
#pragma unroll
    for (int e = 0; e < 8; ++e) sp[(int64_t)blockIdx.x * C + 8 * c8 + e] = v[e];
  }
}

// The same partials, streamed by LDS-DMA (gram_partial_kernel above is register-staged: one tile ahead at
// C = 256 for lack of registers, ~14-35 % of HBM speed).  A 32-row tile [32][C] bf16 lands in an NS-deep
// LDS ring by buffer_load ... lds (rows past M read as zeros), row-major with 16-B chunk c of row r at
// c ^ 2 h(r) (h below: the MFMA operand's transposed reads are bank-conflict-free); the 256 threads then
// transform it IN PLACE -- thread (chunk c = tid % CPR) applies relu(x scale + shift), rounds, subtracts
// the pilot shift mu, rounds again (exactly the register-staged kernel's operand) and keeps the column
// sums of its 8 channels -- and every wave multiplies its fragments (I <= J) of G straight from the tile
// with ds_read_b64_tr_b16 (8 rows of 16 channels per operand).  Two barriers per tile.  Output layout and
// reduction order of the partials as gram_partial_kernel (fixed: deterministic).
DPE_DEVICE int gram_h(int row, int C) {
  return C >= 128 ? ((row & 3) | (((row >> 3) & 1) << 2)) : (((row >> 1) & 1) | (((row >> 3) & 1) << 1));
}
DPE_DEVICE void gram_dma16(__amdgpu_buffer_rsrc_t r, char* wave_dst, uint32_t voff, uint32_t soff) {
  const unsigned m0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)wave_dst);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               ::"s"(m0), "v"(voff), "s"(r), "s"(soff) : "memory");
}
template <int N>
DPE_DEVICE void gram_wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
  asm volatile("" ::: "memory");
}
typedef __attribute__((address_space(3))) s16x4 gram_lds4;

// fragment f of the upper triangle (I <= J, row-major) -> (I << 8) | J; f >= NF: the last one (padding)
constexpr int gram_frag(int f, int NB, int NF) {
  if (f >= NF) f = NF - 1;
  int I = 0;
  while (f >= NB - I) { f -= NB - I; ++I; }
  return (I << 8) | (I + f);
}

// does wave W (fragments W + NW i, i < FPW) read operand block I
constexpr bool gram_uses(int W, int I, int NB, int NF, int NW, int FPW) {
  for (int i = 0; i < FPW; ++i) {
    const int f = gram_frag(W + NW * i, NB, NF);
    if ((f >> 8) == I || (f & 255) == I) return true;
  }
  return false;
}
// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>)
template <class F, int... Is>
DPE_DEVICE void gram_sfor_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
DPE_DEVICE void gram_sfor(F&& f) {
  gram_sfor_impl(f, std::make_integer_sequence<int, N>{});
}

// Row m of the stride-2 subsample of an [*, sh, sw] image -> its pixel index (n, 2 oh, 2 ow) in the full image
DPE_DEVICE int64_t gram_s2_pixel(int64_t m, int sh, int sw) {
  const int ow_ = sw >> 1, per = (sh >> 1) * ow_;
  const int64_t n = m / per;
  const int r = (int)(m - n * per), oh = r / ow_, ow = r - oh * ow_;
  return (n * sh + 2 * oh) * sw + 2 * ow;
}

// STR: the M rows are the stride-2 subsample x[:, ::2, ::2, :] of an [*, sh, sw, C] image (a stride-2 1x1 conv's
// input pixels), taken by row addressing -- every DMA piece's rows are mapped to their pixel offsets per group
// (whole 2 C-byte pixel rows), no compacting copy.
template <int C, bool STR = false>
__global__ __launch_bounds__(512, 1) void gram_dma_kernel(const uint16_t* __restrict__ x, const float* __restrict__ coef,
                                                          const float* __restrict__ scoef, int64_t M, int rpb,
                                                          float* __restrict__ gp, float* __restrict__ sp,
                                                          float* __restrict__ mu_out, int sh, int sw) {
  constexpr int NT = 512, NW = 8;
  constexpr int CPR = C / 8, RB = 2 * C, SB = TR * RB;  // chunks per row, bytes per row / tile
  constexpr int NS = C == 256 ? 8 : (C == 128 ? 12 : 16); // ring depth (tiles)
  constexpr int GT = C == 64 ? 4 : 2, NG = NS / GT;        // tiles per step (one barrier pair), ring groups
  constexpr int DPG = GT * SB / 1024 / NW;                // DMA pieces (1 KiB) per wave per group
  constexpr int RPT = NT / CPR, TPG = GT * TR / RPT;      // transform: row stride, rows per thread per group
  constexpr int NB = C / 16, NF = NB * (NB + 1) / 2, FPW = (NF + NW - 1) / NW;
  static_assert(NG * GT == NS && NG >= 3 && DPG >= 1 && DPG * NW * 1024 == GT * SB && TPG * RPT == GT * TR, "split");
  __shared__ __attribute__((aligned(16))) char ring[NS * SB];
  __shared__ __attribute__((aligned(16))) float cf[3 * C];  // scale | shift | mu

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = min<int64_t>(M, r0 + rpb);
  const int ntile = r0 < r1 ? (int)((r1 - r0 + TR - 1) / TR) : 0;
  for (int c = tid; c < C; c += NT) {
    cf[c] = coef ? coef[c] : 1.f;
    cf[C + c] = coef ? coef[C + c] : 0.f;
    const float m = scoef ? relu_gauss_mean(scoef, C, c) : 0.f;
    cf[2 * C + c] = m;
    if (blockIdx.x == 0) mu_out[c] = m;
  }
  // DMA: lane l of the group's piece q (= wid + NW v) fills byte 1024 q + 16 l of the group's GT tiles
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(x), (short)0, (int)((STR ? 4 : 1) * M * C * 2), 0x00020000);
  uint32_t voff[DPG];  // (STR: the chunk's byte offset inside its pixel row; lrow = its row within the group)
  int lrow[DPG];
#pragma unroll
  for (int v = 0; v < DPG; ++v) {
    const int o = ((wid + NW * v) * 1024 + lane * 16) % SB, tk = ((wid + NW * v) * 1024) / SB;
    const int row = o / RB, chs = (o % RB) / 16;
    const int ch = chs ^ (2 * gram_h(row, C));
    lrow[v] = tk * TR + row;
    voff[v] = STR ? (uint32_t)(ch * 16) : (uint32_t)(((tk * TR + row) * C + ch * 8) * 2);
  }
  const int ngrp = (ntile + GT - 1) / GT;
  // group q = tiles [q GT, q GT + GT) in ring slots (q % NG) GT + [0, GT); rows past the block's range (the
  // next block's, or zeros past M) are masked in the transform
  auto dma_group = [&](int q) {
    char* slot = ring + (q % NG) * GT * SB;
    if constexpr (STR) {
      // (rows past M are clamped to the last row: in range, masked in the transform)
#pragma unroll
      for (int v = 0; v < DPG; ++v) {
        const int64_t m = min<int64_t>(r0 + (int64_t)q * GT * TR + lrow[v], M - 1);
        gram_dma16(rs, slot + (wid + NW * v) * 1024, (uint32_t)(gram_s2_pixel(m, sh, sw) * (C * 2)) + voff[v], 0u);
      }
      return;
    }
    const uint32_t so = (uint32_t)((r0 + (int64_t)q * GT * TR) * C * 2);
#pragma unroll
    for (int v = 0; v < DPG; ++v) gram_dma16(rs, slot + (wid + NW * v) * 1024, voff[v], so);
  };
  __syncthreads();
  // transform: this thread's chunk and its coefficients
  const int tc = tid % CPR, trow = tid / CPR;
  float sc8[8], sh8[8], mu8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc8[e] = cf[8 * tc + e];
    sh8[e] = cf[C + 8 * tc + e];
    mu8[e] = cf[2 * C + 8 * tc + e];
  }
  f32x4 acc[FPW];  // fragments (I <= J) f = wid + NW i of G (gram_frag)
#pragma unroll
  for (int i = 0; i < FPW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 csa[FPW];  // column sums of block J for the wave's diagonal fragments (J, J): ones^T X'
#pragma unroll
  for (int i = 0; i < FPW; ++i) csa[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 ones = __builtin_bit_cast(bf16x8, u32x4{0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u});
  // operand read: lane (g, i = 4 q + p) takes rows 8 g + q (+ 4), channels 16 I + 4 p .. + 3
  const int g = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
  const int rw1 = 8 * g + qq, rw2 = rw1 + 4;
  const int ro1 = rw1 * RB, ro2 = rw2 * RB;
  const int h1 = 2 * gram_h(rw1, C), h2 = 2 * gram_h(rw2, C);

#pragma unroll 1
  for (int q = 0; q < NG - 1; ++q)
    if (q < ngrp) dma_group(q);
#pragma unroll 1
  for (int q = 0; q < ngrp; ++q) {
    // every DMA of groups <= q retired (younger: groups q + 1 .. q + NG - 2, all issued when they exist)
    if (q + NG - 2 < ngrp) gram_wait_vm<(NG - 2) * DPG>();
    else gram_wait_vm<0>();
    __syncthreads();  // group q landed for every wave; every wave is past group q - 1's operand reads
    if (q + NG - 1 < ngrp) dma_group(q + NG - 1);  // into group q - 1's slots
    char* const S = ring + (q % NG) * GT * SB;
    const bool full = r0 + (int64_t)(q + 1) * GT * TR <= r1;  // block-uniform
#pragma unroll
    for (int k = 0; k < TPG; ++k) {
      const int rg = trow + RPT * k, row = rg % TR;
      char* a = S + (rg / TR) * SB + row * RB + ((tc ^ (2 * gram_h(row, C))) << 4);
      float f[8];
      unpack8(*(const u32x4*)a, f);
      if (coef) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = fmaxf(fmaf(f[e], sc8[e], sh8[e]), 0.f);
        unpack8(pack8(f), f);  // the rounded operand
      }
      if (full) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] -= mu8[e];
      } else {
        const bool valid = r0 + (int64_t)q * GT * TR + rg < r1;
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = valid ? f[e] - mu8[e] : 0.f;  // (pad rows stay 0, not -mu)
      }
      *(u32x4*)a = pack8(f);  // the centred MFMA operand
    }
    __syncthreads();
    // the wave's fragments are compile-time per wave index: operands read once, only those it uses
    auto mm = [&](auto wc) {
      constexpr int W = decltype(wc)::value;
#pragma unroll
      for (int tk = 0; tk < GT; ++tk) {
        const char* T = S + tk * SB;
        bf16x8 op[NB];
        gram_sfor<NB>([&](auto Ic) {
          constexpr int I = decltype(Ic)::value;
          if constexpr (!gram_uses(W, I, NB, NF, NW, FPW)) return;
          const int ch = 2 * I + (pp >> 1), sub = (pp & 1) * 8;
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gram_lds4*)(T + ro1 + ((ch ^ h1) << 4) + sub));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gram_lds4*)(T + ro2 + ((ch ^ h2) << 4) + sub));
          s16x8 r;
          r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
          r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
          op[I] = __builtin_bit_cast(bf16x8, r);
        });
        gram_sfor<FPW>([&](auto ic) {
          constexpr int i = decltype(ic)::value;
          constexpr int f = gram_frag(W + NW * i, NB, NF);
          if constexpr (W + NW * i < NF) {
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(op[f >> 8], op[f & 255], acc[i], 0, 0, 0);
            if constexpr ((f >> 8) == (f & 255))
              csa[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, op[f & 255], csa[i], 0, 0, 0);
          }
        });
      }
    };
    switch (wid) {
      case 0: mm(std::integral_constant<int, 0>{}); break;
      case 1: mm(std::integral_constant<int, 1>{}); break;
      case 2: mm(std::integral_constant<int, 2>{}); break;
      case 3: mm(std::integral_constant<int, 3>{}); break;
      case 4: mm(std::integral_constant<int, 4>{}); break;
      case 5: mm(std::integral_constant<int, 5>{}); break;
      case 6: mm(std::integral_constant<int, 6>{}); break;
      default: mm(std::integral_constant<int, 7>{}); break;
    }
  }
  // partial G, upper-triangle fragments only, fragment-native: fragment f's element e of lane l at
  // [block][f][e][l] (whole 256-B rows per store; gram_reduce_tri_kernel mirrors); the column sums (every row
  // of ones^T X' is the same): row 0 = lanes 0..15, element 0
  float* Gt = gp + (int64_t)blockIdx.x * NF * 256;
  const int li = lane & 15;
#pragma unroll
  for (int i = 0; i < FPW; ++i) {
    const int fl = wid + NW * i;
    if (fl >= NF) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) Gt[(int64_t)fl * 256 + e * 64 + lane] = acc[i][e];
    const int f = gram_frag(fl, NB, NF);
    if ((f >> 8) == (f & 255) && g == 0) sp[(int64_t)blockIdx.x * C + 16 * (f & 255) + li] = csa[i][0];
  }
}

// Pilot shift of a plain operand (no producing BN whose coefficients relu_gauss_mean could work from: the
// block input x of a downsample conv): the per-channel mean of ns rows spread evenly over the M rows, written
// as the degenerate BN description [4][C] = (scale 1, shift 0, mean, invstd 0) -- sigma = 0, for which
// relu_gauss_mean returns max(mean, 0) rounded to its 5 significant bits.  Any mu within O(std) of the column
// mean removes the cancellation; a few hundred rows put the sample mean within a small fraction of one std.
// One block; the partial sums of a channel chunk are added in a fixed order (deterministic).
// (sh > 0: the M rows are the stride-2 subsample of an [*, sh, sw, C] image, as gram_dma_kernel's STR)
__global__ __launch_bounds__(256) void gram_pilot_kernel(const uint16_t* __restrict__ x, int64_t M, int C, int ns,
                                                         float* __restrict__ coef, int sh, int sw) {
  __shared__ float red[256][9];
  const int tid = threadIdx.x, cpr = C / 8, nr = 256 / cpr;  // C <= 256: nr >= 8 sample-row groups
  const int tc = tid % cpr, tr = tid / cpr;
  float a[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = 0.f;
#pragma unroll 4
  for (int i = tr; i < ns; i += nr) {
    int64_t row = (int64_t)i * M / ns;  // ns <= M: distinct rows < M
    if (sh > 0) row = gram_s2_pixel(row, sh, sw);
    float f[8];
    unpack8(*(const u32x4*)(x + row * C + 8 * tc), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += f[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[tid][e] = a[e];
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float t = 0.f;
    for (int r = 0; r < nr; ++r) t += red[r * cpr + (c >> 3)][c & 7];
    coef[c] = 1.f;
    coef[C + c] = 0.f;
    coef[2 * C + c] = t / (float)ns;
    coef[3 * C + c] = 0.f;
  }
}

// sum_b p[b * stride] over b = q, q + 8, ... < nb in that order (double): 32 (then 8) loads in flight per batch
__device__ __forceinline__ double gram_slab_sum(const float* __restrict__ p, int64_t stride, int q, int nb) {
  double a = 0.0;
  int b = q;
  for (; b + 248 < nb; b += 256) {
    float v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = p[(int64_t)(b + 8 * i) * stride];
#pragma unroll
    for (int i = 0; i < 32; ++i) a += v[i];
  }
  for (; b + 56 < nb; b += 64) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p[(int64_t)(b + 8 * i) * stride];
#pragma unroll
    for (int i = 0; i < 8; ++i) a += v[i];
  }
  for (; b < nb; b += 8) a += p[(int64_t)b * stride];
  return a;
}

// gram_reduce_kernel for the triangle layout of gram_dma_kernel: output j < NF * 256 is element e of lane l of
// fragment f (contiguous partial reads across the block), written to G at (r, c) and mirrored at (c, r); then
// the C column sums.  Same fixed order (8 slab groups, then group order, in double).
__global__ __launch_bounds__(256) void gram_reduce_tri_kernel(const float* __restrict__ gp, const float* __restrict__ sp,
                                                              int nb, int C, float* __restrict__ G, float* __restrict__ s) {
  __shared__ double part[8][32];
  const int o = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int NB = C / 16, NF = NB * (NB + 1) / 2;
  const int64_t nt = (int64_t)NF * 256;
  const int64_t j = (int64_t)blockIdx.x * 32 + o;
  double a = 0.0;
  if (j < nt) a = gram_slab_sum(gp + j, nt, q, nb);
  else if (j < nt + C) a = gram_slab_sum(sp + (j - nt), C, q, nb);
  part[q][o] = a;
  __syncthreads();
  if (q == 0) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += part[k][o];
    if (j < nt) {
      const int fr = gram_frag((int)(j >> 8), NB, NF), I = fr >> 8, J = fr & 255;
      const int e = (int)((j >> 6) & 3), l = (int)(j & 63);
      const int r = 16 * I + 4 * (l >> 4) + e, c = 16 * J + (l & 15);
      G[(int64_t)r * C + c] = (float)t;
      if (I != J) G[(int64_t)c * C + r] = (float)t;
    } else if (j < nt + C) {
      s[j - nt] = (float)t;
    }
  }
}

// G[i] = sum_b gp[b][i] (i over C*C, then the C column sums), in a fixed order, in double.  A block
// covers 32 consecutive outputs with 8 slab groups (thread = output x group: group q sums blocks
// q, q + 8, ...), then the 8 group sums are added in group order.
__global__ __launch_bounds__(256) void gram_reduce_kernel(const float* __restrict__ gp, const float* __restrict__ sp, int nb,
                                                          int C, float* __restrict__ G, float* __restrict__ s) {
  __shared__ double part[8][32];
  const int o = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int64_t i = (int64_t)blockIdx.x * 32 + o;
  const int64_t cc = (int64_t)C * C;
  double a = 0.0;
  if (i < cc) a = gram_slab_sum(gp + i, cc, q, nb);
  else if (i < cc + C) a = gram_slab_sum(sp + (i - cc), C, q, nb);
  part[q][o] = a;
  __syncthreads();
  if (q == 0) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += part[k][o];
    if (i < cc) G[i] = (float)t;
    else if (i < cc + C) s[i - cc] = (float)t;
  }
}

// Small fp32 GEMM on 32x32 output tiles: out[m][n] = sum_k A(m, k) B[k][n].
//   AT = false: A(m, k) = a[m * lda + k]        (row-major, u = W G: A = W3 [Cout][Cin] bf16)
//   AT = true:  A(m, k) = a[k * lda + m] scale[k] (Q = W^T diag(b) W: A = W3 read down its columns)
// K chunks of KC staged in LDS as fp32 (KC = the whole K slice at the shapes used: one memory round trip),
// any next chunk's loads in flight (registers) during the current chunk's FMAs; 256 threads, each 1 row x 4
// columns of the tile.  A row-major A is read along k (coalesced).
// AT with ecoef: the blocks of tile row 0 also form eout[z][n] = sum_{k in slice z} ecoef[k] B[k][n] (the data
// grad's bias c^T W from the staged B rows: 8 k groups per column, then the groups in order).
template <bool AT, typename TB, int KC>
__global__ __launch_bounds__(256) void gram_mm_kernel(const uint16_t* __restrict__ a, int64_t lda,
                                                      const float* __restrict__ scale, const TB* __restrict__ b,
                                                      int64_t ldb, int K, int kslice, float* __restrict__ out,
                                                      int64_t ldo, int64_t slab, const float* __restrict__ ecoef,
                                                      float* __restrict__ eout) {
  // blockIdx.z: K slice [z * kslice, +kslice) -> out + z * slab (partials summed by the caller, in order)
  constexpr int NE = KC / 8, GK = KC / 8;  // elements per thread per operand; k per e group
  __shared__ float As[KC][33], Bs[KC][32], Es[KC];
  __shared__ float ep[8][32];
  const int tid = threadIdx.x, m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  const int tm = tid >> 3, tn = (tid & 7) * 4;
  const int kb = blockIdx.z * kslice, ke = min(K, kb + kslice);
  const bool doe = AT && ecoef != nullptr && blockIdx.y == 0;
  out += (int64_t)blockIdx.z * slab;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  // raw operands in flight: loads are unconditional (k clamped into the slice) so a chunk's are all
  // outstanding together; conversion, scaling and the k < ke mask happen at the LDS store
  uint16_t ra[NE];
  TB rb[NE];
  float rs[NE], rc = 0.f, re = 0.f;
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + 256 * i;
      const int kB = min(k0 + (e >> 5), ke - 1), c = e & 31;
      rb[i] = b[(int64_t)kB * ldb + n0 + c];
      if constexpr (AT) {
        ra[i] = a[(int64_t)kB * lda + m0 + c];
        rs[i] = scale ? scale[kB] : 1.f;
      } else {
        ra[i] = a[(int64_t)(m0 + e / KC) * lda + min(k0 + e % KC, ke - 1)];
      }
    }
    if (doe) rc = ecoef[min(k0 + (tid % KC), ke - 1)];
  };
  auto tof = [](TB v) -> float {
    if constexpr (sizeof(TB) == 2) return bf2f((uint16_t)v);
    else return (float)v;
  };
  load(kb);
  for (int k0 = kb; k0 < ke; k0 += KC) {
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + 256 * i;
      const bool kv = k0 + (e >> 5) < ke;
      Bs[e >> 5][e & 31] = kv ? tof(rb[i]) : 0.f;
      if constexpr (AT) As[e >> 5][e & 31] = kv ? bf2f(ra[i]) * rs[i] : 0.f;
      else As[e % KC][e / KC] = k0 + e % KC < ke ? bf2f(ra[i]) : 0.f;
    }
    if (doe && tid < KC) Es[tid] = k0 + tid < ke ? rc : 0.f;
    __syncthreads();
    if (k0 + KC < ke) load(k0 + KC);
    const int kn = min(KC, ke - k0);  // (a multiple of 8: K % 32 == 0)
#pragma unroll 8
    for (int kk = 0; kk < kn; ++kk) {
      const float av = As[kk][tm];
      const f32x4 bv = *(const f32x4*)&Bs[kk][tn];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(av, bv[e], acc[e]);
    }
    if (doe) {
      const int o = tid & 31, q = tid >> 5;
#pragma unroll
      for (int u = 0; u < GK; ++u)
        if (GK * q + u < kn) re = fmaf(Es[GK * q + u], Bs[GK * q + u][o], re);
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) out[(int64_t)(m0 + tm) * ldo + n0 + tn + e] = acc[e];
  if (doe) {
    const int o = tid & 31, q = tid >> 5;
    ep[q][o] = re;
    __syncthreads();
    if (q == 0) {
      float t = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) t += ep[g][o];
      eout[(int64_t)blockIdx.z * ldo + n0 + o] = t;
    }
  }
}

// Forward: per output channel k of conv3 (weights w [Cout][Cin] bf16, u = W G from gram_mm_kernel, G and
// s = s[0 .. Cin) centred on mu = s[Cin .. 2 Cin)):
//   ms = (w_k . s) / M,  mean = w_k . mu + ms,  var = (w_k . u[k]) / M - ms^2   (no cancellation: ms ~ 0)
//   -> coef [4][Cout] = scale, shift, mean, invstd (the layout of bn_finalize_kernel), running stats
// updated as there (unbiased variance).  One wave per k.
__global__ __launch_bounds__(256) void gram_coef_kernel(const float* __restrict__ u, const float* __restrict__ s,
                                                        const uint16_t* __restrict__ w, int Cin, int Cout, int64_t M,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float* __restrict__ rmean, float* __restrict__ rvar, float momentum,
                                                        float eps, float* __restrict__ coef) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= Cout) return;
  // Cin <= 256 (the Gram pass's C): every lane's <= 4 columns and the channel's scalars loaded up front,
  // unconditionally (clamped, masked after), so they are all in flight at once
  const int jl = min(lane, Cin - 1);
  const float gm = gamma ? gamma[k] : 1.f, bt = beta ? beta[k] : 0.f;
  const float rm0 = rmean ? rmean[k] : 0.f, rv0 = rmean ? rvar[k] : 0.f;
  uint16_t wr[4];
  float ur[4], sr[4], mr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = min(jl + 64 * i, Cin - 1);
    wr[i] = w[(int64_t)k * Cin + j];
    ur[i] = u[(int64_t)k * Cin + j];
    sr[i] = s[j];
    mr[i] = s[Cin + j];
  }
  double e2 = 0.0, ws = 0.0, wm = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (lane + 64 * i >= Cin) continue;
    const double wv = bf2f(wr[i]);
    e2 += wv * ur[i];
    ws += wv * sr[i];
    wm += wv * mr[i];
  }
  for (int o = 32; o > 0; o >>= 1) {
    e2 += __shfl_xor(e2, o, 64);
    ws += __shfl_xor(ws, o, 64);
    wm += __shfl_xor(wm, o, 64);
  }
  if (lane != 0) return;
  const double ms = ws / (double)M;
  const double mean = wm + ms;
  double var = e2 / (double)M - ms * ms;
  if (var < 0) var = 0;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = gm * invstd;
  coef[k] = sc;
  coef[Cout + k] = bt - (float)mean * sc;
  coef[2 * Cout + k] = (float)mean;
  coef[3 * Cout + k] = invstd;
  if (rmean) {
    const double unbiased = M > 1 ? var * (double)M / (double)(M - 1) : var;
    rmean[k] = (1.f - momentum) * rm0 + momentum * (float)mean;
    rvar[k] = (1.f - momentum) * rv0 + momentum * (float)unbiased;
  }
}

constexpr int KPB = 8;  // output channels per block of the backward coefficient kernel

// Backward, per output channel k.  part [2][Cout][RG]: row 0 = partial sums of dz3 (row 1 unused);
// P [Cout][Cin] = dz3^T a2 (uncentred: the weight-grad GEMM); G, u = W3 G and s centred on mu (gram_partial);
// coef3 = BN3's (scale, shift, mean, invstd).  With a' = a2 - mu, h = h' + w_k . mu (h' = w_k . a'):
//   Sdz = sum dz,  w_k . P'[k] = w_k . P[k] - Sdz (w_k . mu)  (P' = dz^T a'),  ms = w_k . s / M  (centred mean, ~0)
//   Sdzx = invstd sum dz (h - mean) = invstd (w_k . P'[k] - Sdz ms)
//   dgamma += Sdzx, dbeta += Sdz;  a = gamma invstd, b = -a invstd Sdzx / M, c = -a Sdz / M - b mean
//   dW3[k] += sum dh a2 = sum dh a' (sum dh = 0) = a P'[k] + b u[k] + (-a Sdz / M - b ms) s
//   bcat[k][:] = bf16(a w_k)                              (the data grad's B rows 0 .. Cout-1)
//   abc [3][Cout] = (a, b, c) for the Q GEMM and the bias
// Every term is formed in double from exact products: no E[h^2] - mean^2 style cancellation (w_k . P and
// Sdz w_k . mu cancel only down to P' itself, at double's 1e-16).  Cin <= 256: thread j owns column j of the
// block's KPB channels.  Every operand is loaded up front (one memory round trip), the 4 KPB dot products
// and sums reduce in one LDS pass (thread (value, group) sums 32 partials in order, then 8 groups by xor).
__global__ __launch_bounds__(256) void gram_bwd_kernel(const float* __restrict__ part, int rg, const float* __restrict__ P,
                                                       const uint16_t* __restrict__ w, const float* __restrict__ u,
                                                       const float* __restrict__ s, const float* __restrict__ coef3,
                                                       const float* __restrict__ gamma, int Cin, int Cout, int64_t M,
                                                       float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                       float* __restrict__ dw, uint16_t* __restrict__ bcat,
                                                       float* __restrict__ abc) {
  constexpr int NV = 4 * KPB;  // Sdz, w.P, w.mu, w.s per channel
  __shared__ double red[NV][8][33];
  __shared__ double tot[NV];
  __shared__ float kc[KPB][4];  // A, B, the s coefficient, Sdz
  const int k0 = blockIdx.x * KPB, tid = threadIdx.x, j = tid;
  const bool jv = j < Cin;
  // every load unconditional (indices clamped in range, masked after): all in flight at once
  const int jc = min(j, Cin - 1);
  float wv[KPB], pv[KPB], uv[KPB], dwv[KPB], sp[KPB];
  uint16_t wr[KPB];
  const float muj0 = s[Cin + jc], sj0 = s[jc];
  const int qc = min(tid, rg - 1);
#pragma unroll
  for (int kk = 0; kk < KPB; ++kk) {
    const int64_t o = (int64_t)min(k0 + kk, Cout - 1) * Cin + jc;
    wr[kk] = w[o];
    pv[kk] = P[o];
    uv[kk] = u[o];
    dwv[kk] = dw[o];
    sp[kk] = part[(int64_t)min(k0 + kk, Cout - 1) * rg + qc];
  }
  const int kt = k0 + tid, ktc = min(k0 + (tid & (KPB - 1)), Cout - 1);
  const float cmean = coef3[2 * Cout + ktc], cinv = coef3[3 * Cout + ktc];
  const float cgm = gamma ? gamma[ktc] : 1.f, cdg = dgamma ? dgamma[ktc] : 0.f, cdb = dbeta ? dbeta[ktc] : 0.f;
  const float muj = jv ? muj0 : 0.f, sj = jv ? sj0 : 0.f;
#pragma unroll
  for (int kk = 0; kk < KPB; ++kk) {
    const bool ok = jv && k0 + kk < Cout;
    wv[kk] = ok ? bf2f(wr[kk]) : 0.f;
    pv[kk] = ok ? pv[kk] : 0.f;
    if (k0 + kk >= Cout || tid >= rg) sp[kk] = 0.f;
  }
#pragma unroll
  for (int kk = 0; kk < KPB; ++kk) {
    double sd = sp[kk];
    if (k0 + kk < Cout)
      for (int q = tid + 256; q < rg; q += 256) sd += part[(int64_t)(k0 + kk) * rg + q];
    const double wd = wv[kk];
    red[kk][tid >> 5][tid & 31] = sd;
    red[KPB + kk][tid >> 5][tid & 31] = wd * pv[kk];
    red[2 * KPB + kk][tid >> 5][tid & 31] = wd * muj;
    red[3 * KPB + kk][tid >> 5][tid & 31] = wd * sj;
  }
  __syncthreads();
  {
    const int v = tid >> 3, g = tid & 7;
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 32; ++i) t += red[v][g][i];
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) t += __shfl_xor(t, o, 64);
    if (g == 0) tot[v] = t;
  }
  __syncthreads();
  if (tid < KPB) {
    double A = 0.0, B = 0.0, Cs = 0.0, Sdz = 0.0;
    if (kt < Cout) {
      Sdz = tot[tid];
      const double Sdzh = tot[KPB + tid] - Sdz * tot[2 * KPB + tid];
      const double ms = tot[3 * KPB + tid] / (double)M;
      const double mean = cmean, invstd = cinv;
      const double Sdzx = invstd * (Sdzh - Sdz * ms);
      if (dgamma) dgamma[kt] = cdg + (float)Sdzx;
      if (dbeta) dbeta[kt] = cdb + (float)Sdz;
      A = (double)cgm * invstd;
      B = -A * invstd * Sdzx / (double)M;
      const double Cc = -A * Sdz / (double)M - B * mean;
      Cs = -A * Sdz / (double)M - B * ms;
      abc[kt] = (float)A;
      abc[Cout + kt] = (float)B;
      abc[2 * Cout + kt] = (float)Cc;
    }
    kc[tid][0] = (float)A; kc[tid][1] = (float)B; kc[tid][2] = (float)Cs; kc[tid][3] = (float)Sdz;
  }
  __syncthreads();
#pragma unroll
  for (int kk = 0; kk < KPB; ++kk) {
    const int k = k0 + kk;
    if (!jv || k >= Cout) continue;
    const float A = kc[kk][0], B = kc[kk][1], Cs = kc[kk][2], Sdz = kc[kk][3];
    const int64_t o = (int64_t)k * Cin + j;
    const float pc = fmaf(-Sdz, muj, pv[kk]);  // P' = dz^T (a2 - mu)
    dw[o] = dwv[kk] + fmaf(A, pc, fmaf(B, uv[kk], Cs * sj));
    bcat[o] = f2bf(A * wv[kk]);
  }
}

// Backward: the bf16 cast of Q (gram_mm_kernel's K-slice partials, fp32, summed in slice order) into the B
// rows Cout + j', and (the last block) the data grad's bias e[j] = sum_k c_k W3[k][j] from gram_mm_kernel's
// per-slice partials, in slice order.
__global__ __launch_bounds__(256) void gram_e_kernel(int Cin, int Cout, const float* __restrict__ Q, int qslices,
                                                     const float* __restrict__ ep, uint16_t* __restrict__ bcat,
                                                     float* __restrict__ ebias) {
  const int64_t n = (int64_t)Cin * Cin, slab = n;
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i < n) {
    float4 v[8];
    const int z0 = min(qslices, 8);
#pragma unroll
    for (int z = 0; z < 8; ++z)
      if (z < z0) v[z] = *(const float4*)(Q + z * slab + i);
    float4 acc = v[0];
#pragma unroll
    for (int z = 1; z < 8; ++z)
      if (z < z0) { acc.x += v[z].x; acc.y += v[z].y; acc.z += v[z].z; acc.w += v[z].w; }
    for (int z = 8; z < qslices; ++z) {
      const float4 t = *(const float4*)(Q + z * slab + i);
      acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
    }
    uint16_t* dst = bcat + (int64_t)Cout * Cin + i;
    *(uint2*)dst = make_uint2(pack_bf2(acc.x, acc.y), pack_bf2(acc.z, acc.w));
  }
  if (blockIdx.x == gridDim.x - 1) {
    for (int jj = threadIdx.x; jj < Cin; jj += 256) {
      float t = 0.f;
      for (int z = 0; z < qslices; ++z) t += ep[(int64_t)z * Cin + jj];
      ebias[jj] = t;
    }
  }
}

}  // namespace gram
}  // namespace dpe

using namespace dpe;

// Gram pass: x [M][C] bf16 (C in {64, 128, 256}), coef = BN [scale | shift] applied with ReLU on load (or
// nullptr), scoef = the [4][C] BN coefficients the pilot shift comes from (nullptr: no shift);
// ws >= dpe_gram_ws_floats(M, C) floats.  Writes G [C][C] and s [2][C] = (colsum, mu), centred on mu.
static bool gram_dma_on() {
  const char* ev = getenv("DPE_GRAM_DMA");  // (read per call: tests compare both kernels in one process)
  return !(ev && ev[0] == '0');
}
extern "C" int dpe_gram_blocks(int64_t M, int C) {
  // (the LDS-DMA pass keeps 256 blocks at C = 256 too: its triangle partials are half the full matrices)
  const int nb = (C <= 128 || gram_dma_on()) ? 256 : 128;
  return (int)std::min<int64_t>(nb, std::max<int64_t>(1, (M + gram::TR - 1) / gram::TR));
}
extern "C" int64_t dpe_gram_ws_floats(int64_t M, int C) { return (int64_t)dpe_gram_blocks(M, C) * ((int64_t)C * C + C); }

// sh, sw > 0: x is an [*, sh, sw, C] image and the M rows are its stride-2 subsample (LDS-DMA kernel only)
extern "C" int dpe_gram(const uint16_t* x, const float* coef, const float* scoef, int64_t M, int C, float* ws, float* G,
                        float* s, hipStream_t st, int sh, int sw) {
  if (C != 64 && C != 128 && C != 256) return -1;
  const bool str = sh > 0;
  if (str && (sh % 2 || sw % 2 || sw <= 0 || M % ((int64_t)(sh / 2) * (sw / 2)))) return -1;
  const int nb = dpe_gram_blocks(M, C);
  const int64_t tiles = (M + gram::TR - 1) / gram::TR;
  const int rpb = (int)(((tiles + nb - 1) / nb) * gram::TR);
  float* gp = ws;
  float* sp = ws + (int64_t)nb * C * C;
  float* mu = s + C;
  // DPE_GRAM_DMA=0: the register-staged kernel (A/B)
  const bool dma = gram_dma_on();
  const bool dma_used = dma && (str ? 4 : 1) * M * C * 2 < (1ll << 31) - 4096;
  if (str && !dma_used) return -1;
  if (str) {
    if (C == 64)
      hipLaunchKernelGGL((gram::gram_dma_kernel<64, true>), dim3(nb), dim3(512), 0, st, x, coef, scoef, M, rpb, gp, sp, mu, sh, sw);
    else if (C == 128)
      hipLaunchKernelGGL((gram::gram_dma_kernel<128, true>), dim3(nb), dim3(512), 0, st, x, coef, scoef, M, rpb, gp, sp, mu, sh, sw);
    else
      hipLaunchKernelGGL((gram::gram_dma_kernel<256, true>), dim3(nb), dim3(512), 0, st, x, coef, scoef, M, rpb, gp, sp, mu, sh, sw);
  } else if (dma_used) {
    if (C == 64)
      hipLaunchKernelGGL(gram::gram_dma_kernel<64>, dim3(nb), dim3(512), 0, st, x, coef, scoef, M, rpb, gp, sp, mu, 0, 0);
    else if (C == 128)
      hipLaunchKernelGGL(gram::gram_dma_kernel<128>, dim3(nb), dim3(512), 0, st, x, coef, scoef, M, rpb, gp, sp, mu, 0, 0);
    else
      hipLaunchKernelGGL(gram::gram_dma_kernel<256>, dim3(nb), dim3(512), 0, st, x, coef, scoef, M, rpb, gp, sp, mu, 0, 0);
  } else if (C == 64)
    hipLaunchKernelGGL(gram::gram_partial_kernel<64>, dim3(nb), dim3(256), 0, st, x, coef, scoef, M, rpb, gp, sp, mu);
  else if (C == 128)
    hipLaunchKernelGGL(gram::gram_partial_kernel<128>, dim3(nb), dim3(256), 0, st, x, coef, scoef, M, rpb, gp, sp, mu);
  else
    hipLaunchKernelGGL(gram::gram_partial_kernel<256>, dim3(nb), dim3(512), 0, st, x, coef, scoef, M, rpb, gp, sp, mu);
  const int64_t n = (int64_t)C * C + C;
  if (dma_used || str) {
    const int64_t nf = (int64_t)(C / 16) * (C / 16 + 1) / 2, nt = nf * 256 + C;
    hipLaunchKernelGGL(gram::gram_reduce_tri_kernel, dim3((unsigned)((nt + 31) / 32)), dim3(256), 0, st, gp, sp, nb, C, G, s);
  }
  else
    hipLaunchKernelGGL(gram::gram_reduce_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, st, gp, sp, nb, C, G, s);
  return 0;
}

// Pilot shift for dpe_gram's scoef from a sample of x's rows (x has no producing BN): coef [4][C]
extern "C" int dpe_gram_pilot(const uint16_t* x, int64_t M, int C, float* coef, hipStream_t st, int sh, int sw) {
  if ((C != 64 && C != 128 && C != 256) || M <= 0) return -1;
  if (sh > 0 && (sh % 2 || sw % 2 || sw <= 0 || M % ((int64_t)(sh / 2) * (sw / 2)))) return -1;
  const int ns = (int)std::min<int64_t>(M, 512);
  hipLaunchKernelGGL(gram::gram_pilot_kernel, dim3(1), dim3(256), 0, st, x, M, C, ns, coef, sh, sw);
  return 0;
}

// u = W G  (M = Cout, N = Cin, K = Cin) alone: no BN coefficients, no running statistics touched
extern "C" int dpe_gram_u(const float* G, const uint16_t* w, int Cin, int Cout, float* u, hipStream_t st) {
  if (Cin % 32 || Cout % 32 || Cin > 256) return -1;
  hipLaunchKernelGGL((gram::gram_mm_kernel<false, float, 256>), dim3(Cin / 32, Cout / 32, 1), dim3(256), 0, st, w,
                     (int64_t)Cin, (const float*)nullptr, G, (int64_t)Cin, Cin, Cin, u, (int64_t)Cin, (int64_t)0,
                     (const float*)nullptr, (float*)nullptr);
  return 0;
}

extern "C" int dpe_gram_coef(const float* G, const float* s, const uint16_t* w, int Cin, int Cout, int64_t M,
                             const float* gamma, const float* beta, float* rmean, float* rvar, float momentum, float eps,
                             float* coef, float* u, hipStream_t st) {
  if (dpe_gram_u(G, w, Cin, Cout, u, st) != 0) return -1;
  hipLaunchKernelGGL(gram::gram_coef_kernel, dim3((Cout + 3) / 4), dim3(256), 0, st, u, s, w, Cin, Cout, M, gamma, beta,
                     rmean, rvar, momentum, eps, coef);
  return 0;
}

// qws (the caller's scratch) >= dpe_gram_bwd_ws_floats(Cin, Cout): Q's K-slice partials before the bf16 cast,
// then the bias's per-slice partials
extern "C" int64_t dpe_gram_bwd_ws_floats(int Cin, int Cout) {
  return (int64_t)((Cout + 127) / 128) * ((int64_t)Cin * Cin + Cin);
}
extern "C" int dpe_gram_bwd(const float* part, int rg, const float* P, const uint16_t* w, const float* u, const float* s,
                            const float* coef3, const float* gamma, int Cin, int Cout, int64_t M, float* dgamma,
                            float* dbeta, float* dw, uint16_t* bcat, float* abc, float* ebias, float* qws, hipStream_t st) {
  if (Cin % 32 || Cout % 32 || Cin > 256) return -1;
  const unsigned nb = (unsigned)((Cout + gram::KPB - 1) / gram::KPB);
  hipLaunchKernelGGL(gram::gram_bwd_kernel, dim3(nb), dim3(256), 0, st, part, rg, P, w, u, s, coef3, gamma, Cin, Cout, M,
                     dgamma, dbeta, dw, bcat, abc);
  // Q = W^T diag(b) W  (M = N = Cin, K = Cout; A = W read down its columns, scaled by b = abc row 1), and the
  // bias partials c^T W from tile row 0 (c = abc row 2)
  // (split over K = Cout in 128-deep slices: the 32x32-tile grid alone is 4-64 blocks)
  const int qs = (Cout + 127) / 128;
  float* ep = qws + (int64_t)qs * Cin * Cin;
  hipLaunchKernelGGL((gram::gram_mm_kernel<true, uint16_t, 128>), dim3(Cin / 32, Cin / 32, qs), dim3(256), 0, st, w,
                     (int64_t)Cin, abc + Cout, w, (int64_t)Cin, Cout, 128, qws, (int64_t)Cin, (int64_t)Cin * Cin,
                     abc + 2 * Cout, ep);
  const int ncast = (int)(((int64_t)Cin * Cin + 1023) / 1024);
  hipLaunchKernelGGL(gram::gram_e_kernel, dim3(ncast), dim3(256), 0, st, Cin, Cout, qws, qs, ep, bcat, ebias);
  return 0;
}
