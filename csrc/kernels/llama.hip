// The three elementwise / row kernels of a Llama-style decoder block beside the GQA flash attention of attn.hip:
// rotary position embedding on the packed qkv rows, RMSNorm forward / backward, SwiGLU forward / backward.
// House rules of norm.hip and eltwise.hip: 16-B lanes, every load of a step issued up front and unconditional,
// a tail lane clamped onto the last chunk (same loads, same stored bytes as its owner, its share of any sum
// masked), output forms chosen at compile time, no atomics, fp32 arithmetic and one RNE rounding at a bf16 store.
//
// RoPE.  A head is 64 bf16 = 8 chunks of 16 B.  One lane owns chunk j < 4 of a head together with chunk j + 4, so
// both halves of each rotated pair (i, i + 32) sit in one lane: the in-place form needs no synchronisation.
// 16 lanes serve one token -- 4 heads side by side, 4 lanes each -- and walk the token's heads in steps of 4 with
// the lane's 8 cos and 8 sin values, loaded once per token, in registers: the table is read per token, not per
// head, and a 16-lane group touches 512 contiguous bytes per step.  Two steps' loads are in flight at once.  A
// head past the last one is clamped onto the last head, which the same wave owns in the same trip of the loop:
// owner and copy execute the same load and then the same store instruction, so also in place both see the
// unrotated values.  (Hence no __restrict__ on src / dst, and all four loads of a trip precede its stores.)
// No LDS.
//
// RMSNorm.  D <= 2048: one wave per row, the row in registers (at most 4 chunks per lane), the lean LayerNorm
// form without its mean pass.  D > 2048 (to 8192): one 256-thread block per row, at most 4 chunks per thread,
// the row sum reduced over the 4 waves through LDS (block_sum) -- x and dy are still read exactly once, which a
// column-sliced second pass (LayerNorm's wide backward) does not manage.  The backward walks rows per block and
// keeps the dw partial of its columns in registers: one [D] partial per block (the wave form adds its 4 waves'
// partials through LDS, the block form's threads own their columns outright), then a fixed-order column
// reduction adds the partials into dw, so dw is bitwise repeatable and is accumulated into like LayerNorm's.
//
// SwiGLU.  gu [M, 2F] = [gate | up] per row from one GEMM; u = silu(g) v.  Flat exact grid over the M F / 8
// output chunks, 2 chunks per thread one grid-stride apart (the fastest form of scripts/stream_probe.hip), the
// last threads' second chunk clamped onto the last one.  sigma = 1 / (1 + exp(-g)) with v_exp_f32 / v_rcp_f32: a
// saturated exponent gives exp = inf -> rcp = 0, or exp = 0 -> sigma = 1, never inf * 0.
#include "common.h"
#include "launch.h"

namespace dpe {

template <bool XBF>
DPE_DEVICE void ld8(const void* x, int64_t off, float* f) {
  if constexpr (XBF) {
    unpack8(*(const u32x4*)((const uint16_t*)x + off), f);
  } else {
    const f32x4 a = *(const f32x4*)((const float*)x + off), b = *(const f32x4*)((const float*)x + off + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[e] = a[e]; f[e + 4] = b[e]; }
  }
}
template <bool XBF>
DPE_DEVICE void st8(void* y, int64_t off, const float* o) {
  if constexpr (XBF) {
    *(u32x4*)((uint16_t*)y + off) = pack8(o);
  } else {
    *(f32x4*)((float*)y + off) = f32x4{o[0], o[1], o[2], o[3]};
    *(f32x4*)((float*)y + off + 4) = f32x4{o[4], o[5], o[6], o[7]};
  }
}

// ------------------------------------------------------------------- RoPE
// COPY = false: dst may be src; only the n_rot rotated heads are loaded and stored.  COPY = true (dst != src): all
// W heads are walked, the heads from n_rot on pass through as the bits they are.  sgn = -1: the inverse rotation.
template <bool COPY>
__global__ __launch_bounds__(256) void rope_kernel(const uint16_t* src, uint16_t* dst, const float* __restrict__ cs,
                                                   const float* __restrict__ sn, const int32_t* __restrict__ pos,
                                                   int64_t ntok, int T, int W, int n_rot, int P, float sgn) {
  const int64_t tok = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (tok >= ntok) return;  // (uniform over the 16 lanes of a token)
  const int hs = (threadIdx.x >> 2) & 3, j = threadIdx.x & 3;
  int p = pos ? pos[tok] : (int)(tok % T);
  p = min(max(p, 0), P - 1);  // a position chooses a table row, never an address
  float c[8], s[8];
  ld8<false>(cs, (int64_t)p * 32 + j * 8, c);
  ld8<false>(sn, (int64_t)p * 32 + j * 8, s);
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] *= sgn;
  const int NH = COPY ? W : n_rot;
  const uint16_t* sp = src + tok * W * 64 + j * 8;
  uint16_t* dp = dst + tok * W * 64 + j * 8;
  for (int h0 = 0; h0 < NH; h0 += 8) {
    int h[2];
    u32x4 lo[2], hi[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      h[u] = min(h0 + 4 * u + hs, NH - 1);
      lo[u] = *(const u32x4*)(sp + h[u] * 64);
      hi[u] = *(const u32x4*)(sp + h[u] * 64 + 32);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float a[8], b[8], oa[8], ob[8];
      unpack8(lo[u], a);
      unpack8(hi[u], b);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        oa[e] = a[e] * c[e] - b[e] * s[e];
        ob[e] = b[e] * c[e] + a[e] * s[e];
      }
      u32x4 ra = pack8(oa), rb = pack8(ob);
      if constexpr (COPY) {
        const bool rot = h[u] < n_rot;
        ra = rot ? ra : lo[u];
        rb = rot ? rb : hi[u];
      }
      *(u32x4*)(dp + h[u] * 64) = ra;
      *(u32x4*)(dp + h[u] * 64 + 32) = rb;
    }
  }
}

// ---------------------------------------------------------------- RMSNorm
// BLK = false: 4 rows per block, one wave each, chunk c = lane + 64 j.  BLK = true: one row per block,
// c = thread + 256 j.  NJ chunks per lane.
template <bool BLK>
DPE_DEVICE float row_sum(float v, float* sh) {
  if constexpr (BLK) return block_sum(v, sh);
  else return warp_sum(v);
}

template <bool XBF, int NJ, bool BLK>
__global__ __launch_bounds__(256) void rms_fwd_kernel(const void* __restrict__ x, const float* __restrict__ w,
                                                      uint16_t* __restrict__ y, float* __restrict__ rstd_out, int64_t rows,
                                                      int D, float eps) {
  __shared__ float sh[16];
  constexpr int TPR = BLK ? 256 : 64;
  const int t = BLK ? threadIdx.x : (threadIdx.x & 63);
  const int64_t row = BLK ? (int64_t)blockIdx.x : blockIdx.x * 4ll + (threadIdx.x >> 6);
  if (row >= rows) return;  // (wave-uniform; BLK: the grid is exact)
  const int CH = D >> 3;
  const int64_t base = row * D;
  float f[NJ][8], wv[NJ][8], m[NJ];
  int cc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = t + TPR * j;
    m[j] = c < CH ? 1.f : 0.f;
    cc[j] = min(c, CH - 1);
    ld8<XBF>(x, base + cc[j] * 8, f[j]);
    ld8<false>(w, cc[j] * 8, wv[j]);
  }
  __builtin_amdgcn_sched_barrier(0);
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += f[j][e] * f[j][e] * m[j];
  const float rstd = rsqrtf(row_sum<BLK>(ss, sh) / (float)D + eps);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f[j][e] * rstd * wv[j][e];
    *(u32x4*)(y + base + cc[j] * 8) = pack8(o);
  }
  if (t == 0) rstd_out[row] = rstd;
}

// dx = rstd (g - xh mean(g xh)), g = dy w, xh = x rstd, in x's dtype; part[block][D] = the block's rows' sum of dy xh.
template <bool XBF, int NJ, bool BLK>
__global__ __launch_bounds__(256) void rms_bwd_kernel(const uint16_t* __restrict__ dy, const void* __restrict__ x,
                                                      const float* __restrict__ w, const float* __restrict__ rstd_in,
                                                      void* __restrict__ dx, float* __restrict__ part, int64_t rows, int D) {
  __shared__ float sh[16];
  extern __shared__ float red[];  // !BLK: [4][D]
  constexpr int TPR = BLK ? 256 : 64;
  const int wid = threadIdx.x >> 6;
  const int t = BLK ? threadIdx.x : (threadIdx.x & 63);
  const int CH = D >> 3;
  int cc[NJ];
  float m[NJ], wv[NJ][8], pw[NJ][8];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = t + TPR * j;
    m[j] = c < CH ? 1.f : 0.f;
    cc[j] = min(c, CH - 1);
    ld8<false>(w, cc[j] * 8, wv[j]);
#pragma unroll
    for (int e = 0; e < 8; ++e) pw[j][e] = 0.f;
  }
  const int64_t row0 = BLK ? (int64_t)blockIdx.x : blockIdx.x * 4ll + wid;
  const int64_t step = BLK ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
  for (int64_t row = row0; row < rows; row += step) {  // (BLK: block-uniform, block_sum's barriers are met by all)
    const int64_t base = row * D;
    float dd[NJ][8], xh[NJ][8];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      unpack8(*(const u32x4*)(dy + base + cc[j] * 8), dd[j]);
      ld8<XBF>(x, base + cc[j] * 8, xh[j]);
    }
    const float rstd = rstd_in[row];
    __builtin_amdgcn_sched_barrier(0);  // one load round trip per row
    float sgx = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xh[j][e] *= rstd;
        const float dm = dd[j][e] * m[j];
        sgx += dm * wv[j][e] * xh[j][e];
        pw[j][e] += dm * xh[j][e];
      }
    sgx = row_sum<BLK>(sgx, sh) / (float)D;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = rstd * (dd[j][e] * wv[j][e] - xh[j][e] * sgx);
      st8<XBF>(dx, base + cc[j] * 8, o);
    }
  }
  float* pp = part + (int64_t)blockIdx.x * D;
  if constexpr (BLK) {  // every column has one owner thread
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (m[j] != 0.f) st8<false>(pp, cc[j] * 8, pw[j]);
  } else {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (m[j] != 0.f) st8<false>(red, wid * D + cc[j] * 8, pw[j]);
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += 256) pp[i] = (red[i] + red[D + i]) + (red[2 * D + i] + red[3 * D + i]);
  }
}

// dw[col] += the sum over the nb partial rows, in a fixed order: block = 16 columns x 64 row stripes (the shape of
// LayerNorm's finalize: 64-B row segments, 128 blocks at D = 2048), 4 independent accumulators per lane, then one
// thread per column adds the 64 stripes in order.
constexpr int RMF_C = 16, RMF_S = 64;
__global__ __launch_bounds__(RMF_C * RMF_S) void rms_bwd_finalize_kernel(const float* __restrict__ part, int nb, int D,
                                                                          float* __restrict__ dw) {
  __shared__ float red[RMF_S][RMF_C];
  const int cl = threadIdx.x % RMF_C, stripe = threadIdx.x / RMF_C;
  const int col = min((int)blockIdx.x * RMF_C + cl, D - 1);  // (D % 8 == 0: a clamped column only repeats a load)
  const float* src = part + col;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int k = stripe;
  for (; k + 3 * RMF_S < nb; k += 4 * RMF_S) {
    a0 += src[(int64_t)k * D];
    a1 += src[(int64_t)(k + RMF_S) * D];
    a2 += src[(int64_t)(k + 2 * RMF_S) * D];
    a3 += src[(int64_t)(k + 3 * RMF_S) * D];
  }
  for (; k < nb; k += RMF_S) a0 += src[(int64_t)k * D];
  red[stripe][cl] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (threadIdx.x < RMF_C && (int)blockIdx.x * RMF_C + cl < D) {
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < RMF_S; ++i) s += red[i][cl];
    dw[col] += s;
  }
}

// ----------------------------------------------------------------- SwiGLU
DPE_DEVICE float sigmoid_f(float g) { return __builtin_amdgcn_rcpf(1.f + __expf(-g)); }

// chunk i of the [M, F / 8] output chunks -> element offset of its gate chunk in gu (the up chunk: + F)
DPE_DEVICE int64_t gu_off(uint32_t i, uint32_t CH) {
  const uint32_t r = i / CH;
  return ((int64_t)r * 2 * CH + (i - r * CH)) * 8;
}

__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const uint16_t* __restrict__ gu, uint16_t* __restrict__ u,
                                                         uint32_t n, uint32_t CH) {
  const uint32_t i0 = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;  // n <= 2 * stride
  uint32_t i[2];
  u32x4 gr[2], vr[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    i[k] = min(i0 + k * stride, n - 1);
    const int64_t o = gu_off(i[k], CH);
    gr[k] = *(const u32x4*)(gu + o);
    vr[k] = *(const u32x4*)(gu + o + (int64_t)CH * 8);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float g[8], v[8], o[8];
    unpack8(gr[k], g);
    unpack8(vr[k], v);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = g[e] * sigmoid_f(g[e]) * v[e];
    *(u32x4*)(u + (int64_t)i[k] * 8) = pack8(o);
  }
}

// dg = du v sigma (1 + g (1 - sigma)), dv = du g sigma, both halves of dgu's row in the same pass
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const uint16_t* __restrict__ du, const uint16_t* __restrict__ gu,
                                                         uint16_t* __restrict__ dgu, uint32_t n, uint32_t CH) {
  const uint32_t i0 = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
  uint32_t i[2];
  int64_t off[2];
  u32x4 dr[2], gr[2], vr[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    i[k] = min(i0 + k * stride, n - 1);
    off[k] = gu_off(i[k], CH);
    dr[k] = *(const u32x4*)(du + (int64_t)i[k] * 8);
    gr[k] = *(const u32x4*)(gu + off[k]);
    vr[k] = *(const u32x4*)(gu + off[k] + (int64_t)CH * 8);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float d[8], g[8], v[8], og[8], ov[8];
    unpack8(dr[k], d);
    unpack8(gr[k], g);
    unpack8(vr[k], v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float sg = sigmoid_f(g[e]);
      og[e] = d[e] * v[e] * sg * (1.f + g[e] * (1.f - sg));
      ov[e] = d[e] * g[e] * sg;
    }
    *(u32x4*)(dgu + off[k]) = pack8(og);
    *(u32x4*)(dgu + off[k] + (int64_t)CH * 8) = pack8(ov);
  }
}

}  // namespace dpe

using namespace dpe;

extern "C" int dpe_rope(const uint16_t* src, uint16_t* dst, const float* cos, const float* sin, const int32_t* pos, int B,
                        int T, int W, int n_rot, int P, int inverse, hipStream_t st) {
  if (B < 1 || T < 1 || W < 1 || n_rot < 0 || n_rot > W || P < 1 || (!pos && T > P)) return -1;
  const int64_t ntok = (int64_t)B * T;
  const dim3 grid((unsigned)((ntok + 15) / 16));
  const float sgn = inverse ? -1.f : 1.f;
  if (dst != src) {
    hipLaunchKernelGGL(rope_kernel<true>, grid, dim3(256), 0, st, src, dst, cos, sin, pos, ntok, T, W, n_rot, P, sgn);
  } else if (n_rot > 0) {
    hipLaunchKernelGGL(rope_kernel<false>, grid, dim3(256), 0, st, src, dst, cos, sin, pos, ntok, T, W, n_rot, P, sgn);
  }
  return 0;
}

static bool rms_ok(int64_t rows, int D) { return rows >= 1 && D >= 8 && D <= 8192 && D % 8 == 0; }

// NJ_ chunks per lane; the wave form up to D = 2048 (256 chunks), the block form above
#define DPE_RMS_PICK(XB)                                                          \
  if (D <= 2048) {                                                                \
    const int nj = (D / 8 + 63) / 64;                                             \
    if (nj == 1) DPE_RMS_GO(XB, 1, false); else if (nj == 2) DPE_RMS_GO(XB, 2, false); \
    else if (nj == 3) DPE_RMS_GO(XB, 3, false); else DPE_RMS_GO(XB, 4, false);    \
  } else {                                                                        \
    const int nj = (D / 8 + 255) / 256;                                           \
    if (nj == 2) DPE_RMS_GO(XB, 2, true); else if (nj == 3) DPE_RMS_GO(XB, 3, true); \
    else DPE_RMS_GO(XB, 4, true);                                                 \
  }

extern "C" int dpe_rmsnorm_fwd(const void* x, int x_bf16, const float* w, uint16_t* y, float* rstd, int64_t rows, int D,
                               float eps, hipStream_t st) {
  if (!rms_ok(rows, D)) return -1;
  const dim3 grid((unsigned)(D <= 2048 ? (rows + 3) / 4 : rows));
#define DPE_RMS_GO(XB, NJ_, BLK_) \
  hipLaunchKernelGGL((rms_fwd_kernel<XB, NJ_, BLK_>), grid, dim3(256), 0, st, x, w, y, rstd, rows, D, eps)
  if (x_bf16) { DPE_RMS_PICK(true) } else { DPE_RMS_PICK(false) }
#undef DPE_RMS_GO
  return 0;
}

// Partial-sum blocks of the backward.  Wave form: LayerNorm's count, ~2 rows per wave up to 1024 blocks; block form:
// one row per block and trip, up to 1024 blocks.
extern "C" int dpe_rmsnorm_bwd_nblocks(int64_t rows, int D) {
  const int64_t nb = D <= 2048 ? (rows + 7) / 8 : rows;
  return (int)(nb < 1 ? 1 : (nb > 1024 ? 1024 : nb));
}

// Floats of the `part` scratch of dpe_rmsnorm_bwd: [nblocks][D].
extern "C" int64_t dpe_rmsnorm_bwd_scratch(int64_t rows, int D) { return (int64_t)dpe_rmsnorm_bwd_nblocks(rows, D) * D; }

extern "C" int dpe_rmsnorm_bwd(const uint16_t* dy, const void* x, int x_bf16, const float* w, const float* rstd, void* dx,
                               float* dw, float* part, int64_t rows, int D, hipStream_t st) {
  if (!rms_ok(rows, D)) return -1;
  const int nb = dpe_rmsnorm_bwd_nblocks(rows, D);
  const size_t lds = D <= 2048 ? (size_t)4 * D * sizeof(float) : 0;
#define DPE_RMS_GO(XB, NJ_, BLK_) \
  hipLaunchKernelGGL((rms_bwd_kernel<XB, NJ_, BLK_>), dim3(nb), dim3(256), lds, st, dy, x, w, rstd, dx, part, rows, D)
  if (x_bf16) { DPE_RMS_PICK(true) } else { DPE_RMS_PICK(false) }
#undef DPE_RMS_GO
  hipLaunchKernelGGL(rms_bwd_finalize_kernel, dim3((D + RMF_C - 1) / RMF_C), dim3(RMF_C * RMF_S), 0, st, part, nb, D, dw);
  return 0;
}
#undef DPE_RMS_PICK

// n = M F / 8 output chunks, below 2^31 (the kernels index chunks in 32 bits); exact grid, 2 chunks per thread
static int swiglu_grid(int64_t M, int F, uint32_t* n) {
  if (M < 1 || F < 8 || F % 8) return -1;
  const int64_t n64 = M * (F / 8);
  if (n64 >= (1ll << 31)) return -1;
  *n = (uint32_t)n64;
  return (int)((n64 + 511) / 512);
}

extern "C" int dpe_swiglu_fwd(const uint16_t* gu, uint16_t* u, int64_t M, int F, hipStream_t st) {
  uint32_t n;
  const int g = swiglu_grid(M, F, &n);
  if (g < 0) return -1;
  hipLaunchKernelGGL(swiglu_fwd_kernel, dim3(g), dim3(256), 0, st, gu, u, n, (uint32_t)(F / 8));
  return 0;
}

extern "C" int dpe_swiglu_bwd(const uint16_t* du, const uint16_t* gu, uint16_t* dgu, int64_t M, int F, hipStream_t st) {
  uint32_t n;
  const int g = swiglu_grid(M, F, &n);
  if (g < 0) return -1;
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3(g), dim3(256), 0, st, du, gu, dgu, n, (uint32_t)(F / 8));
  return 0;
}
