// GPT-2 generation kernels for gfx950: one decode step is bound by bytes (every weight and the KV cache are read
// once per token) and by launch count, not by FLOPs -- none of the training tiles fit it.
//
//   attn_decode    one query per (batch row, head) against a head-major bf16 KV cache, keys split over S workgroups
//   linear_skinny  y[M, N] = x[M, K] w[N, K]^T for M <= 16: weights straight from global memory into MFMA B fragments
//   sample_logits  temperature / top-k / top-p / Gumbel-max draw of one token per row, the row held in registers
//
// No kernel here uses atomics: every reduction has a fixed order, so the same inputs give the same bits.
#include "common.h"
#include "launch.h"

namespace {

constexpr float L2E = 1.4426950408889634f;
constexpr float NEG_INF = -INFINITY;

// ===================================================================== attn_decode
// Block = 256 threads = 32 groups of 8 lanes; a group takes one key at a time (lane p of the group holds dims
// 8p .. 8p+7: one 16-byte load of K and one of V per key), keys j0 + g, j0 + g + 32, ...  Each group keeps an
// online-softmax state (m, l, o[8 per lane]) in fp32; the 32 states are merged through LDS in group order.
// Key len[b] is the step's own K/V row, read from qkv_step; keys past it are never loaded (the loads of a
// group's out-of-range slots are pointed at the step's row and their values are never used).
constexpr int AD_NT = 256, AD_G = AD_NT / 8, AD_U = 4;
constexpr int AD_PART = 66;  // floats per partial: m, l, o[64]

DPE_DEVICE int clamp_len(int len, int Tmax) { return len < 0 ? 0 : (len > Tmax - 1 ? Tmax - 1 : len); }

DPE_DEVICE void split_range(int n, int S, int s, int& j0, int& j1) {
  const int chunk = (n + S - 1) / S;
  j0 = s * chunk;
  j1 = j0 + chunk < n ? j0 + chunk : n;
  if (j0 > n) j0 = n;
}

__global__ __launch_bounds__(AD_NT) void attn_decode_kernel(const uint16_t* __restrict__ qkv, uint16_t* kc, uint16_t* vc,
                                                            const int32_t* __restrict__ lens, int H, int Tmax, int S,
                                                            float scale, float* __restrict__ ws, uint16_t* __restrict__ out) {
  __shared__ float sm[AD_G], sl[AD_G], so[AD_G][64];
  const int bh = blockIdx.y, s = blockIdx.x, b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, g = tid >> 3, p = tid & 7;
  const int len = clamp_len(lens[b], Tmax);
  const uint16_t* qs = qkv + ((int64_t)(b * 3 + 0) * H + h) * 64;
  const uint16_t* ks = qkv + ((int64_t)(b * 3 + 1) * H + h) * 64;
  const uint16_t* vs = qkv + ((int64_t)(b * 3 + 2) * H + h) * 64;
  uint16_t* kcb = kc + (int64_t)bh * Tmax * 64;
  uint16_t* vcb = vc + (int64_t)bh * Tmax * 64;
  if (s == 0 && tid < 16) {  // the one store of the step's K/V row (no workgroup reads row len of the cache)
    const uint16_t* src = (tid < 8 ? ks : vs) + (tid & 7) * 8;
    uint16_t* dst = (tid < 8 ? kcb : vcb) + (int64_t)len * 64 + (tid & 7) * 8;
    *(u32x4*)dst = *(const u32x4*)src;
  }
  float q[8];
  unpack8(*(const u32x4*)(qs + p * 8), q);
  int j0, j1;
  split_range(len + 1, S, s, j0, j1);
  float m = NEG_INF, l = 0.f, o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  for (int jb = j0 + g; jb < j1; jb += AD_G * AD_U) {
    u32x4 kr[AD_U], vr[AD_U];
#pragma unroll
    for (int u = 0; u < AD_U; ++u) {
      const int j = jb + u * AD_G;
      const bool own = j >= len;  // the step's row, or a slot past the range (unused)
      const uint16_t* kp = own ? ks : kcb + (int64_t)j * 64;
      const uint16_t* vp = own ? vs : vcb + (int64_t)j * 64;
      kr[u] = *(const u32x4*)(kp + p * 8);
      vr[u] = *(const u32x4*)(vp + p * 8);
    }
    float sc[AD_U];
    float mn = m;
#pragma unroll
    for (int u = 0; u < AD_U; ++u) {
      float kf[8];
      unpack8(kr[u], kf);
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d = fmaf(q[e], kf[e], d);
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      d += __shfl_xor(d, 4, 64);
      sc[u] = (jb + u * AD_G < j1) ? d * scale : NEG_INF;
      mn = fmaxf(mn, sc[u]);
    }
    // (slot 0 is in range, so mn is finite here)
    const float corr = (m == NEG_INF) ? 0.f : __builtin_amdgcn_exp2f((m - mn) * L2E);
    l *= corr;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] *= corr;
    m = mn;
#pragma unroll
    for (int u = 0; u < AD_U; ++u) {
      if (jb + u * AD_G < j1) {
        const float pr = __builtin_amdgcn_exp2f((sc[u] - mn) * L2E);
        float vf[8];
        unpack8(vr[u], vf);
        l += pr;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = fmaf(pr, vf[e], o[e]);
      }
    }
  }
  if (p == 0) { sm[g] = m; sl[g] = l; }
#pragma unroll
  for (int e = 0; e < 8; ++e) so[g][p * 8 + e] = o[e];
  __syncthreads();
  if (tid < 64) {
    float M = NEG_INF;
    for (int i = 0; i < AD_G; ++i) M = fmaxf(M, sm[i]);
    float L = 0.f, O = 0.f;
    if (M > NEG_INF) {
      for (int i = 0; i < AD_G; ++i) {
        if (sm[i] > NEG_INF) {  // a group with no key adds nothing (select, not a product with exp(-inf))
          const float w = __builtin_amdgcn_exp2f((sm[i] - M) * L2E);
          L = fmaf(sl[i], w, L);
          O = fmaf(so[i][tid], w, O);
        }
      }
    }
    if (S == 1) {
      out[(int64_t)bh * 64 + tid] = f2bf(O / L);  // key len[b] is always there: L > 0
    } else {
      float* wp = ws + ((int64_t)bh * S + s) * AD_PART;
      if (tid == 0) { wp[0] = M; wp[1] = L; }
      wp[2 + tid] = O;
    }
  }
}

__global__ __launch_bounds__(64) void attn_decode_combine_kernel(const float* __restrict__ ws, int S, uint16_t* __restrict__ out) {
  const int bh = blockIdx.x, d = threadIdx.x;
  const float* wp = ws + (int64_t)bh * S * AD_PART;
  float M = NEG_INF;
  for (int s = 0; s < S; ++s) M = fmaxf(M, wp[s * AD_PART]);
  float L = 0.f, O = 0.f;
  for (int s = 0; s < S; ++s) {
    const float ms = wp[s * AD_PART];
    if (ms > NEG_INF) {
      const float w = __builtin_amdgcn_exp2f((ms - M) * L2E);
      L = fmaf(wp[s * AD_PART + 1], w, L);
      O = fmaf(wp[s * AD_PART + 2 + d], w, O);
    }
  }
  out[(int64_t)bh * 64 + d] = f2bf(O / L);
}

// =================================================================== linear_skinny
// Block = 4 waves on one 16-column tile of y.  v_mfma_f32_16x16x32_bf16: A = x (lane l: row l & 15, k = 8 (l >> 4)
// + j), B = w^T (lane l: w[n0 + (l & 15)][k = 8 (l >> 4) + j], 16 contiguous bytes of a weight row, straight from
// global memory), D: column l & 15, rows 4 (l >> 4) + r.  Rows >= M of A are zero fragments (the load is pointed at
// row M - 1 and replaced).  The 32-wide K chunks of the block's range go round-robin to the waves; the four wave
// partials are summed in wave order through LDS, then -- with a K split over blocks -- the block partials in
// block order by linear_skinny_finish_kernel.
constexpr int LS_NW = 4, LS_U = 4;

DPE_DEVICE float gelu_tanh(float x) {  // hgemm.hip's gelu_fwd
  const float u2 = -1.5957691216057308f * (x + 0.044715f * x * x * x);
  return x * __builtin_amdgcn_rcpf(1.f + __expf(u2));
}

struct LsEpi {
  const float* bias;
  const float* res;
  int64_t ldr;
  void* y;
  int64_t ldy;
  int gelu, out_f32;
};

DPE_DEVICE void ls_emit(const LsEpi& e, int m, int n, float v) {
  if (e.bias) v += e.bias[n];
  if (e.out_f32) {
    if (e.res) v += e.res[(int64_t)m * e.ldr + n];
    ((float*)e.y)[(int64_t)m * e.ldy + n] = v;
  } else {
    if (e.gelu) v = gelu_tanh(v);
    ((uint16_t*)e.y)[(int64_t)m * e.ldy + n] = f2bf(v);
  }
}

// NT: 16-column tiles per block.  A wave loads each A fragment once for its NT B fragments, so a wide N (the LM head:
// 3144 tiles) re-reads x from the L2 NT times less often; narrow N keeps NT = 1 for the workgroup count.
template <int NT>
__global__ __launch_bounds__(64 * LS_NW) void linear_skinny_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                                   const uint16_t* __restrict__ w, int64_t ldw, int M, int N,
                                                                   int K, int ksplit, float* __restrict__ ws, LsEpi epi) {
  constexpr int U = NT == 1 ? LS_U : 2;  // (four tiles: two chunks in flight measured faster than four)
  __shared__ float part[LS_NW][NT][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n0 = blockIdx.x * 16 * NT, ks = blockIdx.y;
  const int nck = K >> 5, per = (nck + ksplit - 1) / ksplit;
  const int c0 = ks * per, c1 = c0 + per < nck ? c0 + per : nck;
  const int r = lane & 15, kq = (lane >> 4) * 8;
  const bool live = r < M;
  const uint16_t* xp = x + (int64_t)(live ? r : M - 1) * ldx + kq;
  const uint16_t* wp = w + (int64_t)(n0 + r) * ldw + kq;
  const int64_t wt = 16 * ldw;  // one column tile further
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  int c = c0 + wid;
  for (; c + (U - 1) * LS_NW < c1; c += U * LS_NW) {
    bf16x8 bf[NT][U], af[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) bf[t][u] = *(const bf16x8*)(wp + t * wt + (int64_t)(c + u * LS_NW) * 32);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      af[u] = *(const bf16x8*)(xp + (int64_t)(c + u * LS_NW) * 32);
      af[u] = live ? af[u] : zero;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u], bf[t][u], acc[t], 0, 0, 0);
  }
  for (; c < c1; c += LS_NW) {
    bf16x8 b[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) b[t] = *(const bf16x8*)(wp + t * wt + (int64_t)c * 32);
    bf16x8 a = *(const bf16x8*)(xp + (int64_t)c * 32);
    a = live ? a : zero;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[t], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wid][t][(lane >> 4) * 4 + i][r] = acc[t][i];
  __syncthreads();
  const int m = tid >> 4, n = tid & 15;
  if (m < M) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float v = part[0][t][m][n];
#pragma unroll
      for (int i = 1; i < LS_NW; ++i) v += part[i][t][m][n];
      if (ksplit == 1) ls_emit(epi, m, n0 + t * 16 + n, v);
      else ws[((int64_t)ks * M + m) * N + n0 + t * 16 + n] = v;
    }
  }
}

__global__ __launch_bounds__(256) void linear_skinny_finish_kernel(const float* __restrict__ ws, int M, int N, int ksplit,
                                                                   LsEpi epi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M * N) return;
  float v = ws[i];
  for (int s = 1; s < ksplit; ++s) v += ws[(int64_t)s * M * N + i];
  ls_emit(epi, i / N, i % N, v);
}

// =================================================================== sample_logits
// One workgroup per row, the row held in registers as loaded.  Both filters are thresholds on the VALUES: with
// key() the order-preserving integer image of a logit, the largest c whose weight W(key >= c) still reaches a
// target is found by bisection over the key's bits (16 for bf16 logits, 32 for fp32; z -> z / temperature is
// monotone, so the logit's key orders the scaled values too):
//   top-k  W = count, target k            -> v_k, the k-th largest value counted with multiplicity
//   top-p  W = softmax mass, target p Z   -> the smallest kept value: j stays iff the mass above it is < p
// Every count and mass is a block reduction in a fixed order.  The draw is a Gumbel-max over the kept columns.
constexpr uint32_t SAMPLE_C3 = 0x5A3C91E7u;  // Philox counter word 3: dropout uses 0x9E3779B9, mix_draw small integers

DPE_DEVICE u32x4 sample_philox(uint64_t seed, uint64_t ctr, uint32_t stream) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t c0 = stream, c1 = (uint32_t)ctr, c2 = (uint32_t)(ctr >> 32), c3 = SAMPLE_C3;
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

template <typename TIn>
struct SRow;
template <>
struct SRow<uint16_t> {
  static constexpr int BITS = 16;
  u32x4 v;
  DPE_DEVICE void load(const uint16_t* p) { v = *(const u32x4*)p; }
  DPE_DEVICE void touch() { asm volatile("" : "+v"(v)); }
  DPE_DEVICE void vals(float* f) const { unpack8(v, f); }
  DPE_DEVICE void keys(uint32_t* k) const {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t h = (i & 1) ? (v[i >> 1] >> 16) : (v[i >> 1] & 0xffffu);
      k[i] = (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
    }
  }
  static DPE_DEVICE float unkey(uint32_t k) {
    const uint32_t h = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
    return __uint_as_float(h << 16);
  }
};
template <>
struct SRow<float> {
  static constexpr int BITS = 32;
  f32x4 a, b;
  DPE_DEVICE void load(const float* p) { a = *(const f32x4*)p; b = *(const f32x4*)(p + 4); }
  DPE_DEVICE void touch() { asm volatile("" : "+v"(a), "+v"(b)); }
  DPE_DEVICE void vals(float* f) const {
    f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
  }
  DPE_DEVICE void keys(uint32_t* k) const {
    float f[8];
    vals(f);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t h = __float_as_uint(f[i]);
      k[i] = (h & 0x80000000u) ? ~h : (h | 0x80000000u);
    }
  }
  static DPE_DEVICE float unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
  }
};

// block sums in a fixed order (lanes by xor tree, then waves 0 .. NW - 1); every thread gets the result
template <int NT>
DPE_DEVICE float sblock_sum(float v, float* sh) {
  v = warp_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) r += sh[w];
  return r;
}

template <int NT>
DPE_DEVICE void sblock_argmax(float& m, int& am, float* shf, int* shi) {
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > m || (om == m && oa < am)) { m = om; am = oa; }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { shf[threadIdx.x >> 6] = m; shi[threadIdx.x >> 6] = am; }
  __syncthreads();
  m = shf[0];
  am = shi[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w)
    if (shf[w] > m || (shf[w] == m && shi[w] < am)) { m = shf[w]; am = shi[w]; }
}

template <typename TIn, int NT, int MAXC>
__global__ __launch_bounds__(NT) void sample_kernel(const TIn* __restrict__ logits, int V, int64_t ld, float temperature,
                                                    int top_k, float top_p, const int64_t* __restrict__ rng, uint32_t stream,
                                                    int eos_id, int32_t* done, int64_t* __restrict__ out) {
  using Row = SRow<TIn>;
  __shared__ float shf[NT / 64];
  __shared__ int shi[NT / 64];
  const int row = blockIdx.x, tid = threadIdx.x;
  if (done != nullptr && eos_id >= 0 && done[row] != 0) {  // (uniform over the block)
    if (tid == 0) out[row] = eos_id;
    return;
  }
  const TIn* z = logits + (int64_t)row * ld;
  const int nch = (V + 7) >> 3;
  Row rc[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = tid + c * NT;
    if (ch < nch) rc[c].load(z + (int64_t)ch * 8);
  }
  float best = NEG_INF;
  int arg = 0x7fffffff;
  if (temperature == 0.f) {
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int ch = tid + c * NT;
      if (ch < nch) {
        float f[8];
        rc[c].vals(f);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (ch * 8 + e < V && (f[e] > best || arg == 0x7fffffff)) { best = f[e]; arg = ch * 8 + e; }
      }
    }
  } else {
    // ---- the largest value: softmax reference point
    float zmax = NEG_INF;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int ch = tid + c * NT;
      if (ch < nch) {
        float f[8];
        rc[c].vals(f);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (ch * 8 + e < V) zmax = fmaxf(zmax, f[e]);
      }
    }
    {
      int dummy = 0;
      sblock_argmax<NT>(zmax, dummy, shf, shi);
    }
    const float smax = zmax / temperature;
    // keys of the columns >= V read as 0, below every candidate c >= 1
    // (the row is opaque to the compiler at every use: keys and scaled values are recomputed per pass, not hoisted
    // out of the bisection loops into 64 more registers each)
    auto row_keys = [&](int c, int ch, uint32_t* k) {
      rc[c].touch();
      rc[c].keys(k);
      if (ch * 8 + 8 > V) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (ch * 8 + e >= V) k[e] = 0u;
      }
    };
    uint32_t ck = 1u;  // kept: key >= ck (1: every real column)
    if (top_k > 0 && top_k < V) {
      uint32_t t = 0u;
      for (int bit = Row::BITS - 1; bit >= 0; --bit) {
        const uint32_t cand = t | (1u << bit);
        float cnt = 0.f;  // counts <= 65536: exact in fp32
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          const int ch = tid + c * NT;
          if (ch < nch) {
            uint32_t k[8];
            row_keys(c, ch, k);
#pragma unroll
            for (int e = 0; e < 8; ++e) cnt += (k[e] >= cand) ? 1.f : 0.f;
          }
        }
        cnt = sblock_sum<NT>(cnt, shf);
        if (cnt >= (float)top_k) t = cand;
      }
      ck = t > 1u ? t : 1u;
    }
    float sthr = Row::unkey(ck) / temperature;  // s_j >= sthr <=> kept (ties in s across different logits stay)
    if (ck == 1u) sthr = NEG_INF;
    if (top_p < 1.f) {
      auto mass_ge = [&](uint32_t cand) {
        float ms = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          const int ch = tid + c * NT;
          if (ch < nch) {
            uint32_t k[8];
            float f[8];
            row_keys(c, ch, k);
            rc[c].vals(f);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              if (k[e] >= cand) ms += expf(f[e] / temperature - smax);
              __builtin_amdgcn_sched_barrier(0);  // one element at a time: interleaved division / expf chains spill
            }
          }
        }
        return sblock_sum<NT>(ms, shf);
      };
      const float target = top_p * mass_ge(ck);
      uint32_t t = 0u;
      for (int bit = Row::BITS - 1; bit >= 0; --bit) {
        const uint32_t cand = t | (1u << bit);
        // below ck the kept mass does not grow: the candidate passes iff it is <= ck or its own mass reaches the target
        const float ms = mass_ge(cand > ck ? cand : ck);
        if (cand <= ck || ms >= target) t = cand;
      }
      if (t > ck) {
        ck = t;
        sthr = Row::unkey(ck) / temperature;
      }
    }
    // ---- Gumbel-max over the kept columns
    const uint64_t seed = (uint64_t)rng[0];
    const uint64_t base = (uint64_t)rng[1] + (uint64_t)row * (uint64_t)((V + 3) >> 2);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int ch = tid + c * NT;
      if (ch < nch) {
        float f[8];
        rc[c].touch();
        rc[c].vals(f);
#pragma unroll
        for (int hq = 0; hq < 2; ++hq) {
          bool any = false;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int j = ch * 8 + hq * 4 + e;
            f[hq * 4 + e] = f[hq * 4 + e] / temperature;
            any = any || (j < V && f[hq * 4 + e] >= sthr);
          }
          if (any) {
            const u32x4 rr = sample_philox(seed, base + (uint64_t)(ch * 2 + hq), stream);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int j = ch * 8 + hq * 4 + e;
              const float s = f[hq * 4 + e];
              if (j < V && s >= sthr) {
                const float u = (float)(2u * (rr[e] >> 9) + 1u) * 5.9604644775390625e-08f;  // (2n + 1) 2^-24, exact
                const float sc = s - logf(-logf(u));
                if (sc > best || arg == 0x7fffffff) { best = sc; arg = j; }
              }
              __builtin_amdgcn_sched_barrier(0);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  if (arg == 0x7fffffff) best = NEG_INF;
  sblock_argmax<NT>(best, arg, shf, shi);
  if (tid == 0) {
    if (arg == 0x7fffffff) arg = 0;  // (a row of NaNs: no column compares)
    out[row] = arg;
    if (done != nullptr && eos_id >= 0 && arg == eos_id) done[row] = 1;
  }
}

template <typename TIn>
int sample_launch(const TIn* logits, int B, int V, int64_t ld, float temperature, int top_k, float top_p, const int64_t* rng,
                  uint32_t stream, int eos_id, int32_t* done, int64_t* out, hipStream_t st) {
  const int nch = (V + 7) >> 3;
#define DPE_SAMPLE(NT, MC)                                                                                               \
  if (nch <= NT * MC) {                                                                                                  \
    hipLaunchKernelGGL((sample_kernel<TIn, NT, MC>), dim3(B), dim3(NT), 0, st, logits, V, ld, temperature, top_k, top_p, \
                       rng, stream, eos_id, done, out);                                                                  \
    return 0;                                                                                                            \
  }
  DPE_SAMPLE(64, 2)
  DPE_SAMPLE(256, 2)
  DPE_SAMPLE(1024, 2)
  // the widest rows: 32 VGPRs of a 1024-thread block's 128 per thread hold 65536 bf16 columns or 32768 fp32 ones (an
  // fp32 row of 64 VGPRs spills); wider fp32 rows are an error
  if constexpr (sizeof(TIn) == 2) {
    DPE_SAMPLE(1024, 8)
  } else {
    DPE_SAMPLE(1024, 4)
  }
#undef DPE_SAMPLE
  return 2;
}

}  // namespace

extern "C" {

int dpe_attn_decode_splits(int BH, int Tmax) {
  int s = 512 / (BH > 0 ? BH : 1), t = Tmax / 128;
  s = s < t ? s : t;
  return s < 1 ? 1 : (s > 16 ? 16 : s);
}

int64_t dpe_attn_decode_ws_floats(int BH, int S) { return S > 1 ? (int64_t)BH * S * AD_PART : 0; }

int dpe_attn_decode(const uint16_t* qkv_step, uint16_t* kc, uint16_t* vc, const int32_t* len, int B, int H, int Tmax, int S,
                    float scale, float* ws, uint16_t* out, hipStream_t st) {
  if (B <= 0 || H <= 0 || Tmax <= 0 || S < 1 || S > 65535 || (S > 1 && ws == nullptr)) return 1;
  hipLaunchKernelGGL(attn_decode_kernel, dim3(S, B * H), dim3(AD_NT), 0, st, qkv_step, kc, vc, len, H, Tmax, S, scale, ws, out);
  if (S > 1) hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(B * H), dim3(64), 0, st, ws, S, out);
  return 0;
}

int dpe_linear_skinny_ok(int M, int N, int K, int64_t ldx, int64_t ldw) {
  return M >= 1 && M <= 16 && K >= 32 && K % 32 == 0 && N >= 16 && N % 16 == 0 && ldx % 8 == 0 && ldw % 8 == 0 && ldx >= K &&
         ldw >= K;
}

// K split over blocks: only where the column tiles alone leave most CUs idle and every block still streams K >= 768
// of its rows.  Measured (scripts/bench_decode.py, docs/perf_notes.md): the second launch costs more than the split
// gains at K = 768 (N = 768 .. 3072) and pays at N = 768, K = 3072.
int dpe_linear_skinny_ksplit(int M, int N, int K) {
  (void)M;
  const int tiles = N / 16, nck = K / 32;
  int ks = 1;
  while (ks < 8 && tiles * ks < 256 && nck / (ks * 2) >= 24) ks *= 2;
  return ks;
}

// column tiles per block: 4 where that still leaves >= 512 workgroups and x has rows enough for its re-reads to
// matter (measured on the LM head: one tile is faster at M = 1, four at M = 8 and 16)
static int ls_tiles(int M, int N) { return (M >= 8 && N % 64 == 0 && N / 64 >= 512) ? 4 : 1; }

int dpe_linear_skinny_waves() { return LS_NW; }

int dpe_linear_skinny(const uint16_t* x, int64_t ldx, const uint16_t* w, int64_t ldw, int M, int N, int K, const float* bias,
                      int gelu, int out_f32, const float* res, int64_t ldr, void* y, int64_t ldy, int ksplit, float* ws,
                      hipStream_t st) {
  if (!dpe_linear_skinny_ok(M, N, K, ldx, ldw)) return 1;
  if (ksplit < 1 || ksplit > K / 32 || (ksplit > 1 && ws == nullptr)) return 2;
  if ((res && !out_f32) || (gelu && out_f32)) return 3;
  LsEpi e{bias, res, ldr, y, ldy, gelu, out_f32};
  if (ls_tiles(M, N) == 4)
    hipLaunchKernelGGL(linear_skinny_kernel<4>, dim3(N / 64, ksplit), dim3(64 * LS_NW), 0, st, x, ldx, w, ldw, M, N, K, ksplit, ws, e);
  else
    hipLaunchKernelGGL(linear_skinny_kernel<1>, dim3(N / 16, ksplit), dim3(64 * LS_NW), 0, st, x, ldx, w, ldw, M, N, K, ksplit, ws, e);
  if (ksplit > 1)
    hipLaunchKernelGGL(linear_skinny_finish_kernel, dim3((M * N + 255) / 256), dim3(256), 0, st, ws, M, N, ksplit, e);
  return 0;
}

int dpe_sample_logits(const void* logits, int in_bf16, int B, int V, int64_t ld, float temperature, int top_k, float top_p,
                      const int64_t* rng, uint32_t stream, int eos_id, int32_t* done, int64_t* out, hipStream_t st) {
  if (B <= 0 || V <= 0 || V > 65536 || ld % 8 != 0 || ld < ((V + 7) / 8) * 8 || !(temperature >= 0.f)) return 1;
  if (in_bf16)
    return sample_launch<uint16_t>((const uint16_t*)logits, B, V, ld, temperature, top_k, top_p, rng, stream, eos_id, done, out, st);
  return sample_launch<float>((const float*)logits, B, V, ld, temperature, top_k, top_p, rng, stream, eos_id, done, out, st);
}
}
