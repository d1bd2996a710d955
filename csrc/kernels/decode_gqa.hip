// Llama generation: grouped-query decode attention with the rotary embedding of the step fused in (gfx950).
//
//   attn_decode_gqa   the new token's Hq = G Hkv query heads against a head-major bf16 cache of Hkv heads
//
// qkv_step [B, Hq + 2 Hkv, 64] is the token's c_attn output, unrotated (Q heads, K heads, V heads); kc / vc
// [B, Hkv, Tmax, 64], kc holding rotated keys.  With n = clamp(len[b], 0, Tmax - 1): the G queries of a group and the
// step's key are rotated by table row clamp(n, 0, P - 1) (rotate-half, rope_kernel's expression, fp32, one RNE
// rounding); row b attends keys 0 .. n, key n being the step's rotated K and unrotated V, which split 0's workgroup
// also stores into cache row n.  No workgroup loads a cache row >= n.  window = W >= 1 (sliding-window attention, 0 =
// none): row b attends keys max(0, n - W + 1) .. n, and no workgroup loads a cache row below that either.
//
// Work split.  Grid (S, B Hkv): one workgroup of 4 waves serves one KV head and all G of its query heads, so every
// K / V byte is loaded once for the group.  The split's key range is cut into 32-key tiles that go round-robin to
// the waves; a wave keeps its own online-softmax state (m, l, O) for the 16 head slots; the four states are merged
// through LDS in wave order, the S split partials in split order by attn_decode_combine_kernel (decode.hip), whose
// [query head, S, 66] workspace layout this kernel writes for the real heads g < G.  No atomics, no scratch.
//
// MFMA form (v_mfma_f32_16x16x32_bf16), the flash forward's "swapped QK^T" at one query row per head:
//   S^T = K Q^T   A = K: lane l takes key l & 15, dims 32 c + 8 (l >> 4) .. + 7 -- 16 contiguous bytes of a cache row,
//                 straight from global memory into the fragment, no LDS.  B = the rotated Q of the group: lane l
//                 holds head l & 15, the same dims; every wave rotates it once into registers (cheaper than one LDS
//                 image and a barrier), heads >= G are zero fragments.  D: head l & 15 on the lane, keys
//                 16 nt + 4 (l >> 4) + e: two MFMAs per 16 keys.
//   softmax       the row maximum of a head is the lane's 8 registers plus two permlane swaps per tile; the rescale
//                 is deferred until a tile's maximum exceeds the running one by 2^8 (attn.hip), raw v_exp_f32.
//   O^T = V^T P^T P stays in registers: packed to bf16 it IS the B operand, the key of k-index 8 (l >> 4) + j being
//                 whatever the first MFMA's D layout left in the lane ({4g .. 4g+3} u {16+4g ..}).  A = V contracted
//                 over keys; V is dim-contiguous in memory, so a wave's V tile goes through a two-slot swizzled LDS
//                 ring of its own (4 KiB a slot) and is read back with the transposing ds_read_b64_tr_b16 from
//                 exactly those permuted rows.  The ring is private to the wave: no workgroup barrier in the loop.
//   row sum       on the matrix unit: an all-ones A operand against the same bf16 P fragment (one MFMA per tile).
//                 Chosen over 8 VALU adds and a final cross-lane sum because l is then the sum of exactly the
//                 rounded P that O accumulated (out is a convex combination of V rows), every lane of a head holds
//                 the whole sum, and the matrix unit is otherwise idle in a kernel bound by the cache stream.
// The next tile's K and V loads are issued before the current tile's arithmetic.  Every load in the tile loop is
// unconditional: a slot at or past min(n, end of the split) points at the step's own (finite) row in qkv_step; its K
// fragment is replaced by the rotated step key by select, its V is the step's V.  A slot past the split is left out
// of the maximum and its P is an exact 0 by select after the exponential, so a masked key multiplies a finite V.
// Every workgroup whose range holds key n computes the same rotated-K bits from the same expression, which are the
// bits stored into the cache.
#include "common.h"
#include "launch.h"

namespace {

constexpr float GD_L2E = 1.4426950408889634f, GD_LN2 = 0.6931471805599453f;
constexpr int GD_NW = 4;               // waves per workgroup
constexpr int GD_TK = 32;              // keys per tile
constexpr int GD_SLOT = GD_TK * 128;   // bytes of one V tile image
constexpr int GD_RING = 2;             // slots per wave
constexpr int GD_PART = 66;            // floats per partial: m, l, o[64] (decode.hip's AD_PART)
constexpr int GD_OST = 68;             // floats per head row of the merge image (16-byte rows, off the bank stride)
constexpr float GD_DEFER = 8.f;        // log2 units: defer the running-max update below 2^8
constexpr float GD_NEG_INF = -INFINITY;

typedef __attribute__((address_space(3))) s16x4 gd_lds4;

#define GD_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

DPE_DEVICE int gd_clamp_len(int len, int Tmax) { return len < 0 ? 0 : (len > Tmax - 1 ? Tmax - 1 : len); }

DPE_DEVICE void gd_split_range(int n, int S, int s, int& j0, int& j1) {  // decode.hip's split_range
  const int chunk = (n + S - 1) / S;
  j0 = s * chunk;
  j1 = j0 + chunk < n ? j0 + chunk : n;
  if (j0 > n) j0 = n;
}

// [32 keys][64 bf16] image (128-B rows) read transposed from the permuted rows {4g + q, 16 + 4g + q}: attn.hip's pimg
DPE_DEVICE int gd_vimg(int k, int chunk) { return k * 128 + ((chunk ^ (((k >> 1) & 3) << 1)) << 4); }

// A operand of O^T = V^T P^T: dims c0 + (lane & 15), k-index 8g + j = keys {4g + j, 16 + 4g + j - 4} (attn.hip's trfrag)
DPE_DEVICE bf16x8 gd_vfrag(const char* img, int c0) {
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int r1 = 4 * g + q, r2 = r1 + 16;
  const int ch = (c0 >> 3) + (p >> 1), sub = (p & 1) * 8;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gd_lds4*)(img + gd_vimg(r1, ch) + sub));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gd_lds4*)(img + gd_vimg(r2, ch) + sub));
  s16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return __builtin_bit_cast(bf16x8, r);
}

DPE_DEVICE bf16x8 gd_pack_frag(const f32x4& a, const f32x4& b) {
  u32x4 u;
  u[0] = pack_bf2(a[0], a[1]); u[1] = pack_bf2(a[2], a[3]);
  u[2] = pack_bf2(b[0], b[1]); u[3] = pack_bf2(b[2], b[3]);
  return __builtin_bit_cast(bf16x8, u);
}

// the maximum over the four lane groups that hold one head (attn.hip's rowmax4)
DPE_DEVICE float gd_rowmax4(float v) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(s[0]), __uint_as_float(s[1]));
}

// the wave's LDS writes have landed and the compiler keeps the transposing reads behind them (the ring is private
// to the wave, whose LDS instructions execute in order: no s_barrier)
DPE_DEVICE void gd_wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

struct GdTile {  // one 32-key tile in flight: K as the four A fragments, V as the lane's four 16-byte chunks
  bf16x8 k[2][2];
  u32x4 v[4];
};

__global__ __launch_bounds__(64 * GD_NW) void attn_decode_gqa_kernel(const uint16_t* __restrict__ qkv, uint16_t* kc, uint16_t* vc,
                                                                     const int32_t* __restrict__ lens,
                                                                     const float* __restrict__ cs, const float* __restrict__ sn,
                                                                     int Hq, int Hkv, int Tmax, int P, int S, float sl2,
                                                                     float* __restrict__ ws, uint16_t* __restrict__ out,
                                                                     int window) {
  __shared__ __attribute__((aligned(16))) char smem[GD_NW * GD_RING * GD_SLOT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, li = lane & 15;
  const int s = blockIdx.x, bk = blockIdx.y, b = bk / Hkv, kvh = bk - b * Hkv;
  const int G = Hq / Hkv, W = Hq + 2 * Hkv;
  const int n = gd_clamp_len(lens[b], Tmax);
  const int pr = n < P - 1 ? n : P - 1;  // a length chooses a table row and loop bounds, never an address beyond them
  const uint16_t* tok = qkv + (int64_t)b * W * 64;
  const uint16_t* qs = tok + (int64_t)(kvh * G + (li < G ? li : G - 1)) * 64;
  const uint16_t* ks = tok + (int64_t)(Hq + kvh) * 64;
  const uint16_t* vs = tok + (int64_t)(Hq + Hkv + kvh) * 64;
  uint16_t* kcb = kc + (int64_t)bk * Tmax * 64;
  uint16_t* vcb = vc + (int64_t)bk * Tmax * 64;

  // ---- the rotation: the lane holds dims 8g .. 8g + 7 and their partners 32 + 8g .. of its head
  float c[8], sv[8];
  {
    const f32x4 c0 = *(const f32x4*)(cs + (int64_t)pr * 32 + 8 * g), c1 = *(const f32x4*)(cs + (int64_t)pr * 32 + 8 * g + 4);
    const f32x4 s0 = *(const f32x4*)(sn + (int64_t)pr * 32 + 8 * g), s1 = *(const f32x4*)(sn + (int64_t)pr * 32 + 8 * g + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { c[e] = c0[e]; c[e + 4] = c1[e]; sv[e] = s0[e]; sv[e + 4] = s1[e]; }
  }
  auto rotate = [&](const uint16_t* row, bf16x8& lo, bf16x8& hi) {
    float a[8], bb[8], oa[8], ob[8];
    unpack8(*(const u32x4*)(row + 8 * g), a);
    unpack8(*(const u32x4*)(row + 32 + 8 * g), bb);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      oa[e] = a[e] * c[e] - bb[e] * sv[e];
      ob[e] = bb[e] * c[e] + a[e] * sv[e];
    }
    lo = __builtin_bit_cast(bf16x8, pack8(oa));
    hi = __builtin_bit_cast(bf16x8, pack8(ob));
  };
  const bf16x8 zfrag = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 qf[2], kr[2];
  rotate(qs, qf[0], qf[1]);
  qf[0] = li < G ? qf[0] : zfrag;
  qf[1] = li < G ? qf[1] : zfrag;
  rotate(ks, kr[0], kr[1]);
  if (s == 0 && w == 0 && li < 2) {  // the one store of the step's row: lanes li = 0 the rotated K, li = 1 the V
    const u32x4 a0 = li == 0 ? __builtin_bit_cast(u32x4, kr[0]) : *(const u32x4*)(vs + 8 * g);
    const u32x4 a1 = li == 0 ? __builtin_bit_cast(u32x4, kr[1]) : *(const u32x4*)(vs + 32 + 8 * g);
    uint16_t* dst = (li == 0 ? kcb : vcb) + (int64_t)n * 64 + 8 * g;
    *(u32x4*)dst = a0;
    *(u32x4*)(dst + 32) = a1;
  }

  // window: the keys below klo = max(0, n - window + 1) are outside it; the splits share klo .. n, so no cache row below
  // klo is loaded (a window chooses loop bounds, never an address beyond the rows 0 .. n)
  const int klo = window > 0 && n + 1 > window ? n + 1 - window : 0;
  int j0, j1;
  gd_split_range(n + 1 - klo, S, s, j0, j1);
  j0 += klo;
  j1 += klo;
  const int jend = j1 < n ? j1 : n;  // keys below come from the cache; from jend on a slot is the step's row
  const int ntile = (j1 - j0 + GD_TK - 1) / GD_TK;
  char* ring = smem + w * (GD_RING * GD_SLOT);
  const int vkey = lane >> 3, vdc = lane & 7;  // V chunk i of the lane: key vkey + 8 i, dims 8 vdc ..

  // every address is in bounds whatever t is: a key below jend <= n is a cache row, anything else the step's row
  auto load = [&](int t, GdTile& tl) {
    const int jt = j0 + t * GD_TK;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int j = jt + 16 * nt + li;
      const uint16_t* p = (j >= jend ? ks : kcb + (int64_t)j * 64) + 8 * g;
      tl.k[nt][0] = *(const bf16x8*)p;
      tl.k[nt][1] = *(const bf16x8*)(p + 32);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = jt + vkey + 8 * i;
      const uint16_t* p = (j >= jend ? vs : vcb + (int64_t)j * 64) + 8 * vdc;
      tl.v[i] = *(const u32x4*)p;
    }
  };

  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const bf16x8 ones = __builtin_bit_cast(bf16x8, u32x4{0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u});
  f32x4 acc[4] = {zero, zero, zero, zero}, lacc = zero;
  float m = GD_NEG_INF;

  auto compute = [&](int t, const GdTile& tl, const char* img) {
    const int jt = j0 + t * GD_TK;
    f32x4 sc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const bool own = jt + 16 * nt + li >= jend;
      const bf16x8 k0 = own ? kr[0] : tl.k[nt][0], k1 = own ? kr[1] : tl.k[nt][1];
      sc[nt] = GD_MFMA(k1, qf[1], GD_MFMA(k0, qf[0], zero));
    }
    bool valid[2][4];
    float mx = GD_NEG_INF;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        valid[nt][e] = jt + 16 * nt + 4 * g + e < j1;
        sc[nt][e] = valid[nt][e] ? sc[nt][e] * sl2 : GD_NEG_INF;
        mx = fmaxf(mx, sc[nt][e]);
      }
    const float mc = gd_rowmax4(mx);  // finite: the tile's first key is in range
    const bool need = mc > m + GD_DEFER;
    if (__builtin_amdgcn_ballot_w64(need)) {
      const float alpha = need ? __builtin_amdgcn_exp2f(m - mc) : 1.f;  // m = -inf: 0 times the zero state
      m = need ? mc : m;
      lacc *= alpha;
#pragma unroll
      for (int d = 0; d < 4; ++d) acc[d] *= alpha;
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pv = __builtin_amdgcn_exp2f(sc[nt][e] - m);
        sc[nt][e] = valid[nt][e] ? pv : 0.f;
      }
    const bf16x8 pk = gd_pack_frag(sc[0], sc[1]);
    lacc = GD_MFMA(ones, pk, lacc);
#pragma unroll
    for (int d = 0; d < 4; ++d) acc[d] = GD_MFMA(gd_vfrag(img, 16 * d), pk, acc[d]);
  };

  GdTile cur, nxt;
  load(w, cur);
  int slot = 0;
  for (int t = w; t < ntile; t += GD_NW) {
    load(t + GD_NW, nxt);
    char* img = ring + slot * GD_SLOT;
#pragma unroll
    for (int i = 0; i < 4; ++i) *(u32x4*)(img + gd_vimg(vkey + 8 * i, vdc)) = cur.v[i];
    gd_wave_lds_fence();
    compute(t, cur, img);
    cur = nxt;
    slot ^= 1;
  }

  // ---- the four wave states, merged in wave order (the ring is dead: its memory carries the merge image)
  __syncthreads();
  float* fm = (float*)smem;            // [NW][16]
  float* fl = fm + GD_NW * 16;         // [NW][16]
  float* fo = fl + GD_NW * 16;         // [NW][16][GD_OST]
  if (g == 0) { fm[w * 16 + li] = m; fl[w * 16 + li] = lacc[0]; }
#pragma unroll
  for (int d = 0; d < 4; ++d) *(f32x4*)(fo + (w * 16 + li) * GD_OST + 16 * d + 4 * g) = acc[d];
  __syncthreads();
  const int hh = tid >> 4, d0 = (tid & 15) * 4;
  float M = GD_NEG_INF;
#pragma unroll
  for (int i = 0; i < GD_NW; ++i) M = fmaxf(M, fm[i * 16 + hh]);
  float L = 0.f;
  f32x4 O = zero;
  if (M > GD_NEG_INF) {
#pragma unroll
    for (int i = 0; i < GD_NW; ++i) {
      const float mw = fm[i * 16 + hh];
      if (mw > GD_NEG_INF) {  // a wave with no key adds nothing (select, not a product with exp(-inf))
        const float wt = __builtin_amdgcn_exp2f(mw - M);
        const f32x4 o = *(const f32x4*)(fo + (i * 16 + hh) * GD_OST + d0);
        L = fmaf(fl[i * 16 + hh], wt, L);
#pragma unroll
        for (int e = 0; e < 4; ++e) O[e] = fmaf(o[e], wt, O[e]);
      }
    }
  }
  if (hh < G) {
    const int64_t bq = (int64_t)b * Hq + kvh * G + hh;
    if (S == 1) {  // key n is always there: L > 0
      const float inv = 1.f / L;
      u32x2 r;
      r[0] = pack_bf2(O[0] * inv, O[1] * inv);
      r[1] = pack_bf2(O[2] * inv, O[3] * inv);
      *(u32x2*)(out + bq * 64 + d0) = r;
    } else {  // the combine kernel's partial: m in natural-log units
      float* wp = ws + (bq * S + s) * GD_PART;
      if ((tid & 15) == 0) { wp[0] = M * GD_LN2; wp[1] = L; }
#pragma unroll
      for (int e = 0; e < 4; ++e) wp[2 + d0 + e] = O[e];
    }
  }
}

}  // namespace

extern "C" int dpe_attn_decode_gqa(const uint16_t* qkv_step, uint16_t* kc, uint16_t* vc, const int32_t* len, const float* cos,
                                   const float* sin, int B, int Hq, int Hkv, int Tmax, int P, int S, float scale, float* ws,
                                   uint16_t* out, int window, hipStream_t st) {
  if (window < 0) return 1;
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0 || Hq / Hkv > 16 || Tmax <= 0 || Tmax > (1 << 24) || P <= 0) return 1;
  if (S < 1 || S > 65535 || (int64_t)B * Hkv > 65535 || (S > 1 && ws == nullptr)) return 1;
  hipLaunchKernelGGL(attn_decode_gqa_kernel, dim3(S, B * Hkv), dim3(64 * GD_NW), 0, st, qkv_step, kc, vc, len, cos, sin, Hq, Hkv,
                     Tmax, P, S, scale * GD_L2E, ws, out, window);
  if (S > 1) return dpe_attn_decode_combine(ws, B * Hq, S, out, st);
  return 0;
}
