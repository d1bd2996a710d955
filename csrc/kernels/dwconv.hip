// Depthwise 7x7 / stride 1 / pad 3 convolution on NHWC (ConvNeXt): forward, data gradient (the same kernel on dy with
// the filter rotated by 180 degrees, no bias) and the weight / bias gradients, walking rows like rowconv.hip and
// stem.hip with the VALU in the MFMA unit's place: one input channel per output channel leaves no K for an MFMA.
//
// Work split (plan() below, a function of the shape only).  A block owns (a slab of 2 CP channels, a run of RB output
// rows of one image, a column tile of WT <= 128 pixels).  Thread (pl, g) owns channel pair pl of the slab and the runs
// of PX = 4 adjacent pixels g, g + G, ...; CP * G <= 256.  CP is the multiple of 4 that keeps most lanes busy
// (whole slabs x whole pixel runs x threads used) under the ring's LDS budget.
//   * rows kernel: the pair's 2 x 49 taps sit in fp32 VGPRs for the whole block; an output row costs, per filter row,
//     10 LDS dwords (4 + 6 pixels of the pair) for 56 FMAs.  bf16 pairs are unpacked per use (2 VALU ops per dword).
//     The file is built with the packed fp32 ops off (_build.py): the compiler's own pairing of the two channels'
//     chains (784 v_pk_fma_f32, no v_fma_f32) takes this kernel to 256 VGPRs with 972 / 1000 B of scratch per lane.
//     So every FMA is a scalar-issue v_fma_f32, 49 per output element, and that is what bounds the kernel.
//     Hand-placed packed pairs (taps and inputs laid out as register pairs from the start) were not tried.
//   * wgrad kernel: the same walk with the roles swapped: 2 x (49 + 1) fp32 accumulators per thread, dy as the
//     multiplier (each dy element has one reader, so it is loaded from global one run ahead, not staged).  After the
//     last row the G threads of a channel are summed through LDS in the order g = 0 .. G - 1 and the block writes one
//     partial [C][50]; the reduce kernel sums the partials in a fixed order (8 interleaved strides, then those 8 in
//     order).  No atomics: bitwise repeatable.
// Data movement.  Input rows pass through an 8-slot LDS ring of [CP][PS] bf16 pairs, pair-major: slot = row & 7,
// PS = (WT + 6) | 1 dwords, the 3 + 3 halo pixels included, out-of-image columns stored as zeros (no test in the tap
// loop).  A thread's 10 dwords of a filter row are then consecutive (immediate offsets, no address arithmetic; with
// the pixel-major layout the 70 runtime-strided addresses spilled to scratch) and the odd PS spreads the lanes of a
// wave over the banks.  Row y + 4 is loaded into
// registers before output row y is computed and stored into the slot of row y - 4 after it: one barrier per row, each
// input row read from HBM once per block (the 6 halo rows of a row run are read by two blocks).  Rows above and below
// the image are skipped by block-uniform bounds on the unrolled filter-row loop; nothing is loaded out of range.  An
// fp32 input is rounded to bf16 (RNE) once, on its way into the ring.  Output: a 4 x 4 lane transpose (two xor
// shuffles) turns the quad's 4 pixels x 4 pairs into one 16-B chunk of 8 channels per lane.
//
// Budgets (hipcc -O3, gfx950; scratch 0 in every kernel):
//   VGPRs: dwconv7_rows_kernel 173 (bf16 in) / 181 (fp32 in), dwconv7_wgrad_kernel 189 / 197, reduce 14.  98 of
//   them are the taps / accumulators; __launch_bounds__(256, 2) = 2 waves per SIMD = 2 blocks per CU.  A bound of 3
//   waves per SIMD (168 VGPRs) spilled ~300 B per lane.
//   LDS: ring = 8 * CP * PS * 4 B <= 64 KiB, so LDS never lowers the 2 blocks per CU; the wgrad combine buffer
//   (20 KiB) reuses the ring, the allocation is the larger of the two.
//   ConvNeXt-T stages: 56x56x96 -> CP 16, G 16, 31.5 KiB; 28x28x192 -> 3 slabs, 35 KiB at CP 32; 14x14x384 -> CP 64,
//   G 4, 46 KiB; 7x7x768 -> CP 128, G 2, 60 KiB.
#include <algorithm>

#include "common.h"
#include "launch.h"

namespace dpe {
namespace dwconv {

constexpr int THREADS = 256, PX = 4, NR = 8, TAPS = 49, NACC = 50;
constexpr int WT_MAX = 128;
constexpr int RING_BYTES = 64 * 1024;
constexpr int KCH = 10;                            // accumulators per combine round (5 rounds of 10 = 50)
constexpr int COMBINE_BYTES = THREADS * KCH * 8;   // [KCH][G][CP] channel pairs of fp32
constexpr int TARGET_BLOCKS = 1024;

struct Plan {
  int CP, G, nslab, WT, PS, ntile, RB, nchunk, ring;
};

static Plan plan(int N, int H, int W, int C) {
  Plan q;
  q.ntile = (W + WT_MAX - 1) / WT_MAX;
  q.WT = ((W + q.ntile - 1) / q.ntile + PX - 1) / PX * PX;
  const int runs = q.WT / PX, pairs = C / 2;
  q.PS = (q.WT + 6) | 1;
  const int cap = std::min({pairs, 128, RING_BYTES / (NR * q.PS * 4) / 4 * 4});
  double best = -1.0;
  q.CP = 4;
  for (int cp = 4; cp <= cap; cp += 4) {
    const int ns = (pairs + cp - 1) / cp, g = THREADS / cp, passes = (runs + g - 1) / g;
    const double score = (double)pairs / (ns * cp) * runs / (passes * g) * (cp * g) / THREADS;
    if (score >= best) best = score, q.CP = cp;
  }
  q.G = THREADS / q.CP;
  q.nslab = (pairs + q.CP - 1) / q.CP;
  const int64_t units = (int64_t)N * q.nslab * q.ntile;
  int nchunk = (int)std::min<int64_t>((TARGET_BLOCKS + units - 1) / units, std::max(1, H / 8));
  q.RB = (H + nchunk - 1) / nchunk;
  q.nchunk = (H + q.RB - 1) / q.RB;
  q.ring = NR * q.CP * q.PS * 4;
  return q;
}

struct Args {
  const void* x;        // [N][H][W][C] bf16 or fp32
  const uint16_t* w;    // rows: [49][C] bf16 taps;  wgrad: dy [N][H][W][C] bf16
  const float* bias;    // rows: [C] or nullptr
  uint16_t* y;          // rows: [N][H][W][C] bf16
  float* part;          // wgrad: [NB][C][50]
  int H, W, C, CP, G, WT, PS, ntile, RB;
};

// One ring row in flight: this thread's (at most two) 16-B chunks of 8 channels, raw as loaded.
template <bool XF32>
struct Stage {
  u32x4 v[XF32 ? 4 : 2];
};

template <bool XF32>
struct RowIO {
  const char* x;
  int H, W, C, nq, nchk, col0, c0, cw, tid, PS;
  int64_t img;  // element offset of image n

  // chunk i of the row: pixel position j = i / nq (input column col0 - 3 + j), channels c0 + 8 (i % nq) .. + 7
  DPE_DEVICE void load(int row, Stage<XF32>& s) const {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = tid + k * THREADS, j = i / nq, ch = 8 * (i - j * nq), col = col0 - 3 + j;
      const bool ok = i < nchk && col >= 0 && col < W && ch < cw;
      const int64_t e = img + ((int64_t)row * W + col) * C + c0 + ch;
      if (XF32) {
        s.v[2 * k] = ok ? *(const u32x4*)(x + e * 4) : u32x4{0u, 0u, 0u, 0u};
        s.v[2 * k + 1] = ok ? *(const u32x4*)(x + e * 4 + 16) : u32x4{0u, 0u, 0u, 0u};
      } else {
        s.v[k] = ok ? *(const u32x4*)(x + e * 2) : u32x4{0u, 0u, 0u, 0u};
      }
    }
  }
  DPE_DEVICE void store(char* slot, const Stage<XF32>& s) const {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = tid + k * THREADS;
      if (i >= nchk) continue;
      u32x4 o;
      if (XF32) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          o[e] = pack_bf2(__uint_as_float(s.v[2 * k][2 * e]), __uint_as_float(s.v[2 * k][2 * e + 1]));
          o[2 + e] = pack_bf2(__uint_as_float(s.v[2 * k + 1][2 * e]), __uint_as_float(s.v[2 * k + 1][2 * e + 1]));
        }
      } else {
        o = s.v[k];
      }
      const int j = i / nq, pr = 4 * (i - j * nq);  // pair-major slot: pair pr + e at dword (pr + e) * PS + j
#pragma unroll
      for (int e = 0; e < 4; ++e) *(uint32_t*)(slot + (((pr + e) * PS + j) << 2)) = o[e];
    }
  }
};

DPE_DEVICE float lo_f(uint32_t v) { return __uint_as_float(v << 16); }
DPE_DEVICE float hi_f(uint32_t v) { return __uint_as_float(v & 0xffff0000u); }

// What both kernels share: the block's coordinates and the ring walk.
template <bool XF32>
struct Walk {
  RowIO<XF32> io;
  int pl, g, c, y0, y1, runs, npass, slot_bytes, n;
  bool live;

  DPE_DEVICE Walk(const Args& p) {
    const int tid = threadIdx.x;
    pl = tid % p.CP;
    g = tid / p.CP;
    const int tile = blockIdx.y % p.ntile, chunk = blockIdx.y / p.ntile;
    n = blockIdx.z;
    io.x = (const char*)p.x;
    io.H = p.H, io.W = p.W, io.C = p.C, io.tid = tid;
    io.nq = p.CP / 4;
    io.nchk = (p.WT + 6) * io.nq;
    io.col0 = tile * p.WT;
    io.c0 = blockIdx.x * p.CP * 2;
    io.cw = min(p.CP * 2, p.C - io.c0);
    io.img = (int64_t)n * p.H * p.W * p.C;
    c = io.c0 + 2 * pl;
    live = g < p.G && 2 * pl < io.cw;
    y0 = chunk * p.RB;
    y1 = min(p.H, y0 + p.RB);
    runs = p.WT / PX;
    npass = (runs + p.G - 1) / p.G;
    io.PS = p.PS;
    slot_bytes = p.CP * p.PS * 4;
  }
  DPE_DEVICE void prologue(char* ring) const {
    Stage<XF32> st;
    for (int row = max(0, y0 - 3); row <= min(io.H - 1, y0 + 3); ++row) {
      io.load(row, st);
      io.store(ring + (row & (NR - 1)) * slot_bytes, st);
    }
    __syncthreads();
  }
  // the row to prefetch while output row y is computed (-1: none)
  DPE_DEVICE int next_row(int y) const { return (y + 4 < io.H && y + 4 <= y1 + 2) ? y + 4 : -1; }
};

template <bool XF32>
__global__ __launch_bounds__(THREADS, 2) void dwconv7_rows_kernel(Args p) {
  extern __shared__ __attribute__((aligned(16))) char ring[];
  const Walk<XF32> k(p);
  const int H = p.H, W = p.W, C = p.C;

  float wa[TAPS], wb[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; ++t) {
    const uint32_t v = *(const uint32_t*)(p.w + (int64_t)t * C + (k.live ? k.c : 0));  // idle lanes: channel 0, unused
    wa[t] = lo_f(v);
    wb[t] = hi_f(v);
  }
  const float ba = p.bias ? p.bias[k.live ? k.c : 0] : 0.f, bb = p.bias ? p.bias[k.live ? k.c + 1 : 1] : 0.f;
  const int q = threadIdx.x & 3;  // lane of the quad = pixel of the run after the transpose
  const int cq = k.io.c0 + 2 * (k.pl & ~3);

  k.prologue(ring);
  Stage<XF32> st;
  for (int y = k.y0; y < k.y1; ++y) {
    const int nrow = k.next_row(y);
    if (nrow >= 0) k.io.load(nrow, st);
    for (int pass = 0; pass < k.npass; ++pass) {
      const int run = k.g + pass * p.G;
      const bool act = k.live && run < k.runs;
      const int px0 = act ? run * PX : 0;
      float a0[PX], a1[PX];
#pragma unroll
      for (int i = 0; i < PX; ++i) a0[i] = ba, a1[i] = bb;
      if (act) {
#pragma unroll
        for (int r = 0; r < 7; ++r) {
          const int row = y + r - 3;
          if (row < 0 || row >= H) continue;  // block-uniform: the exact zero rows are not visited
          const uint32_t* src = (const uint32_t*)(ring + (row & (NR - 1)) * k.slot_bytes) + k.pl * p.PS + px0;
          float xa[PX + 6], xb[PX + 6];
#pragma unroll
          for (int j = 0; j < PX + 6; ++j) {
            const uint32_t v = src[j];
            xa[j] = lo_f(v);
            xb[j] = hi_f(v);
          }
#pragma unroll
          for (int s = 0; s < 7; ++s)
#pragma unroll
            for (int i = 0; i < PX; ++i) {
              a0[i] = fmaf(xa[i + s], wa[r * 7 + s], a0[i]);
              a1[i] = fmaf(xb[i + s], wb[r * 7 + s], a1[i]);
            }
        }
      }
      // quad transpose: lane q ends with pixel px0 + q of the quad's four channel pairs (16 B)
      int v0 = (int)pack_bf2(a0[0], a1[0]), v1 = (int)pack_bf2(a0[1], a1[1]);
      int v2 = (int)pack_bf2(a0[2], a1[2]), v3 = (int)pack_bf2(a0[3], a1[3]);
      const bool b0 = q & 1, b1 = q & 2;
      const int t0 = __shfl_xor(b0 ? v0 : v1, 1, 64), t1 = __shfl_xor(b0 ? v2 : v3, 1, 64);
      if (b0) v0 = t0, v2 = t1; else v1 = t0, v3 = t1;
      const int s0 = __shfl_xor(b1 ? v0 : v2, 2, 64), s1 = __shfl_xor(b1 ? v1 : v3, 2, 64);
      u32x4 o;
      if (b1) o = u32x4{(uint32_t)s0, (uint32_t)s1, (uint32_t)v2, (uint32_t)v3};
      else o = u32x4{(uint32_t)v0, (uint32_t)v1, (uint32_t)s0, (uint32_t)s1};
      const int col = k.io.col0 + px0 + q;
      if (act && col < W) *(u32x4*)(p.y + k.io.img + ((int64_t)y * W + col) * C + cq) = o;
    }
    if (nrow >= 0) k.io.store(ring + (nrow & (NR - 1)) * k.slot_bytes, st);
    __syncthreads();
  }
}

// dy of one pixel run: 4 channel-pair dwords, zeros past the image's last column
struct DyRun {
  uint32_t v[PX];
};

template <bool XF32>
__global__ __launch_bounds__(THREADS, 2) void dwconv7_wgrad_kernel(Args p) {
  extern __shared__ __attribute__((aligned(16))) char ring[];
  const Walk<XF32> k(p);
  const int H = p.H, W = p.W, C = p.C;
  const uint16_t* dy = p.w;

  float wa[TAPS], wb[TAPS], ba = 0.f, bb = 0.f;
#pragma unroll
  for (int t = 0; t < TAPS; ++t) wa[t] = wb[t] = 0.f;

  auto load_dy = [&](int y, int pass, DyRun& d) {
    const int run = k.g + pass * p.G;
    const bool act = k.live && run < k.runs && y < k.y1;
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      const int col = k.io.col0 + run * PX + i;
      d.v[i] = (act && col < W) ? *(const uint32_t*)(dy + k.io.img + ((int64_t)y * W + col) * C + k.c) : 0u;
    }
  };

  k.prologue(ring);
  Stage<XF32> st;
  DyRun dn;
  load_dy(k.y0, 0, dn);
  for (int y = k.y0; y < k.y1; ++y) {
    const int nrow = k.next_row(y);
    if (nrow >= 0) k.io.load(nrow, st);
    for (int pass = 0; pass < k.npass; ++pass) {
      const DyRun d = dn;
      if (pass + 1 < k.npass) load_dy(y, pass + 1, dn); else load_dy(y + 1, 0, dn);
      const int run = k.g + pass * p.G;
      if (!(k.live && run < k.runs)) continue;
      float da[PX], db_[PX];
#pragma unroll
      for (int i = 0; i < PX; ++i) {
        da[i] = lo_f(d.v[i]);
        db_[i] = hi_f(d.v[i]);
        ba += da[i];
        bb += db_[i];
      }
#pragma unroll
      for (int r = 0; r < 7; ++r) {
        const int row = y + r - 3;
        if (row < 0 || row >= H) continue;
        const uint32_t* src = (const uint32_t*)(ring + (row & (NR - 1)) * k.slot_bytes) + k.pl * p.PS + run * PX;
        float xa[PX + 6], xb[PX + 6];
#pragma unroll
        for (int j = 0; j < PX + 6; ++j) {
          const uint32_t v = src[j];
          xa[j] = lo_f(v);
          xb[j] = hi_f(v);
        }
#pragma unroll
        for (int s = 0; s < 7; ++s)
#pragma unroll
          for (int i = 0; i < PX; ++i) {
            wa[r * 7 + s] = fmaf(da[i], xa[i + s], wa[r * 7 + s]);
            wb[r * 7 + s] = fmaf(db_[i], xb[i + s], wb[r * 7 + s]);
          }
      }
    }
    if (nrow >= 0) k.io.store(ring + (nrow & (NR - 1)) * k.slot_bytes, st);
    __syncthreads();
  }

  // combine the G threads of each channel in the order g = 0 .. G - 1, KCH accumulators per round (the ring is free:
  // the loop ended on a barrier); red[kk][g][pl] holds a channel pair
  float* const red = (float*)ring;
  float* const out = p.part + ((int64_t)(blockIdx.z * gridDim.y + blockIdx.y) * C + k.io.c0) * NACC;
  const int nent = k.io.cw * KCH;
#pragma unroll
  for (int rd = 0; rd < NACC / KCH; ++rd) {
    if (k.g < p.G) {
#pragma unroll
      for (int kk = 0; kk < KCH; ++kk) {
        const int t = rd * KCH + kk;
        float* dst = red + ((kk * p.G + k.g) * p.CP + k.pl) * 2;
        dst[0] = t < TAPS ? wa[t < TAPS ? t : 0] : ba;
        dst[1] = t < TAPS ? wb[t < TAPS ? t : 0] : bb;
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nent; e += THREADS) {
      const int ch = e / KCH, kk = e - ch * KCH;
      float s = 0.f;
      for (int g = 0; g < p.G; ++g) s += red[((kk * p.G + g) * p.CP) * 2 + ch];
      out[ch * NACC + rd * KCH + kk] = s;
    }
    __syncthreads();
  }
}

// dw[c][t] (t < 49) and db[c] (t = 49) = the sum of part[b][c][t] over b: 8 interleaved strides per entry, then
// those 8 in order.  32 entries per block.
__global__ __launch_bounds__(THREADS) void dwconv7_wgrad_reduce_kernel(const float* part, int NB, int C, float* dw,
                                                                       float* db, int accumulate) {
  __shared__ float sh[8][32];
  const int i = threadIdx.x & 31, j = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + i, ne = C * NACC;
  float s = 0.f;
  if (e < ne)
    for (int b = j; b < NB; b += 8) s += part[(int64_t)b * ne + e];
  sh[j][i] = s;
  __syncthreads();
  if (j != 0 || e >= ne) return;
  float t = sh[0][i];
#pragma unroll
  for (int jj = 1; jj < 8; ++jj) t += sh[jj][i];
  const int c = e / NACC, tap = e - c * NACC;
  float* dst = tap < TAPS ? dw + c * TAPS + tap : (db ? db + c : nullptr);
  if (dst) *dst = accumulate ? *dst + t : t;
}

static bool shape_ok(int N, int H, int W, int C) { return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0; }

static Args make_args(const Plan& q, int H, int W, int C) {
  Args a{};
  a.H = H, a.W = W, a.C = C, a.CP = q.CP, a.G = q.G, a.WT = q.WT, a.PS = q.PS, a.ntile = q.ntile, a.RB = q.RB;
  return a;
}

}  // namespace dwconv
}  // namespace dpe

using namespace dpe::dwconv;

extern "C" int dpe_dwconv7_fwd(const void* x, int x_f32, const uint16_t* w49, const float* bias, uint16_t* y, int N, int H,
                               int W, int C, hipStream_t st) {
  if (!shape_ok(N, H, W, C)) return 1;
  const Plan q = plan(N, H, W, C);
  if ((int64_t)q.nchunk * q.ntile > 65535) return 2;
  Args a = make_args(q, H, W, C);
  a.x = x, a.w = w49, a.bias = bias, a.y = y;
  const dim3 grid(q.nslab, q.nchunk * q.ntile, N);
  if (x_f32) hipLaunchKernelGGL(dwconv7_rows_kernel<true>, grid, dim3(THREADS), q.ring, st, a);
  else hipLaunchKernelGGL(dwconv7_rows_kernel<false>, grid, dim3(THREADS), q.ring, st, a);
  return (int)hipGetLastError();
}

extern "C" int64_t dpe_dwconv7_wgrad_blocks(int N, int H, int W, int C) {
  if (!shape_ok(N, H, W, C)) return 0;
  const Plan q = plan(N, H, W, C);
  return (int64_t)N * q.nchunk * q.ntile;
}

extern "C" int dpe_dwconv7_wgrad(const uint16_t* dy, const void* x, int x_f32, float* part, float* dw, float* db,
                                 int accumulate, int N, int H, int W, int C, hipStream_t st) {
  if (!shape_ok(N, H, W, C)) return 1;
  const Plan q = plan(N, H, W, C);
  const int64_t nb = (int64_t)N * q.nchunk * q.ntile;
  if ((int64_t)q.nchunk * q.ntile > 65535 || nb > INT32_MAX) return 2;
  Args a = make_args(q, H, W, C);
  a.x = x, a.w = dy, a.part = part;
  const dim3 grid(q.nslab, q.nchunk * q.ntile, N);
  const int lds = std::max(q.ring, COMBINE_BYTES);
  if (x_f32) hipLaunchKernelGGL(dwconv7_wgrad_kernel<true>, grid, dim3(THREADS), lds, st, a);
  else hipLaunchKernelGGL(dwconv7_wgrad_kernel<false>, grid, dim3(THREADS), lds, st, a);
  if (const int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(dwconv7_wgrad_reduce_kernel, dim3((C * NACC + 31) / 32), dim3(THREADS), 0, st, part, (int)nb, C, dw,
                     db, accumulate);
  return (int)hipGetLastError();
}
