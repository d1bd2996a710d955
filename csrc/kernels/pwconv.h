// Host-visible arguments of the streaming pointwise-conv kernel (pwconv.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dpe {

enum PwEpi : int {
  PW_FWD = 0,    // y = x . W^T; stats = BatchNorm-forward (sum, sum of squares) of the stored y
  PW_DGRAD = 1,  // y = x . W (+ residual [masked]); stats = BatchNorm-backward (sum dz, sum dz*(st_x - mean))
  PW_APPLY = 2,  // y = relu(BN(x . W^T) + residual): out_coef = the BN's [4][N] coefficients, known before the
                 // conv (Gram algebra, bngram.hip); the pre-BN tensor is never stored; out_bits = ReLU bits of y
  PW_DSUM = 3,   // PW_DGRAD with st_mask and no st_x: stats row 0 = sum dz only (row 1 left unwritten)
  PW_CAT = 4,    // y = relu(out_coef.scale * (x' . W^T) + res_coef.scale * (x2 . W2^T) + out_coef.shift + res_coef.shift)
                 // over the concatenated K = [x' | x2] (x' = relu(x * in_coef) or x; K = 2 cat_k2): a bottleneck's conv3 +
                 // BN3 and its 1x1 stride-1 downsample conv + BN_d in one pass, both BNs' coefficients known before the
                 // convs (Gram algebra); neither pre-BN tensor is stored; out_bits = ReLU bits of y
};

struct PwArgs {
  const uint16_t* x;         // [M][K] bf16 (forward: the conv input; data grad: dy)
  const uint16_t* w;         // PW_FWD: [N][K] (conv weight [Cout][Cin]); PW_DGRAD: [K][N] (the same tensor)
  uint16_t* y;               // [M][N] bf16
  float* stats;              // [2][N][row groups] partials, or nullptr
  const uint16_t* residual;  // PW_DGRAD: bf16 [M][N] added to y, or nullptr
  const uint8_t* res_mask;   // PW_DGRAD: ReLU bits of the residual's producer ([M][N/8]), or nullptr
  const uint16_t* st_x;      // PW_DGRAD BN backward: pre-BN input [M][N]; nullptr = no stats
  const float* st_coef;      // [4][N]: scale, shift, mean, invstd of that BatchNorm
  const uint8_t* st_mask;    // ReLU bits of the BN output ([M][N/8]); the stored y is then the masked dz
  int64_t M, N, K;
  int rg;                    // row groups (= partial columns), from dpe_pw_rowgroups
  const float* in_coef;      // PW_FWD: x is the pre-BN tensor; the operand is relu(x * in_coef[k] + in_coef[K + k])
  int res_h, res_w;          // PW_DGRAD, > 0: y is an [*, res_h, res_w] image and the residual is the compact
                             // [*, res_h/2, res_w/2] grid of a stride-2 1x1 conv's data grad, added at even (h, w) only
  const float* out_coef;     // PW_APPLY: [4][N] BN coefficients (scale, shift, ...) applied to the conv output
  const float* res_coef;     // PW_APPLY: the residual is BN'd first: bf16(residual * res_coef[n] + res_coef[N + n])
  uint8_t* out_bits;         // PW_APPLY: ReLU bits of y ([M][N/8]), or nullptr
  unsigned* sched;           // claim counters (HGEMM_SCHED_BYTES, zeroed, left zeroed) for the dynamic schedule,
                             // or nullptr: static (see dpe_pw_rowgroups)
  // PW_DSUM with the fused product P = y^T a2 (the BN3 Gram backward's dz3^T a2, from the rows this epilogue
  // stores): p_k2 in {64, 128} columns of p_src; 0 = none
  const uint16_t* p_src;     // [M][p_k2] bf16: the second operand's rows (the pre-BN h2, or a plain operand)
  const float* p_coef;       // [4][p_k2]: the operand is bf16(relu(p_src * scale + shift)); nullptr = plain
  float* p_slab;             // [rg][N][p_k2] fp32: one partial product per row group (dpe_pw_p_reduce sums them)
  int p_k2;
  // PW_CAT: the second K segment (plain operand), cat_k2 = K / 2 channels; x and w then hold K - cat_k2 channels
  const uint16_t* x2;        // [M][cat_k2] bf16
  const uint16_t* w2;        // [N][cat_k2] bf16
  int cat_k2;
  // PW_APPLY with the next block's conv1 formed from the rows this pass stores (K = 64, N = 256, a plain residual):
  // c1_next in {64, 128} output channels; 0 = none
  const uint16_t* w_next;    // [c1_next][N] bf16: the next conv1's weight
  uint16_t* y_next;          // [M][c1_next] bf16: h1 = y . w_next^T, rounded once
  float* stats_next;         // [2][c1_next][rg]: BatchNorm-forward (sum, sum of squares) of the stored h1, as PW_FWD's stats
  int c1_next;
};

// The concatenated-K data grad of the Gram-path BN3 backward (bngram.hip) on a streaming kernel:
//   y[M][N] = [dz | relu(h2 * s + t)] . Bcat + e,  N = K2 (the bottleneck width: 64 or 128), K1 = 4 N,
// with the BN2-backward partials (sum dz, sum dz*(h2 - mean)) of the stored y; mask and h2 from the raw h2
// tile the kernel already holds in LDS (the LDS-DMA implicit GEMM re-read h2 for its epilogue).
// coef == nullptr (and stats == nullptr): the second segment is a plain operand, y = [dz | h2] . Bcat + e with no
// partials (the downsample BN's Gram backward: h2 = the block input x).
struct PwCatArgs {
  const uint16_t* dz;     // [M][K1] bf16
  const uint16_t* h2;     // [M][K2] bf16, pre-BN2 (or the plain operand)
  const float* coef;      // BN2 [4][K2]: scale, shift, mean, invstd, or nullptr
  const uint16_t* bcat;   // [K1 + K2][N] bf16
  const float* ebias;     // [N]
  uint16_t* y;            // [M][N] bf16
  float* stats;           // [2][N][rg], or nullptr (with coef == nullptr)
  int64_t M;
  int rg;                 // blocks (= partial columns)
};

}  // namespace dpe

// Blocks (= partial columns) of the concatenated-K data grad for (M, K1, K2), 0: outside the kernel's envelope.
extern "C" int dpe_pw_cat_blocks(int64_t M, int64_t K1, int64_t K2);
extern "C" int dpe_pw_cat_launch(const dpe::PwCatArgs* args, int64_t K1, int64_t K2, hipStream_t stream);

// Row groups of the launch for (M, N, K, epi), or 0 outside the kernel's envelope
// (K in {64, 128, 256}, N a multiple of the block's column slice, N >= 2K).  With a CU budget in force
// (dpe_cu_reserve() > 0: collectives in flight) there are three times as many row groups as resident block
// rows and the last two thirds are claimed at run time (PwArgs::sched); otherwise one per resident block row.
extern "C" int dpe_pw_rowgroups(int64_t M, int64_t N, int64_t K, int epi);
extern "C" int dpe_pw_launch(const dpe::PwArgs* args, int epi, hipStream_t stream);

// PW_CAT: row groups of the launch for two segments of k2 channels each (K = 2 k2), or 0 outside its envelope
// (k2 in {64, 128}, N = 4 k2).  The launch is dpe_pw_launch with K = 2 k2, cat_k2 = k2 and rg from here.
extern "C" int dpe_pw_cat_fwd_rowgroups(int64_t M, int64_t N, int64_t k2);

// PW_DSUM with the fused product (PwArgs::p_src): row groups of that launch, or 0 outside its envelope
// ((K, k2) in {(64, 64), (128, 64), (128, 128)} inside PW_DSUM's own).  The launch is dpe_pw_launch with
// p_k2 = k2 and rg from here; dpe_pw_p_reduce then sums the slabs in row-group order: P[N][k2] fp32.
extern "C" int dpe_pw_p_rowgroups(int64_t M, int64_t N, int64_t K, int64_t k2);
// PW_APPLY with the next conv1 (PwArgs::w_next): row groups of that launch, or 0 outside its envelope (K = 64,
// N = 256, c1 in {64, 128}; static schedule only, so 0 while a CU budget is in force with the dynamic schedule on --
// the caller then makes the two separate calls).  The launch is dpe_pw_launch with c1_next = c1 and rg from here.
extern "C" int dpe_pw_next_rowgroups(int64_t M, int64_t N, int64_t K, int64_t c1);

extern "C" int dpe_pw_p_reduce(const float* slab, int rg, int64_t n, float* P, hipStream_t stream);
