// pybind11 bindings of the dense GEMM (Linear) and convolution ops.  Every entry point validates
// device / dtype / layout and fails loudly (no silent fallback), picks the
// launch configuration (tile shape, split-K) and enqueues on torch's current
// HIP stream, so the ops compose with the caching allocator and hipGraph
// capture (no host sync, no hipMalloc inside).
#include <algorithm>
#include <cstring>
#include <vector>

#include "../kernels/pwconv.h"
#include "gemm_plan.h"
#include "ops_common.h"

namespace dpe_ops {

// ------------------------------------------------- shared with bn.cpp (ops_common.h)
// DPE_IGEMM_DMA=0: forward-form convolutions stay on the register-staged kernel (A/B reference)
bool igemm_dma_on() { static const bool on = env_on("DPE_IGEMM_DMA", true); return on; }

dpe::IgemmArgs base_args() {
  dpe::IgemmArgs a;
  memset(&a, 0, sizeof(a));
  a.alpha = 1.f;
  return a;
}

dpe::HgemmArgs hargs() {
  dpe::HgemmArgs a;
  memset(&a, 0, sizeof(a));
  a.alpha = 1.f;
  a.splits = 1;
  return a;
}

dpe::ConvGeom geom(const Tensor& x, const Tensor& w, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw,
                   int64_t OH, int64_t OW) {
  dpe::ConvGeom g;
  g.N = (int)x.size(0); g.H = (int)x.size(1); g.W = (int)x.size(2); g.C = (int)x.size(3);
  g.K = (int)w.size(0); g.R = (int)w.size(1); g.S = (int)w.size(2);
  g.sh = (int)sh; g.sw = (int)sw; g.ph = (int)ph; g.pw = (int)pw; g.dh = (int)dh; g.dw = (int)dw;
  g.OH = (int)OH; g.OW = (int)OW;
  g.RR = g.R; g.SS = g.S;
  g.pr0 = 0; g.ps0 = 0; g.psh = 1; g.psw = 1;
  g.remap = 0; g.Hr = g.H; g.Wr = g.W; g.oa = 0; g.ob = 0;
  return g;
}

// DPE_PW_STREAM=0 / set_pw_stream(false): the write-heavy pointwise convs stay on the implicit-GEMM
// kernels (A/B reference and the equivalence tests)
static Toggle g_pw_stream("DPE_PW_STREAM");
bool pw_stream_on() { return g_pw_stream.on(); }

// Forward-form convolutions with taps (3x3, stride 1 or 2, and the stride-1 data grads run as forward
// convs of dy with the flipped filter) and >= 256 output channels on the persistent GEMM with an
// implicit-im2col A (hgemm.hip AC): its BK-64 ping-pong schedule ran the dense GEMMs of these shapes at
// 818-1,102 TF where the implicit-GEMM kernel ran them at 668-829 (profiles/conv_as_gemm_r3.jsonl);
// with 128 output channels the 256-wide tiles lose (481 vs 680 TF), so those stay.
// DPE_HGEMM_CONV=0 (or set_hgemm_conv(false)): the implicit-GEMM kernel (A/B, tests).
static int g_hgemm_conv = env_on("DPE_HGEMM_CONV", true) ? 1 : 0;
bool hgemm_conv_on() { return g_hgemm_conv != 0; }
// the weight-grad half (implicit-im2col B) separately: DPE_HGEMM_CONV_WGRAD=0/1 (A/B)
static int g_hgemm_conv_wgrad = env_on("DPE_HGEMM_CONV_WGRAD", true) ? 1 : 0;
bool hgemm_conv_wgrad_on() { return g_hgemm_conv_wgrad != 0; }

namespace {
void set_pw_stream(bool on) { g_pw_stream.set(on); }
void set_hgemm_conv(bool on) { g_hgemm_conv = on ? 1 : 0; }

// --------------------------------------------------------------- GEMM tiling
struct Cfg { int bm, bn, splits, k_split; };

Cfg pick_cfg(int64_t M, int64_t N, int64_t K, bool allow_split) {
  Cfg c{128, N <= 64 ? 64 : 128, 1, (int)((K + 31) / 32 * 32)};
  auto tiles = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
  const int64_t target = 512;  // >= 2 workgroups per CU on 256 CUs
  if (allow_split && K >= 32 * 64) {
    // split-K (weight-grad) GEMMs: big K, small output.  Keep the largest
    // tile (highest MFMA:LDS ratio) and let the K split supply parallelism.
    c.bm = M <= 64 ? 64 : 128;
    c.bn = N <= 64 ? 64 : 128;
    const int64_t t = tiles(c.bm, c.bn);
    const int64_t ksteps = (K + 31) / 32;
    // register-staged weight-grad tiles (1x1 with 128 channels): 512 blocks (768 / 1024 / 1536 measured
    // worse, docs/perf_notes.md); the LDS-DMA im2col weight-grad kernel re-derives its split (run_igemm)
    // (at the CU budget -- an overlapped RCCL collective holding `reserve` slots -- a slot fewer per
    // reserved workgroup, so the split still fits one resident wave: SURVEY §5.8 item 7)
    // (budget in force: two such rounds, as the LDS-DMA weight grads in run_igemm)
    const int64_t target_blocks =
        std::max<int64_t>(64, (dpe_cu_reserve() > 0 ? 2 : 1) * (2 * (int64_t)dpe_gemm::num_cus() - dpe_cu_reserve()));
    const int64_t per = dpe_cu_reserve() > 0 ? target_blocks / t : (target_blocks + t - 1) / t;
    int64_t splits = std::max<int64_t>(1, std::min<int64_t>(per, ksteps / 8));
    const int64_t kps = (ksteps + splits - 1) / splits;
    c.k_split = (int)(kps * 32);
    c.splits = (int)((ksteps + kps - 1) / kps);
    return c;
  }
  if (tiles(c.bm, c.bn) < target && M <= 64) c.bm = 64;
  if (tiles(c.bm, c.bn) < target && c.bn == 128 && c.bm == 128 && tiles(128, 64) <= tiles(64, 128)) c.bn = 64;
  if (tiles(c.bm, c.bn) < target && c.bm == 128) c.bm = 64;
  if (tiles(c.bm, c.bn) < target && c.bn == 128) c.bn = 64;
  if (allow_split) {
    const int64_t t = tiles(c.bm, c.bn);
    int64_t splits = (1024 + t - 1) / t;
    const int64_t ksteps = (K + 31) / 32;
    const int64_t max_splits = std::max<int64_t>(1, ksteps / 4);  // >= 4 K-steps per split
    splits = std::min(splits, max_splits);
    if (splits < 1) splits = 1;
    const int64_t kps = (ksteps + splits - 1) / splits;
    c.k_split = (int)(kps * 32);
    c.splits = (int)((ksteps + kps - 1) / kps);
  }
  return c;
}

// DPE_WGRAD_DMA=0: im2col weight grads on the register-staged kernel (documented fallback)
bool wgrad_dma_on() { static const bool on = env_on("DPE_WGRAD_DMA", true); return on; }
// 64x256 weight-grad tile: 1 = for the C <= 16 stem, 2 = also for C > 16 (test hook set_wgrad_wide;
// measured slower there: 388 -> 512 us on the 64->64 3x3), 0 = never
int g_wgrad_wide = 1;

// Tile of the LDS-DMA conv kernel: 0 auto, 1 128-tile (pick_cfg), 2 256x128, 3 256x256
// (8 waves; only where pick_cfg chose a 128-row tile, so BN partial layouts never change).
// Forced tiles are a test hook (set_conv_tile): every one is numerics-tested, only "auto" is timed.
int g_dma_tile = [] { const char* e = getenv("DPE_CONV_TILE"); return e ? atoi(e) : 0; }();  // (env: A/B runs)
int dma_tile_mode() { return g_dma_tile; }

void dma_tile(const dpe::IgemmArgs& a, int aload, int bload, int& bm, int& bn) {
  if (bm != 128) return;
  // (1x1 data grads, N-contiguous weights: the 256x128 8-wave tile measured slower at K >= 1024,
  // ResNet-50 37.77-37.82 vs 37.63-37.67 ms: they stay on the 128-row tiles)
  if (bload != dpe::B_DENSE_K) return;
  int mode = dma_tile_mode();
  const bool taps = aload == dpe::A_CONV_FWD && a.g.R * a.g.S > 1;
  if (a.N <= 64) {
    // N = 64 with K >= 256 (layer-1 3x3 forward / data grad, 1x1 256->64): 256x64 tile, 4 waves of
    // 64x64 on a 2-stage ring (40 KiB, 4 blocks/CU): 236 -> 229 / 227 -> 213 / 215 -> 203 us
    // (profiles/conv_w64_ab_r2.txt; a 3-stage ring's 60 KiB halved the blocks per CU: 296 / 271 us).
    // Not the C = 16 s2d stem (short K: 519 -> 539 us on 256x64 with the 2-stage ring).
    const bool stem = aload == dpe::A_CONV_FWD && a.g.C == 16;
    if (mode >= 2 || (mode == 0 && a.K >= 256 && !stem)) { bm = 256; bn = 64; }
    return;
  }
  if (mode == 0) {
    // measured (scripts/bench_convs.py, batch 512): 256x128 wins on 3x3 convs with K >= 576 and
    // on K >= 1024; 256x256 (one block per CU) loses on most ResNet-50 shapes
    mode = (a.K >= 1024 || (taps && a.K >= 576)) ? 2 : 1;
  }
  if (mode == 3 && a.N > 128) { bm = 256; bn = 256; }
  else if (mode >= 2 && a.N > 64) { bm = 256; bn = 128; }
}

// Strided data grads: the per-parity sub-GEMMs in one grid (igemm_dma_group_kernel) with DPE_PHASE_GROUP=1 or
// set_phase_group(true); default one launch per parity.  Measured neutral (ResNet-50 31.07-31.13 vs
// 31.10-31.16 ms/step; per shape 492 / 334 / 251 vs 487 / 329 / 232 us with the BN epilogue, layers 2 / 3 / 4:
// the shared dy rows and the single launch are not what the parity sub-GEMMs lose their time to)
bool g_phase_group = env_on("DPE_PHASE_GROUP", false);

// ---------------------------------------------------------- flipped filters
// The stride-1 / per-parity data grads run as forward convs of dy with flipped, transposed filters
// (conv_w_flipT).  A filter only changes when the optimizer (or a torch-side edit) rewrites the bf16 shadow,
// which bumps the weight epoch (set_weight_epoch, ops/_state.py).  The flipped copies are cached per (filter,
// tap subset) and, at the first request of a new epoch, ALL cached copies are refreshed in one launch (one
// instead of ~26 per ResNet-50 backward); a copy first requested in this epoch is flipped on its own.
struct FlipDescHost {
  const uint16_t* w;
  uint16_t* wt;
  int K, R, S, C, r0, rs, Rp, s0, ss, Sp;
};
struct FlipEntry {
  Tensor w, wt;
  FlipDescHost d;
  int64_t epoch;
};
std::vector<FlipEntry> g_flips;
int64_t g_weight_epoch = 0;
Tensor g_flip_desc, g_flip_start;  // device copies of the descriptor table (rebuilt when the set changes)
bool g_flip_table_dirty = true;
int g_flip_total = 0;

Tensor flipped(const Tensor& w, int K, int R, int S, int C, int r0, int rs, int Rp, int s0, int ss, int Sp) {
  static const bool cache_on = env_on("DPE_FLIP_CACHE", true);
  if (!cache_on) {
    Tensor wt = at::empty({C, Rp, Sp, K}, w.options());
    CHECK_RC(dpe_conv_w_flipT(bp(w), bpm(wt), K, R, S, C, r0, rs, Rp, s0, ss, Sp, cur_stream()), "conv_w_flipT");
    return wt;
  }
  if (!g_flips.empty() && g_flips.front().w.device() != w.device()) {
    // one device per table: the batched refresh launches on the current device's stream
    g_flips.clear();
    g_flip_desc = Tensor();
    g_flip_start = Tensor();
    g_flip_table_dirty = true;
  }
  FlipEntry* hit = nullptr;
  for (auto& e : g_flips)
    if (e.d.w == bp(w) && e.w.is_same(w) && e.d.K == K && e.d.R == R && e.d.S == S && e.d.C == C && e.d.r0 == r0 &&
        e.d.rs == rs && e.d.Rp == Rp && e.d.s0 == s0 && e.d.ss == ss && e.d.Sp == Sp) {
      hit = &e;
      break;
    }
  if (hit && hit->epoch == g_weight_epoch) return hit->wt;
  if (hit) {
    // a new epoch: refresh every cached copy at once.  This first stale request comes from the first
    // flipped-filter user of the backward pass; every other cached filter's layer back-propagates after it,
    // so none of them can have been stepped yet -- with DDP.overlap_optimizer a bucket is stepped only after
    // every reader of its parameters returned -- and all cached weights are current (one device: below)
    if (g_flip_table_dirty) {
      std::vector<int> start(g_flips.size() + 1, 0);
      std::vector<FlipDescHost> desc(g_flips.size());
      for (size_t i = 0; i < g_flips.size(); ++i) {
        desc[i] = g_flips[i].d;
        start[i + 1] = start[i] + dpe_flip_blocks(desc[i].K, desc[i].C, desc[i].Rp, desc[i].Sp);
      }
      TORCH_CHECK((int)sizeof(FlipDescHost) == dpe_flip_desc_bytes(), "FlipDesc ABI mismatch");
      auto u8 = at::TensorOptions().dtype(at::kByte);
      Tensor hd = at::empty({(int64_t)(desc.size() * sizeof(FlipDescHost))}, u8);
      memcpy(hd.data_ptr(), desc.data(), desc.size() * sizeof(FlipDescHost));
      Tensor hs = at::empty({(int64_t)start.size()}, at::TensorOptions().dtype(at::kInt));
      memcpy(hs.data_ptr(), start.data(), start.size() * sizeof(int));
      g_flip_desc = hd.to(w.device());
      g_flip_start = hs.to(w.device());
      g_flip_total = start.back();
      g_flip_table_dirty = false;
    }
    CHECK_RC(dpe_conv_w_flipT_multi(g_flip_desc.data_ptr(), (const int*)g_flip_start.data_ptr(), (int)g_flips.size(),
                                    g_flip_total, cur_stream()),
             "conv_w_flipT_multi");
    for (auto& e : g_flips) e.epoch = g_weight_epoch;
    return hit->wt;
  }
  if (g_flips.size() >= 256) {  // (models come and go in tests: bounded, nothing stale is kept alive)
    g_flips.clear();
    g_flip_desc = Tensor();
    g_flip_start = Tensor();
  }
  Tensor wt = at::empty({C, Rp, Sp, K}, w.options());
  CHECK_RC(dpe_conv_w_flipT(bp(w), bpm(wt), K, R, S, C, r0, rs, Rp, s0, ss, Sp, cur_stream()), "conv_w_flipT");
  g_flips.push_back(FlipEntry{w, wt, FlipDescHost{bp(w), bpm(wt), K, R, S, C, r0, rs, Rp, s0, ss, Sp}, g_weight_epoch});
  g_flip_table_dirty = true;
  return wt;
}

void run_igemm(dpe::IgemmArgs& a, int aload, int bload, int epi, bool allow_split, bool conv = false,
               bool deterministic = false, bool overwrite = false) {
  Cfg c = pick_cfg(a.M, a.N, a.K, allow_split && epi == dpe::EPI_ATOMIC_F32);
  a.k_split = c.k_split;
  // weight grads over an im2col B (3x3 / strided; split-K fp32 atomics): LDS-DMA kernel, measured 1.3-1.5x
  // faster (scripts/bench_convs.py) (DPE_WGRAD_DMA=0: the im2col ones register-staged)
  // the dense 1x1 ones (< 256 channels) too: on the LDS-DMA kernel since its round-5 changes, same-box
  // ResNet-50 31.42-31.47 vs 31.48-31.60 ms/step (3 alternating pairs; the register-staged tile measured
  // 10-15 % faster in round 1).  DPE_WGRAD_DMA_1X1=0: register-staged (A/B)
  static const bool dma_1x1 = env_on("DPE_WGRAD_DMA_1X1", true);
  if (conv && epi == dpe::EPI_ATOMIC_F32 && aload == dpe::A_DENSE_M &&
      ((igemm_dma_on() && wgrad_dma_on() && bload == dpe::B_CONV_WGRAD) ||
       (bload == dpe::B_DENSE_N && (a.b_coef || deterministic || (dma_1x1 && igemm_dma_on() && a.K % 32 == 0))))) {
    int bm = c.bm, bn = c.bn, splits = c.splits;
    {
      // ~3 resident 128x128 blocks per CU (4 fit): ResNet-50 step, alternating
      // (profiles/wgrad_blocks_ab_r2.txt, all split-K weight grads at one target): 256 -8 %, 384 -2.4 %,
      // 512 0, 768 +1.4-1.8 %, 1024 -0.5 %, 1536 -0.5 %, 2048 -1 %; 704-768 best of 640-896.  The
      // register-staged 1x1 tiles measured best at 512 and keep pick_cfg's split.
      // 3 per CU (768 on 256 CUs), less the slots an overlapped RCCL collective holds (CU budget,
      // comm.cpp): a split that needs more blocks than fit beside the collective's workgroups runs a
      // second, nearly empty wave (x1.56-1.60 per kernel next to 16 RCCL-sized workgroups,
      // profiles/cu_hog_probe_r3.txt in git history).  Rounded down, so tiles x splits <= the target.
      // With a CU budget in force the split targets TWO rounds of blocks: foreign workgroups do not take
      // our slots away (they fit beside them) but slow the CUs they share, and with one round the
      // slowest CU set the kernel's time (x1.27 next to 16 VALU-bound hogs, profiles/cu_hog_probe_r4.txt);
      // with two, the dispatcher gives those CUs fewer blocks.
      static const bool two_rounds = env_on("DPE_WGRAD_TWO_ROUNDS", true);
      const int rsv = dpe_cu_reserve();
      const int64_t dma_target = std::max<int64_t>(64, (rsv > 0 && two_rounds ? 2 : 1) * (3 * (int64_t)dpe_gemm::num_cus() - rsv));
      const int64_t t = (int64_t)((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn), ksteps = (a.K + 31) / 32;
      const int64_t rs = dpe_cu_reserve() > 0 ? dma_target / t : (dma_target + t - 1) / t;  // (unchanged at no reserve)
      const int64_t sp = std::max<int64_t>(1, std::min<int64_t>(rs, ksteps / 8));
      const int64_t kps = (ksteps + sp - 1) / sp;
      a.k_split = (int)(kps * 32);
      splits = (int)((ksteps + kps - 1) / kps);
    }
    if (c.bm == 64 && bload == dpe::B_CONV_WGRAD && a.N >= 256 && g_wgrad_wide && (a.g.C <= 16 || g_wgrad_wide > 1)) {
      // Cout = 64 with few channels per tap (the stem): 64x256 tile (4 waves across N), split-K
      // re-derived for its tile count.  Measured: stem 1167 -> 783 us; 64->64 3x3 388 -> 512 us
      // (2 instead of 4 blocks per CU), so C > 16 keeps 64x128 unless forced (set_wgrad_wide(2)).
      bn = 256;
      const int64_t t = (int64_t)((a.N + 255) / 256), ksteps = (a.K + 31) / 32;
      const int64_t sp = std::max<int64_t>(1, std::min<int64_t>((512 + t - 1) / t, ksteps / 8));
      const int64_t kps = (ksteps + sp - 1) / sp;
      a.k_split = (int)(kps * 32);
      splits = (int)((ksteps + kps - 1) / kps);
    }
    Tensor slab;
    if (deterministic && splits > 1) {
      // split partials stored to slabs, summed in split order below (no atomics: bitwise reproducible)
      slab = at::empty({(int64_t)splits * a.M * a.N}, at::TensorOptions().dtype(at::kFloat).device(at::kCUDA));
      a.slab = fp(slab);
    }
    if (overwrite && !slab.defined())  // atomics accumulate: start from zeros
      TORCH_CHECK(hipMemsetAsync(a.C, 0, (size_t)a.M * a.ldc * sizeof(float), cur_stream()) == hipSuccess, "memset");
    const int rc = dpe_igemm_wgrad_dma_launch(&a, bm, bn, bload, splits, cur_stream());
    a.slab = nullptr;
    TORCH_CHECK(rc == 0 || (!a.b_coef && !deterministic),
                "weight grad with BN on load / deterministic: outside the LDS-DMA kernel's envelope (rc=", rc, ")");
    static const bool skip_fin = [] {  // (timing diagnostic: gemm.cpp launch_planned)
      const bool on = env_on("DPE_AB_SKIP_FINALIZE", false);
      if (on) fprintf(stderr, "[dpe] DPE_AB_SKIP_FINALIZE=1: deterministic weight-grad splits are NOT reduced (timing only)\n");
      return on;
    }();
    if (rc == 0 && slab.defined() && !skip_fin) {
      dpe::HgemmArgs f;
      memset(&f, 0, sizeof(f));
      f.C = a.C; f.ws = fp(slab); f.M = a.M; f.N = a.N; f.ldc = a.ldc; f.splits = splits; f.alpha = 1.f;
      // overwrite: the split sum IS the result (the caller's buffer needs no zero fill)
      CHECK_RC(dpe_hgemm_finalize(&f, overwrite ? dpe::HE_F32 : dpe::HE_ACC_F32, cur_stream()), "weight-grad slab finalize");
    }
    a.k_split = c.k_split;  // (register-staged fallback uses pick_cfg's split)
    if (rc == 0) {
      const hipError_t e = hipGetLastError();
      TORCH_CHECK(e == hipSuccess, "igemm_wgrad_dma launch failed: ", hipGetErrorString(e));
      return;
    }
  }
  // LDS-DMA kernel where it measured faster (2-stage ring, batch 512, profiles/convs_bs512_*):
  //   im2col A (3x3 / strided), K-contiguous B: always;
  //   dense 1x1 forward (A_DENSE_K x B_DENSE_K): unless K and N are both 64 (store-bound);
  //   1x1 data grads (A_DENSE_K x B_DENSE_N): for 128 <= N <= 512 (8-27 % faster; N = 64 and
  //   N >= 1024 measured 2-10 % slower in round 1).
  // Since the round-2 kernel changes every forward-form role on the LDS-DMA kernel measures +0.2 %
  // on the ResNet-50 step (5 alternating pairs: +0.14 / +0.29 / +0.17 / +0.63 / -0.16 %,
  // profiles/dma_all_ab_r2.txt), so that is the default (the round-1 role table is gone).
  constexpr bool dma_all = true;
  bool dma_role = false;
  if (aload == dpe::A_CONV_FWD) dma_role = bload == dpe::B_DENSE_K || dma_all;
  else if (aload == dpe::A_DENSE_K && bload == dpe::B_DENSE_K) dma_role = dma_all || a.K >= 128 || a.N >= 256;
  else if (aload == dpe::A_DENSE_K && bload == dpe::B_DENSE_N) dma_role = dma_all || (a.N >= 128 && a.N <= 512);
  if (conv && c.splits == 1 && dma_role && igemm_dma_on()) {
    // convolutions whose A is an im2col / dense K-contiguous operand: LDS-DMA kernel
    // (same tile shape, so BatchNorm partial layouts are unchanged)
    int bm = c.bm, bn = c.bn;
    dma_tile(a, aload, bload, bm, bn);
    const int rc = dpe_igemm_dma_launch(&a, bm, bn, aload, bload, epi, cur_stream());
    if (rc == 0) {
      const hipError_t e = hipGetLastError();
      TORCH_CHECK(e == hipSuccess, "igemm_dma launch failed: ", hipGetErrorString(e));
      return;
    }
  }
  const int rc = dpe_igemm_launch(&a, c.bm, c.bn, aload, bload, epi, c.splits, cur_stream());
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "igemm launch failed: ", hipGetErrorString(e));
  TORCH_CHECK(rc == 0, "igemm: unsupported configuration (aload=", aload, " bload=", bload, " epi=", epi, ") rc=", rc);
}

// optional device scalar (f32, 1 element) multiplied into the GEMM alpha
const float* alpha_ptr_of(const c10::optional<Tensor>& t) {
  if (!has(t)) return nullptr;
  CHECK_GPU((*t)); CHECK_F32((*t));
  TORCH_CHECK(t->numel() == 1, "alpha tensor must have one element");
  return (const float*)t->data_ptr();
}

// -------------------------------------------------------------- dense GEMMs
// Every Linear GEMM runs on our MFMA kernels: the persistent hgemm kernel
// (csrc/kernels/hgemm.hip; tile / K split from the deterministic planner in
// bindings/gemm.cpp, identical on every rank, no timing) whenever the shape is
// inside its envelope (K % 64, 16-B aligned rows, N % 8 for bf16 outputs), and
// the 128-tile implicit-GEMM kernel otherwise (SimpleNet's K = 784 input, odd
// classifier widths).  There is no vendor-library arm.

// y[M,N] = act(x[M,K] @ w[N,K]^T + bias) (+ residual);  aux_out (act = GELU): pre-activation v
Tensor linear_fwd(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias, int64_t act, bool out_f32,
                  const c10::optional<Tensor>& residual, const c10::optional<Tensor>& out,
                  const c10::optional<Tensor>& aux_out) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_BF16(w); CHECK_CONTIG(w);
  TORCH_CHECK(x.stride(-1) == 1, "x must have unit inner stride");
  const int64_t K = x.size(-1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "linear: weight shape mismatch");
  TORCH_CHECK(K % 8 == 0, "linear: in_features must be a multiple of 8");
  Tensor x2 = x.reshape({-1, K});
  TORCH_CHECK(x2.stride(0) % 8 == 0, "x row stride must be a multiple of 8");
  const int64_t M = x2.size(0);
  auto sizes = x.sizes().vec();
  sizes.back() = N;
  Tensor y;
  if (has(out)) {
    y = *out;
    TORCH_CHECK(y.numel() == M * N && y.is_contiguous(), "linear: bad out tensor");
  } else {
    y = at::empty(sizes, x.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
  }
  const bool has_aux = has(aux_out);
  if (has_aux) {
    TORCH_CHECK(act == dpe::ACT_GELU && !out_f32, "linear: aux_out (pre-activation) is for bf16 GELU outputs");
    CHECK_BF16((*aux_out)); CHECK_CONTIG((*aux_out));
    TORCH_CHECK(aux_out->numel() == M * N, "linear: aux_out shape mismatch");
  }
  const bool bf16_res = has(residual) && !out_f32;
  if (K % 64 == 0 && N % 8 == 0 && !bf16_res && (out_f32 ? act == 0 : true)) {
    auto a = hargs();
    a.A = bp(x2); a.B = bp(w); a.C = y.data_ptr();
    a.M = (int)M; a.N = (int)N; a.K = (int)K;
    a.lda = x2.stride(0); a.ldb = K; a.ldc = N;
    a.bias = fpo(bias);
    a.act = (int)act;
    if (has_aux) a.aux_out = bpm(*aux_out);
    if (out_f32 && has(residual)) {
      CHECK_F32((*residual)); CHECK_CONTIG((*residual));
      TORCH_CHECK(residual->numel() == M * N, "residual shape mismatch");
      a.residual_f32 = (const float*)residual->data_ptr();
    }
    dpe_gemm::run(a, 1, 1, out_f32 ? dpe::HE_F32 : dpe::HE_BF16, true, out_f32 ? 4 : 2);
    return y;
  }
  TORCH_CHECK(!has_aux, "linear: aux_out needs K % 64 == 0 and N % 8 == 0");
  auto a = base_args();
  a.A = bp(x2); a.B = bp(w); a.C = y.data_ptr();
  a.M = (int)M; a.N = (int)N; a.K = (int)K;
  a.lda = x2.stride(0); a.ldb = K; a.ldc = N;
  a.bias = fpo(bias);
  a.act = (int)act;
  if (has(residual)) {
    CHECK_CONTIG((*residual));
    TORCH_CHECK(residual->numel() == M * N, "residual shape mismatch");
    if (out_f32) {
      CHECK_F32((*residual));
      a.residual_f32 = (const float*)residual->data_ptr();
    } else {
      CHECK_BF16((*residual));
      a.residual = bp(*residual);
    }
  }
  run_igemm(a, dpe::A_DENSE_K, dpe::B_DENSE_K, out_f32 ? dpe::EPI_F32 : dpe::EPI_BF16, false);
  return y;
}

// dx[M,K] = dy[M,N] @ w[N,K]  (alpha_t: device scalar; gelu_in: dx *= gelu'(gelu_in), the
// backward of a GELU whose pre-activation gelu_in [M,K] produced this layer's input)
Tensor linear_dgrad(const Tensor& dy, const Tensor& w, const c10::optional<Tensor>& residual,
                    const c10::optional<Tensor>& alpha_t, const c10::optional<Tensor>& gelu_in) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_BF16(w); CHECK_CONTIG(w); CHECK_CONTIG(dy);
  const int64_t N = w.size(0), K = w.size(1);
  TORCH_CHECK(dy.size(-1) == N, "linear_dgrad: shape mismatch");
  TORCH_CHECK(N % 8 == 0 && K % 8 == 0, "linear_dgrad: features must be multiples of 8");
  const int64_t M = dy.numel() / N;
  auto sizes = dy.sizes().vec();
  sizes.back() = K;
  Tensor dx = at::empty(sizes, dy.options());
  const bool has_res = has(residual);
  const bool has_gelu = has(gelu_in);
  if (has_gelu) {
    CHECK_BF16((*gelu_in)); CHECK_CONTIG((*gelu_in));
    TORCH_CHECK(gelu_in->numel() == M * K, "linear_dgrad: gelu_in shape mismatch");
  }
  if (N % 64 == 0 && !has_res) {
    auto a = hargs();
    a.A = bp(dy); a.B = bp(w); a.C = dx.data_ptr();
    a.M = (int)M; a.N = (int)K; a.K = (int)N;
    a.lda = N; a.ldb = K; a.ldc = K;
    a.alpha_ptr = alpha_ptr_of(alpha_t);
    if (has_gelu) { a.act = dpe::HACT_GELU_BWD; a.aux_in = bp(*gelu_in); }
    dpe_gemm::run(a, 1, 0, dpe::HE_BF16, true, 2);
    return dx;
  }
  TORCH_CHECK(!has_gelu, "linear_dgrad: gelu_in needs out_features % 64 == 0 and no residual");
  auto a = base_args();
  a.A = bp(dy); a.B = bp(w); a.C = dx.data_ptr();
  a.M = (int)M; a.N = (int)K; a.K = (int)N;
  a.lda = N; a.ldb = K; a.ldc = K;
  if (has_res) { CHECK_BF16((*residual)); CHECK_CONTIG((*residual)); a.residual = bp(*residual); }
  a.alpha_ptr = alpha_ptr_of(alpha_t);
  run_igemm(a, dpe::A_DENSE_K, dpe::B_DENSE_N, dpe::EPI_BF16, false);
  return dx;
}

// dw[N,K] (+)= alpha * dy[M,N]^T @ x[M,K]   (fp32 accumulate into dw, e.g. a DDP bucket view).
// dy may be column-padded (row stride ldy >= N, ldy % 8 == 0, pad columns zero): then N need not be a
// multiple of 8 (vocab-padded LM head: N = 50257, ldy = 50304).
// overwrite: dw = alpha dy^T x instead of dw += (the step's first writer of a gradient whose stale
// contents were not zeroed, ops/_state.py grad_fresh); the bias gradient always accumulates.
void linear_wgrad(const Tensor& dy, const Tensor& x, Tensor& dw, double alpha, const c10::optional<Tensor>& alpha_t,
                  const c10::optional<Tensor>& dbias, int64_t fin_stream, bool overwrite) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_BF16(x); CHECK_CONTIG(dy); CHECK_CONTIG(x); CHECK_F32(dw); CHECK_CONTIG(dw);
  const int64_t N = dw.size(0), K = dw.size(1), ldy = dy.size(-1);
  TORCH_CHECK(ldy >= N && x.size(-1) == K && dy.numel() / ldy == x.numel() / K, "linear_wgrad: shape mismatch");
  TORCH_CHECK(ldy % 8 == 0 && K % 8 == 0, "linear_wgrad: dy row stride and in_features must be multiples of 8");
  const int64_t M = dy.numel() / ldy;
  if (M % 64 == 0) {
    // TN: A = dy^T (M-contiguous), B = x (N-contiguous).  The loads of A stop at a_dim = round8(N) (hgemm.hip
    // stage_setup clamps every 16-B chunk to it): the pad columns [N, a_dim) are read (zero by the contract above), the
    // columns [a_dim, ldy) are never read and need no fill
    auto a = hargs();
    a.A = bp(dy); a.B = bp(x); a.C = dw.data_ptr();
    a.M = (int)N; a.N = (int)K; a.K = (int)M;
    a.lda = ldy; a.ldb = K; a.ldc = K;
    a.a_dim = (int)((N + 7) / 8 * 8);
    a.alpha = (float)alpha;
    a.alpha_ptr = alpha_ptr_of(alpha_t);
    if (has(dbias)) {
      // bias gradient from the same launch: row sums of dy^T taken from the A fragments (hgemm BG)
      CHECK_F32((*dbias)); CHECK_CONTIG((*dbias));
      TORCH_CHECK(dbias->numel() == N, "linear_wgrad: dbias must have out_features elements");
      a.dbias = fp(*dbias);
    }
    dpe_gemm::run(a, 0, 0, overwrite ? dpe::HE_F32 : dpe::HE_ACC_F32, true, 4, (hipStream_t)(uintptr_t)fin_stream);
    return;
  }
  if (overwrite) dw.zero_();  // the split-K fallback below accumulates with atomics
  if (has(dbias)) {
    CHECK_F32((*dbias)); CHECK_CONTIG((*dbias));
    TORCH_CHECK(dbias->numel() == N, "linear_wgrad: dbias must have out_features elements");
    TORCH_CHECK(alpha == 1.0 && !alpha_ptr_of(alpha_t), "linear_wgrad: dbias with M % 64 != 0 needs alpha == 1");
    CHECK_RC(dpe_colsum(dy.data_ptr(), M, (int)N, ldy, fp(*dbias), 1, 1, cur_stream()), "colsum");
  }
  auto a = base_args();
  a.A = bp(dy); a.B = bp(x); a.C = dw.data_ptr();
  a.M = (int)N; a.N = (int)K; a.K = (int)M;
  a.lda = ldy; a.ldb = K; a.ldc = K;
  a.alpha = (float)alpha;
  a.alpha_ptr = alpha_ptr_of(alpha_t);
  run_igemm(a, dpe::A_DENSE_M, dpe::B_DENSE_N, dpe::EPI_ATOMIC_F32, true);
}

// ------------------------------------------------------------------- conv
// DPE_ROWCONV=0 / set_rowconv(false): the 64-channel 3x3 convs stay on the implicit-GEMM tiles
Toggle g_rowconv("DPE_ROWCONV");
bool rowconv_on() { return g_rowconv.on(); }
void set_rowconv(bool on) { g_rowconv.set(on); }
// DPE_ROW_WGRAD=0 / set_row_wgrad(false): their weight grads stay on the im2col weight-grad tile
Toggle g_row_wgrad("DPE_ROW_WGRAD");
bool row_wgrad_on() { return g_row_wgrad.on(); }
void set_row_wgrad(bool on) { g_row_wgrad.set(on); }
// 3x3 / stride 1 / pad 1 / dilation 1, 64 -> 64 channels, W <= 64: the row-walking kernel's envelope
bool rowconv_geom(const dpe::ConvGeom& g) {
  return rowconv_on() && g.C == 64 && g.K == 64 && g.R == 3 && g.S == 3 && g.sh == 1 && g.sw == 1 && g.ph == 1 &&
         g.pw == 1 && g.dh == 1 && g.dw == 1 && g.OH == g.H && g.OW == g.W &&
         dpe_conv3x3_rows_blocks(g.N, g.H, g.W) > 0;
}

// DPE_STEM=0 / set_stem_kernel(false): the s2d stem conv stays on the implicit-GEMM tile
Toggle g_stem("DPE_STEM");
bool stem_on() { return g_stem.on(); }
void set_stem_kernel(bool on) { g_stem.set(on); }

// DPE_WGRAD_HGEMM=0 / set_wgrad_hgemm(false): every conv weight grad stays on the implicit GEMM
Toggle g_wgrad_hgemm("DPE_WGRAD_HGEMM");
bool wgrad_hgemm_on() { return g_wgrad_hgemm.on(); }
void set_wgrad_hgemm(bool on) { g_wgrad_hgemm.set(on); }

// DPE_HGEMM_CONV_1X1S=0: the strided 1x1 convs (bottleneck downsamples) stay on the implicit-GEMM kernel (A/B)
bool g_hgemm_conv_1x1s = env_on("DPE_HGEMM_CONV_1X1S", true);
bool hconv_ok(const dpe::ConvGeom& f, int64_t nout) {
  // 1x1 only when strided (a stride-1 1x1 conv is a dense GEMM, routed elsewhere) and at >= 512 input
  // channels: the layer-3/4 downsamples 185 -> 169 and 145 -> 139 us, the layer-2 one (K = 256) slower
  // there, 287 vs 272 us (scripts/bench_down_fwd.py, profiles/down_fwd_r4.jsonl)
  const bool one = f.R * f.S == 1 && (f.sh > 1 || f.sw > 1) && f.ph == 0 && f.pw == 0 && f.C >= 512 && g_hgemm_conv_1x1s;
  if (!g_hgemm_conv || (f.R * f.S <= 1 && !one) || f.R * f.S > 32 || f.C < 64 || (f.C & (f.C - 1)) || nout < 256 || nout % 8) return false;
  const int64_t abytes = (((int64_t)f.N * f.H * f.W * f.C) + ((int64_t)f.ph * f.W + f.pw) * f.C) * 2;
  return abytes < (1ll << 31) - 4096 && (int64_t)f.N * f.OH * f.OW < (1ll << 31);
}
// y [M = N*OH*OW][nout] = im2col(x) . w^T with the BN-forward sums (act HACT_BNF) or the BN-backward
// partials of dL/d relu(BN(st_x)) (HACT_BNB) or neither (ACT_NONE); stats sized by the plan.  Returns
// false when no plan fits.
bool run_hconv(const uint16_t* x, const uint16_t* w, uint16_t* y, const dpe::ConvGeom& f, int64_t nout, int act,
               const Tensor& like, Tensor* stats, const uint16_t* st_x, const float* st_coef) {
  const int64_t M = (int64_t)f.N * f.OH * f.OW, K = (int64_t)f.R * f.S * f.C;
  int pcols = 0;
  const auto pl = dpe_gemm::plan_bnb(M, nout, K, 1, 1, &pcols);
  if (pl.cfg < 0 || pl.splits != 1 || pcols <= 0) return false;
  auto h = hargs();
  h.A = x; h.B = w; h.C = y;
  h.M = (int)M; h.N = (int)nout; h.K = (int)K;
  h.lda = K; h.ldb = K; h.ldc = nout;
  h.conv = 1; h.conv_g = f; h.conv_smagic = (65536 + f.S - 1) / f.S;
  h.act = act;
  if (act != dpe::ACT_NONE) {
    *stats = at::empty({2, nout, pcols}, like.options().dtype(at::kFloat));
    h.col_stats = fp(*stats); h.stats_ld = pcols;
    h.st_x = st_x; h.st_coef = st_coef;
    dpe_gemm::run_bnb(h, pl, 1, 1);
  } else {
    dpe_gemm::launch_plain(h, pl, 1, 1);
  }
  return true;
}

// DPE_HGEMM_DGRAD=0: 1x1 convs (data grads, and forwards with BN statistics) with K >= 1024 stay on the
// implicit-GEMM kernel (A/B reference)
bool hgemm_dgrad_on() { static const bool on = env_on("DPE_HGEMM_DGRAD", true); return on; }

bool is_pointwise(const dpe::ConvGeom& g) {
  return g.R == 1 && g.S == 1 && g.sh == 1 && g.sw == 1 && g.ph == 0 && g.pw == 0;
}

// x NHWC bf16 [N,H,W,C], w [K,R,S,C] bf16 -> y NHWC [N,OH,OW,K]
// in_coef: x is the pre-BN tensor of a BatchNorm+ReLU whose output was never stored ([4][C] coefficients;
// relu(x * scale + shift) is applied on load) -- only on the row-walking 64-channel 3x3 kernel
std::vector<Tensor> conv_fwd(const Tensor& x, const Tensor& w, std::vector<int64_t> stride, std::vector<int64_t> pad,
                             std::vector<int64_t> dil, bool want_stats, const c10::optional<Tensor>& bias,
                             const c10::optional<Tensor>& in_coef) {
  CHECK_GPU(x); CHECK_BF16(x); CHECK_BF16(w); CHECK_CONTIG(x); CHECK_CONTIG(w);
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4 && x.size(3) == w.size(3), "conv: NHWC x / KRSC w shape mismatch");
  TORCH_CHECK(x.size(3) % 8 == 0 && w.size(0) % 8 == 0, "conv: channels must be multiples of 8");
  TORCH_CHECK(pad.size() == 2 || pad.size() == 4, "conv: pad is [ph, pw] or [top, left, bottom, right]");
  const int64_t H = x.size(1), W = x.size(2), R = w.size(1), S = w.size(2);
  const int64_t pb = pad.size() == 4 ? pad[2] : pad[0], pr = pad.size() == 4 ? pad[3] : pad[1];
  const int64_t OH = (H + pad[0] + pb - dil[0] * (R - 1) - 1) / stride[0] + 1;
  const int64_t OW = (W + pad[1] + pr - dil[1] * (S - 1) - 1) / stride[1] + 1;
  Tensor y = at::empty({x.size(0), OH, OW, w.size(0)}, x.options());
  auto g = geom(x, w, stride[0], stride[1], pad[0], pad[1], dil[0], dil[1], OH, OW);
  auto a = base_args();
  a.g = g;
  a.A = bp(x); a.B = bp(w); a.C = y.data_ptr();
  a.M = (int)(x.size(0) * OH * OW); a.N = g.K; a.K = (int)(R * S * g.C);
  a.lda = g.C; a.ldb = a.K; a.ldc = g.K;
  a.bias = fpo(bias);
  Tensor stats;
  // the space-to-depth ResNet stem (16 channels, 4x4 / s1 / pad 2-2-1-1 -> 64): row-walking
  // kernel with the filter in VGPRs and each input row loaded once (csrc/kernels/stem.hip)
  const int stem_nb = (stem_on() && g.C == 16 && g.K == 64 && R == 4 && S == 4 && g.sh == 1 && g.sw == 1 && g.ph == 2 &&
                       g.pw == 2 && pb == 1 && pr == 1 && g.dh == 1 && g.dw == 1 && OH == H && OW == W && !a.bias)
                          ? dpe_stem_blocks(g.N, g.H, g.W) : 0;
  const float* icoef = fpo(in_coef);
  const int pw_rg_in = (pw_stream_on() && is_pointwise(g) && !a.bias) ? dpe_pw_rowgroups(a.M, a.N, a.K, dpe::PW_FWD) : 0;
  TORCH_CHECK(!icoef || (rowconv_geom(g) && pb == 1 && pr == 1 && !a.bias) || pw_rg_in > 0,
              "conv_fwd: in_coef (BN+ReLU on load) needs the row-walking 64-channel 3x3 kernel or the streaming "
              "pointwise kernel");
  if (rowconv_geom(g) && pb == 1 && pr == 1 && !a.bias) {
    // 64-channel 3x3 (layer 1 conv2): row-walking kernel, filter in VGPRs (csrc/kernels/rowconv.hip)
    const int nb = dpe_conv3x3_rows_blocks(g.N, g.H, g.W);
    if (want_stats) stats = at::empty({2, g.K, nb}, x.options().dtype(at::kFloat));
    CHECK_RC(dpe_conv3x3_rows_launch(bp(x), bp(w), bpm(y), want_stats ? fp(stats) : nullptr, nullptr, nullptr, g.N, g.H,
                                     g.W, nb, 0, icoef, cur_stream()),
             "conv3x3 rows fwd");
    return {y, stats};
  }
  if (stem_nb > 0) {
    if (want_stats) stats = at::empty({2, g.K, stem_nb}, x.options().dtype(at::kFloat));
    CHECK_RC(dpe_stem_launch(bp(x), bp(w), bpm(y), want_stats ? fp(stats) : nullptr, g.N, g.H, g.W, cur_stream()),
             "stem conv");
    return {y, stats};
  }
  // write-heavy pointwise convs (K <= 256, N >= 2K; the bottleneck conv3 shapes): persistent
  // streaming kernel (csrc/kernels/pwconv.hip), BN partials per row group.
  const int pw_rg = (pw_stream_on() && is_pointwise(g) && !a.bias) ? dpe_pw_rowgroups(a.M, a.N, a.K, dpe::PW_FWD) : 0;
  if (pw_rg > 0) {
    if (want_stats) stats = at::empty({2, g.K, pw_rg}, x.options().dtype(at::kFloat));
    dpe::PwArgs pa{};
    pa.x = bp(x); pa.w = bp(w); pa.y = bpm(y); pa.stats = want_stats ? fp(stats) : nullptr;
    pa.in_coef = icoef;
    pa.M = a.M; pa.N = a.N; pa.K = a.K; pa.rg = pw_rg; pa.sched = dpe_gemm::sched_buffer(cur_stream());
    CHECK_RC(dpe_pw_launch(&pa, dpe::PW_FWD, cur_stream()), "pw_stream fwd");
    return {y, stats};
  }
  // 1x1 stride-1 forward at depth >= 1024 (layers 3-4 conv1) with BN statistics: the persistent GEMM's
  // BN-forward-partials epilogue (hgemm.hip HACT_BNF; its GEMM alone 60-71 vs 79-89 us,
  // profiles/pw_vs_hgemm_r3.jsonl)
  // DPE_HG_BNF_MINK (default 1024): the smallest depth routed there (with >= 256 output channels below 1024)
  static const int bnf_min_k = [] { const char* e = getenv("DPE_HG_BNF_MINK"); return e ? atoi(e) : 1024; }();
  if (want_stats && is_pointwise(g) && !a.bias && !icoef && hgemm_dgrad_on() && a.K >= bnf_min_k &&
      (a.K >= 1024 || a.N >= 256) && a.K % 64 == 0 && a.N % 8 == 0) {
    int pcols = 0;
    const auto pl = dpe_gemm::plan_bnb(a.M, a.N, a.K, 1, 1, &pcols);
    if (pl.cfg >= 0 && pcols > 0) {
      stats = at::empty({2, g.K, pcols}, x.options().dtype(at::kFloat));
      auto h = hargs();
      h.A = bp(x); h.B = bp(w); h.C = y.data_ptr();
      h.M = a.M; h.N = a.N; h.K = a.K;
      h.lda = a.K; h.ldb = a.K; h.ldc = a.N;
      h.act = dpe::HACT_BNF;
      h.col_stats = fp(stats); h.stats_ld = pcols;
      dpe_gemm::run_bnb(h, pl, 1, 1);
      return {y, stats};
    }
  }
  if (!is_pointwise(g) && !a.bias && !icoef && hconv_ok(g, a.N) &&
      run_hconv(bp(x), bp(w), bpm(y), g, a.N, want_stats ? dpe::HACT_BNF : dpe::ACT_NONE, x, &stats, nullptr, nullptr))
    return {y, stats};
  if (want_stats) {
    // [2][K][tilesM] partial (sum, sumsq) per output channel and M-tile, reduced by bn_fwd_train
    const Cfg c = pick_cfg(a.M, a.N, a.K, false);
    const int64_t tilesM = (a.M + c.bm - 1) / c.bm;
    stats = at::empty({2, g.K, tilesM}, x.options().dtype(at::kFloat));
    a.col_stats = fp(stats);
  }
  run_igemm(a, is_pointwise(g) ? dpe::A_DENSE_K : dpe::A_CONV_FWD, dpe::B_DENSE_K, dpe::EPI_BF16, false, true);
  return {y, stats};
}

// dx NHWC [N,H,W,C] = conv_transpose(dy, w); optional residual added into dx.
// With bn_x/bn_coef (dx is dL/d relu(BN(bn_x))), the epilogue also emits the
// BatchNorm-backward partials [2][C][tiles] (sum dz, sum dz*(x-mean)).

// DPE_DGRAD_FWD=0: stride-1 data grads on the transposed-filter loaders (A/B reference)
bool dgrad_as_fwd() { static const bool on = env_on("DPE_DGRAD_FWD", true); return on; }

// dy of a data / weight grad must be the forward conv's output for this input size: OH, OW from H, W, stride, pad
// and dilation as conv_fwd computes them.  pad [top, left, bottom, right]: exactly that size.  pad [ph, pw] names
// the top / left pad only (the bottom / right one is whatever produced dy: the s2d stem passes [2, 2] for its
// [2, 2, 1, 1]), so the size with a bottom / right pad of ph / pw or of one less is accepted.  A dy of any other
// size would be walked with a pixel grid that is not the conv's (wrong gradients, nothing to catch them downstream).
void check_dy_shape(const char* op, const Tensor& dy, const dpe::ConvGeom& g, const std::vector<int64_t>& pad) {
  TORCH_CHECK(pad.size() == 2 || pad.size() == 4, op, ": pad is [ph, pw] or [top, left, bottom, right]");
  TORCH_CHECK(g.sh >= 1 && g.sw >= 1 && g.dh >= 1 && g.dw >= 1 && g.ph >= 0 && g.pw >= 0, op, ": bad stride / pad / dilation");
  auto out = [](int64_t in, int64_t p0, int64_t p1, int64_t d, int64_t k, int64_t s) -> int64_t {
    const int64_t span = in + p0 + p1 - d * (k - 1) - 1;
    return span < 0 ? 0 : span / s + 1;
  };
  const bool four = pad.size() == 4;
  const int64_t oh_hi = out(g.H, g.ph, four ? pad[2] : g.ph, g.dh, g.R, g.sh), oh_lo = four ? oh_hi : out(g.H, g.ph, std::max(g.ph - 1, 0), g.dh, g.R, g.sh);
  const int64_t ow_hi = out(g.W, g.pw, four ? pad[3] : g.pw, g.dw, g.S, g.sw), ow_lo = four ? ow_hi : out(g.W, g.pw, std::max(g.pw - 1, 0), g.dw, g.S, g.sw);
  TORCH_CHECK(dy.dim() == 4 && dy.size(1) >= std::max<int64_t>(1, oh_lo) && dy.size(1) <= oh_hi &&
                  dy.size(2) >= std::max<int64_t>(1, ow_lo) && dy.size(2) <= ow_hi,
              op, ": dy is [", dy.size(0), ", ", dy.size(1), ", ", dy.size(2), ", ", dy.size(3), "] but an input of ", g.H, " x ",
              g.W, " with a ", g.R, " x ", g.S, " filter, stride (", g.sh, ", ", g.sw, "), pad (", g.ph, ", ", g.pw,
              four ? ", ...)" : ")", ", dilation (", g.dh, ", ", g.dw, ") gives OH in [", oh_lo, ", ", oh_hi, "], OW in [", ow_lo,
              ", ", ow_hi, "]");
}

void conv_wgrad(const Tensor& dy, const Tensor& x, Tensor& dw, std::vector<int64_t> stride, std::vector<int64_t> pad,
                std::vector<int64_t> dil, double alpha, const c10::optional<Tensor>& in_coef, int64_t fin_stream,
                bool deterministic, bool overwrite);

std::vector<Tensor> conv_dgrad_impl(const Tensor& dy, const Tensor& w, std::vector<int64_t> xshape,
                                    std::vector<int64_t> stride, std::vector<int64_t> pad, std::vector<int64_t> dil,
                                    const c10::optional<Tensor>& residual, const c10::optional<Tensor>& bn_x,
                                    const c10::optional<Tensor>& bn_coef, const Tensor* acc_into = nullptr,
                                    const c10::optional<Tensor>& bn_mask = c10::nullopt,
                                    const c10::optional<Tensor>& residual_mask = c10::nullopt,
                                    bool res_stride2 = false, const c10::optional<Tensor>& sum_mask = c10::nullopt,
                                    const c10::optional<Tensor>& p_src = c10::nullopt,
                                    const c10::optional<Tensor>& p_coef = c10::nullopt) {
  TORCH_CHECK(!has(p_src) || has(sum_mask), "conv_dgrad: p_src needs sum_mask");
  TORCH_CHECK(!has(p_coef) || has(p_src), "conv_dgrad: p_coef needs p_src");
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_BF16(w); CHECK_CONTIG(dy); CHECK_CONTIG(w);
  // acc_into: dx += dgrad in place (the epilogue reads each element as its residual
  // right before overwriting it); parities no tap reaches are left untouched.
  Tensor dx = acc_into ? *acc_into : at::empty(xshape, dy.options());
  auto g = geom(dx, w, stride[0], stride[1], pad[0], pad[1], dil[0], dil[1], dy.size(1), dy.size(2));
  TORCH_CHECK(dy.size(3) == g.K && dy.size(0) == g.N, "conv_dgrad: dy shape mismatch");
  check_dy_shape("conv_dgrad", dy, g, pad);
  auto a = base_args();
  a.g = g;
  a.A = bp(dy); a.B = bp(w); a.C = dx.data_ptr();
  a.M = g.N * g.H * g.W; a.N = g.C; a.K = g.R * g.S * g.K;
  a.lda = g.K; a.ldb = g.C; a.ldc = g.C;
  if (has(residual)) {
    CHECK_BF16((*residual)); CHECK_CONTIG((*residual));
    a.residual = bp(*residual);
    // the data-grad residual (a block's dz3 pass-through) is at its last use
    static const bool nt = env_on("DPE_EPI_NT", true);
    a.res_nt = nt ? 1 : 0;
    if (has(residual_mask)) {
      // residual = dy of a BN + residual + ReLU output: masked by that output's bits in the epilogue
      CHECK_CONTIG((*residual_mask));
      TORCH_CHECK(residual_mask->scalar_type() == at::kByte && residual_mask->numel() * 8 == residual->numel() &&
                      residual->size(-1) % 8 == 0,
                  "conv_dgrad: residual_mask must be uint8 mask bits [.., C/8] of the residual");
      a.res_mask = (const uint8_t*)residual_mask->data_ptr();
    }
  }
  if (acc_into) {
    TORCH_CHECK(!a.residual && !has(bn_x), "conv_dgrad_acc: no residual / BN with accumulate");
    CHECK_BF16(dx); CHECK_CONTIG(dx);
    TORCH_CHECK(dx.sizes().vec() == xshape, "conv_dgrad_acc: dx shape mismatch");
    a.residual = bp(dx);
  }
  const bool want_bn = has(bn_x);
  if (want_bn) {
    CHECK_BF16((*bn_x)); CHECK_CONTIG((*bn_x)); CHECK_F32((*bn_coef));
    TORCH_CHECK(bn_x->sizes() == dx.sizes(), "conv_dgrad: bn_x must have dx's shape");
    TORCH_CHECK(bn_coef->numel() == 4 * g.C, "conv_dgrad: bn_coef must be [4][C]");
    a.st_x = bp(*bn_x);
    a.st_coef = fp(*bn_coef);
    if (has(bn_mask)) {
      // BN + residual + ReLU: ReLU-mask bits of the saved block output (bn_apply want_mask),
      // dx stored already masked
      CHECK_CONTIG((*bn_mask));
      TORCH_CHECK(bn_mask->scalar_type() == at::kByte && bn_mask->numel() * 8 == dx.numel() && g.C % 8 == 0,
                  "conv_dgrad: bn_mask must be uint8 mask bits [N,H,W,C/8] of dx's shape");
      a.st_mask = (const uint8_t*)bn_mask->data_ptr();
    }
  }
  Tensor part;
  // write-heavy pointwise data grads (a bottleneck's conv1: K = Cout <= 256, N = Cin >= 2K), with the
  // residual / BN-backward epilogue: streaming kernel (pwconv.hip), BN partials per row group
  const int pw_rg = (pw_stream_on() && is_pointwise(g) && !acc_into) ? dpe_pw_rowgroups(a.M, a.N, a.K, dpe::PW_DGRAD) : 0;
  if (res_stride2) {
    // residual = the compact data grad of a downsample block's stride-2 1x1 conv ([N, H/2, W/2, C]),
    // added at even (h, w) by the streaming kernel's epilogue
    TORCH_CHECK(a.residual && !a.res_mask && (pw_rg > 0 || has(sum_mask)) &&
                    g.H % 2 == 0 && g.W % 2 == 0,
                "conv_dgrad: residual_stride2 needs the streaming pointwise data grad, even H / W, no residual mask");
    TORCH_CHECK(residual->dim() == 4 && residual->size(0) == g.N && residual->size(1) == g.H / 2 &&
                    residual->size(2) == g.W / 2 && residual->size(3) == g.C,
                "conv_dgrad: residual_stride2 residual must be [N, H/2, W/2, C]");
  }
  if (has(sum_mask)) {
    // BN + residual + ReLU backward partials WITHOUT the pre-BN input (Gram algebra, bngram.hip): dx stored
    // masked by the output's bits, partials row 0 = sum dz (row 1 unwritten); streaming kernel only
    TORCH_CHECK(!want_bn && !acc_into && is_pointwise(g), "conv_dgrad: sum_mask excludes bn_x / accumulate");
    CHECK_CONTIG((*sum_mask));
    TORCH_CHECK(sum_mask->scalar_type() == at::kByte && sum_mask->numel() * 8 == dx.numel() && g.C % 8 == 0,
                "conv_dgrad: sum_mask must be uint8 mask bits [N,H,W,C/8] of dx's shape");
    // p_src (+ p_coef): also P = dx^T a2 [C, 1, 1, k2] fp32, a2 = relu(BN(p_src)) or p_src itself -- the BN3 Gram
    // backward's dz3^T a2, formed by the epilogue that stores dx (inside dpe_pw_p_rowgroups' envelope; outside
    // it the deterministic weight grad over the stored dx)
    int64_t k2 = 0;
    int rgp = 0;
    if (has(p_src)) {
      CHECK_GPU((*p_src)); CHECK_BF16((*p_src)); CHECK_CONTIG((*p_src));
      TORCH_CHECK(p_src->dim() == 4 && p_src->size(0) == g.N && p_src->size(1) == g.H && p_src->size(2) == g.W,
                  "conv_dgrad: p_src must be [N, H, W, k2] over dx's pixels");
      k2 = p_src->size(3);
      if (has(p_coef)) {
        CHECK_F32((*p_coef)); CHECK_CONTIG((*p_coef));
        TORCH_CHECK(p_coef->numel() == 4 * k2, "conv_dgrad: p_coef must be [4][k2]");
      }
      rgp = pw_stream_on() ? dpe_pw_p_rowgroups(a.M, a.N, a.K, k2) : 0;
    }
    const int rg = rgp > 0 ? rgp : (pw_stream_on() ? dpe_pw_rowgroups(a.M, a.N, a.K, dpe::PW_DSUM) : 0);
    TORCH_CHECK(rg > 0, "conv_dgrad: sum_mask needs the streaming pointwise data grad");
    dpe::PwArgs pa{};
    pa.x = bp(dy); pa.w = bp(w); pa.y = bpm(dx);
    pa.residual = a.residual; pa.res_mask = a.res_mask;
    if (res_stride2) { pa.res_h = g.H; pa.res_w = g.W; }
    pa.st_mask = (const uint8_t*)sum_mask->data_ptr();
    pa.M = a.M; pa.N = a.N; pa.K = a.K; pa.rg = rg; pa.sched = dpe_gemm::sched_buffer(cur_stream());
    part = at::empty({2, g.C, rg}, dy.options().dtype(at::kFloat));
    pa.stats = fp(part);
    Tensor slab;
    if (rgp > 0) {
      slab = at::empty({rg, g.C, k2}, dy.options().dtype(at::kFloat));
      pa.p_src = bp(*p_src);
      pa.p_coef = has(p_coef) ? fp(*p_coef) : nullptr;
      pa.p_slab = fp(slab);
      pa.p_k2 = (int)k2;
    }
    CHECK_RC(dpe_pw_launch(&pa, dpe::PW_DSUM, cur_stream()), "pw_stream dgrad (sum dz)");
    if (has(p_src)) {
      Tensor P = at::empty({g.C, 1, 1, k2}, dy.options().dtype(at::kFloat));
      if (rgp > 0) CHECK_RC(dpe_pw_p_reduce(fp(slab), rg, (int64_t)g.C * k2, fp(P), cur_stream()), "pw_stream P reduce");
      else conv_wgrad(dx, *p_src, P, {1, 1}, {0, 0}, {1, 1}, 1.0, p_coef, 0, true, true);
      return {dx, part, P};
    }
    return {dx, part};
  }
  if (pw_rg > 0) {
    dpe::PwArgs pa{};
    pa.x = bp(dy); pa.w = bp(w); pa.y = bpm(dx);
    pa.residual = a.residual; pa.res_mask = a.res_mask;
    if (res_stride2) { pa.res_h = g.H; pa.res_w = g.W; }
    pa.st_x = a.st_x; pa.st_coef = a.st_coef; pa.st_mask = a.st_mask;
    pa.M = a.M; pa.N = a.N; pa.K = a.K; pa.rg = pw_rg; pa.sched = dpe_gemm::sched_buffer(cur_stream());
    if (want_bn) {
      part = at::empty({2, g.C, pw_rg}, dy.options().dtype(at::kFloat));
      pa.stats = fp(part);
    }
    CHECK_RC(dpe_pw_launch(&pa, dpe::PW_DGRAD, cur_stream()), "pw_stream dgrad");
    return {dx, part};
  }
  // 1x1 data grads at depth >= 1024 (layers 3-4: conv3's) with the plain BN-backward epilogue: the
  // persistent GEMM (NN layout, hgemm.hip HACT_BNB) -- its GEMM alone 73 vs 112-118 us for layer 3's conv3
  // data grad (profiles/pw_vs_hgemm_r3.jsonl); ResNet-50 37.73-37.76 vs 37.81-37.88 ms/step.  At K = 512
  // (layer 2) it measured +0.3 ms/step, so that depth stays on the implicit GEMM.
  if (is_pointwise(g) && !a.residual && !a.res_mask && !a.st_mask && !acc_into && !res_stride2 && want_bn &&
      hgemm_dgrad_on() && a.K >= 1024 && a.K % 64 == 0 && g.C % 8 == 0) {
    int pcols = 0;
    const auto pl = dpe_gemm::plan_bnb(a.M, g.C, a.K, 1, 0, &pcols);
    if (pl.cfg >= 0 && pcols > 0) {
      part = at::empty({2, g.C, pcols}, dy.options().dtype(at::kFloat));
      auto h = hargs();
      h.A = bp(dy); h.B = bp(w); h.C = dx.data_ptr();
      h.M = a.M; h.N = g.C; h.K = a.K;
      h.lda = g.K; h.ldb = g.C; h.ldc = g.C;
      h.col_stats = fp(part); h.st_x = a.st_x; h.st_coef = a.st_coef; h.stats_ld = pcols;
      dpe_gemm::run_bnb(h, pl, 1, 0);
      return {dx, part};
    }
  }
  auto tiles_of = [&](int64_t M, int64_t K) { const Cfg c = pick_cfg(M, g.C, K, false); return (M + c.bm - 1) / c.bm; };
  if (!is_pointwise(g) && g.sh == 1 && g.sw == 1 && g.dh == 1 && g.dw == 1 && dgrad_as_fwd()) {
    // Stride-1 data grad as a forward conv: dx = conv(dy, flipT(w), pad R-1-p) on the
    // forward loaders (K-contiguous filter, im2col gather of dy).
    Tensor wt = flipped(w, g.K, g.R, g.S, g.C, 0, 1, g.R, 0, 1, g.S);
    auto f = geom(dy, wt, 1, 1, g.R - 1 - g.ph, g.S - 1 - g.pw, 1, 1, g.H, g.W);
    if (rowconv_geom(f) && !acc_into && !a.residual && !a.st_mask) {
      // 64-channel 3x3 data grad (layer 1): the row-walking forward kernel over dy with the flipped
      // filter; BN-backward partials per block
      const int nb = dpe_conv3x3_rows_blocks(f.N, f.H, f.W);
      if (want_bn) part = at::empty({2, g.C, nb}, dy.options().dtype(at::kFloat));
      CHECK_RC(dpe_conv3x3_rows_launch(bp(dy), bp(wt), bpm(dx), want_bn ? fp(part) : nullptr, a.st_x, a.st_coef, f.N, f.H,
                                       f.W, nb, want_bn ? 1 : 0, nullptr, cur_stream()),
               "conv3x3 rows dgrad");
      return {dx, part};
    }
    if (!acc_into && !a.residual && !a.st_mask && !a.res_mask && hconv_ok(f, g.C) &&
        run_hconv(bp(dy), bp(wt), bpm(dx), f, g.C, want_bn ? dpe::HACT_BNB : dpe::ACT_NONE, dy, &part, a.st_x, a.st_coef))
      return {dx, part};
    auto b = a;
    b.g = f;
    b.B = bp(wt);
    b.lda = g.K; b.ldb = a.K; b.ldc = g.C;
    if (want_bn) {
      const int64_t t = tiles_of(b.M, b.K);
      part = at::empty({2, g.C, t}, dy.options().dtype(at::kFloat));
      b.col_stats = fp(part);
      b.stats_ld = (int)t;
    }
    run_igemm(b, dpe::A_CONV_FWD, dpe::B_DENSE_K, want_bn ? dpe::EPI_BF16_BNB : dpe::EPI_BF16, false, true);
  } else if (is_pointwise(g) || (g.sh == 1 && g.sw == 1)) {
    if (want_bn) {
      const int64_t t = tiles_of(a.M, a.K);
      part = at::empty({2, g.C, t}, dy.options().dtype(at::kFloat));
      a.col_stats = fp(part);
      a.stats_ld = (int)t;
    }
    const int epi = want_bn ? dpe::EPI_BF16_BNB : dpe::EPI_BF16;
    if (is_pointwise(g)) run_igemm(a, dpe::A_DENSE_K, dpe::B_DENSE_N, epi, false, true);
    else run_igemm(a, dpe::A_CONV_DGRAD, dpe::B_CONV_DGRAD, epi, false, true);
  } else {
    // Strided: one stride-1 sub-GEMM per output parity (a, b) over only the
    // taps that reach it -- no MFMA work on structural zeros.  A parity with
    // no taps is a K = 0 GEMM that stores zeros (+ residual).
    TORCH_CHECK(g.dh == 1 && g.dw == 1, "strided dgrad with dilation is not supported");
    std::vector<dpe::IgemmArgs> subs;
    std::vector<bool> sub_fwd;
    std::vector<Tensor> phase_w;  // keeps the per-parity filters alive until the launches are queued
    int64_t total_tiles = 0;
    for (int pa = 0; pa < g.sh; ++pa) {
      for (int pb = 0; pb < g.sw; ++pb) {
        dpe::ConvGeom v = g;
        const int r0 = (pa + g.ph) % g.sh, s0 = (pb + g.pw) % g.sw;
        const int Rp = g.R > r0 ? (g.R - r0 + g.sh - 1) / g.sh : 0;
        const int Sp = g.S > s0 ? (g.S - s0 + g.sw - 1) / g.sw : 0;
        const int Hp = (g.H - pa + g.sh - 1) / g.sh, Wp = (g.W - pb + g.sw - 1) / g.sw;
        if (Hp <= 0 || Wp <= 0) continue;
        if (acc_into && (g.R <= r0 || g.S <= s0)) continue;  // no taps: dx += 0
        v.H = Hp; v.W = Wp; v.R = Rp; v.S = Sp;
        v.sh = 1; v.sw = 1;
        v.ph = (pa + g.ph - r0) / g.sh;  // oh = hh + ph' - t
        v.pw = (pb + g.pw - s0) / g.sw;
        v.pr0 = r0; v.ps0 = s0; v.psh = g.sh; v.psw = g.sw;
        v.remap = 1; v.Hr = g.H; v.Wr = g.W; v.oa = pa; v.ob = pb;
        auto b = a;
        b.g = v;
        b.M = g.N * Hp * Wp;
        b.K = Rp * Sp * g.K;
        b.stats_off = (int)total_tiles;
        total_tiles += tiles_of(b.M, b.K);
        bool fwd_form = false;
        if (Rp > 0 && Sp > 0 && dgrad_as_fwd()) {
          // this parity as a forward conv of dy with its own flipped tap subset:
          // oh = hh + ph' - t = hh - (Rp-1-ph') + (Rp-1-t)
          Tensor wt = flipped(w, g.K, g.R, g.S, g.C, r0, g.sh, Rp, s0, g.sw, Sp);
          phase_w.push_back(wt);
          auto f = geom(dy, wt, 1, 1, Rp - 1 - v.ph, Sp - 1 - v.pw, 1, 1, Hp, Wp);
          f.remap = 2; f.Hr = g.H; f.Wr = g.W; f.oa = pa; f.ob = pb; f.psh = g.sh; f.psw = g.sw;
          b.g = f;
          b.B = bp(wt);
          b.lda = g.K; b.ldb = b.K;
          fwd_form = true;
        }
        subs.push_back(b);
        sub_fwd.push_back(fwd_form);
      }
    }
    if (want_bn) part = at::empty({2, g.C, total_tiles}, dy.options().dtype(at::kFloat));
    const int epi = want_bn ? dpe::EPI_BF16_BNB : dpe::EPI_BF16;
    for (auto& b : subs)
      if (want_bn) { b.col_stats = fp(part); b.stats_ld = (int)total_tiles; }
    // g_phase_group: all parities in one grid (igemm_dma_group_kernel), on the first (shortest-K) parity's
    // tile -- one launch instead of four, an XCD's neighbouring blocks holding the four parities of the same
    // dy rows (measured neutral: off by default)
    bool grouped = false;
    if (g_phase_group && igemm_dma_on() && subs.size() > 1 && subs.size() <= (size_t)dpe::IGEMM_GROUP_MAX &&
        std::all_of(sub_fwd.begin(), sub_fwd.end(), [](bool f) { return f; })) {
      const Cfg c0 = pick_cfg(subs[0].M, subs[0].N, subs[0].K, false);
      int bm = c0.bm, bn = c0.bn;
      dma_tile(subs[0], dpe::A_CONV_FWD, dpe::B_DENSE_K, bm, bn);
      for (auto& b : subs) b.k_split = (int)((b.K + 31) / 32 * 32);
      grouped = dpe_igemm_dma_group_launch(subs.data(), (int)subs.size(), bm, bn, dpe::A_CONV_FWD, dpe::B_DENSE_K, epi,
                                           cur_stream()) == 0;
      if (grouped) {
        const hipError_t e = hipGetLastError();
        TORCH_CHECK(e == hipSuccess, "igemm_dma group launch failed: ", hipGetErrorString(e));
      }
    }
    for (size_t i = 0; i < subs.size() && !grouped; ++i) {
      auto& b = subs[i];
      if (sub_fwd[i]) run_igemm(b, dpe::A_CONV_FWD, dpe::B_DENSE_K, epi, false, true);
      else run_igemm(b, dpe::A_CONV_DGRAD, dpe::B_CONV_DGRAD, epi, false, true);
    }
  }
  return {dx, part};
}

void conv_dgrad_acc(const Tensor& dy, const Tensor& w, Tensor& dx, std::vector<int64_t> stride, std::vector<int64_t> pad,
                    std::vector<int64_t> dil) {
  conv_dgrad_impl(dy, w, dx.sizes().vec(), stride, pad, dil, c10::nullopt, c10::nullopt, c10::nullopt, &dx);
}

Tensor conv_dgrad(const Tensor& dy, const Tensor& w, std::vector<int64_t> xshape, std::vector<int64_t> stride,
                  std::vector<int64_t> pad, std::vector<int64_t> dil, const c10::optional<Tensor>& residual,
                  const c10::optional<Tensor>& residual_mask) {
  return conv_dgrad_impl(dy, w, xshape, stride, pad, dil, residual, c10::nullopt, c10::nullopt, nullptr, c10::nullopt,
                         residual_mask)[0];
}

// dw [K,R,S,C] fp32 (+)= alpha * dy^T (x) im2col(x)
// in_coef: as conv_fwd's (x pre-BN, BN+ReLU applied on load; row-walking 64-channel 3x3 kernel only)
void conv_wgrad(const Tensor& dy, const Tensor& x, Tensor& dw, std::vector<int64_t> stride, std::vector<int64_t> pad,
                std::vector<int64_t> dil, double alpha, const c10::optional<Tensor>& in_coef, int64_t fin_stream,
                bool deterministic, bool overwrite) {
  CHECK_GPU(dy); CHECK_BF16(dy); CHECK_BF16(x); CHECK_CONTIG(dy); CHECK_CONTIG(x); CHECK_F32(dw); CHECK_CONTIG(dw);
  auto g = geom(x, dw, stride[0], stride[1], pad[0], pad[1], dil[0], dil[1], dy.size(1), dy.size(2));
  TORCH_CHECK(dy.size(3) == g.K && dy.size(0) == g.N, "conv_wgrad: dy shape mismatch");
  check_dy_shape("conv_wgrad", dy, g, pad);
  auto a = base_args();
  a.g = g;
  a.A = bp(dy); a.B = bp(x); a.C = dw.data_ptr();
  a.M = g.K; a.N = g.R * g.S * g.C; a.K = g.N * g.OH * g.OW;
  a.lda = g.K; a.ldb = g.C; a.ldc = a.N;
  a.alpha = (float)alpha;
  // 64 -> 64 3x3 (ResNet layer 1): the row-walking weight-grad kernel (rowconv.hip)
  const float* icoef = fpo(in_coef);
  const int row_nb = rowconv_geom(g) ? dpe_wgrad3x3_rows_blocks(g.N, g.H, g.W) : 0;  // (depends on the CU budget)
  const bool row = row_nb > 0;
  if (icoef && !row) {
    // 1x1 weight grad over a pre-BN input: the LDS-DMA weight-grad kernel applies BN + ReLU to its
    // B fragments (b_coef); outside that kernel's envelope there is no such path
    TORCH_CHECK(is_pointwise(g), "conv_wgrad: in_coef needs a 1x1 conv or the row-walking 64-channel 3x3 kernel");
    a.b_coef = icoef;
    run_igemm(a, dpe::A_DENSE_M, dpe::B_DENSE_N, dpe::EPI_ATOMIC_F32, true, true, deterministic, overwrite);
    return;
  }
  const bool hgemm_1x1 = wgrad_hgemm_on() && is_pointwise(g) && a.K % 64 == 0 && g.K >= 256 && g.C >= 256 &&
                         g.K % 8 == 0 && g.C % 8 == 0;
  // a plain 1x1 below the persistent GEMM's widths with deterministic: the LDS-DMA weight grad's slab form
  // (run_igemm handles overwrite there; outside that kernel's envelope it is an error)
  const bool det_1x1 = deterministic && is_pointwise(g) && !hgemm_1x1 && !row;
  if (overwrite && !hgemm_1x1 && !det_1x1)  // the accumulating kernels below: start from zeros
    TORCH_CHECK(hipMemsetAsync(dw.data_ptr(), 0, dw.numel() * sizeof(float), cur_stream()) == hipSuccess, "memset");
  if (row && (row_wgrad_on() || icoef)) {
    auto scratch = at::empty({dpe_wgrad3x3_rows_scratch(row_nb)}, dw.options());
    CHECK_RC(dpe_wgrad3x3_rows_launch(bp(x), bp(dy), fp(dw), fp(scratch), g.N, g.H, g.W, row_nb, (float)alpha, icoef,
                                      cur_stream()),
             "wgrad3x3_rows");
    return;
  }
  // the s2d stem (16 channels, 4x4 / s1 / pad 2-2-1-1 -> 64): the row-walking weight grad (stem.hip)
  static const bool stem_wg_env = env_on("DPE_STEM_WGRAD", true);
  if (stem_on() && stem_wg_env && g.C == 16 && g.K == 64 && g.R == 4 && g.S == 4 && g.sh == 1 && g.sw == 1 && g.ph == 2 && g.pw == 2 &&
      g.dh == 1 && g.dw == 1 && g.OH == g.H && g.OW == g.W && dpe_stem_wgrad_scratch(g.N, g.H, g.W) > 0) {
    auto scratch = at::empty({dpe_stem_wgrad_scratch(g.N, g.H, g.W)}, dw.options());
    CHECK_RC(dpe_stem_wgrad_launch(bp(x), bp(dy), fp(dw), fp(scratch), g.N, g.H, g.W, (float)alpha, cur_stream()),
             "stem wgrad");
    return;
  }
  // 1x1 stride-1 weight grads with both channel counts >= 256 (ResNet layers 3-4 and the 512->256
  // entry of layer 3: 53 GFLOP over a few output tiles) are a plain TN GEMM over the pixels: the
  // persistent hgemm kernel with the planner's K split and a deterministic slab finalize, as
  // linear_wgrad.  With 128 channels the TN layout's only tile (256x256) wastes half its MFMAs and
  // the implicit GEMM is faster (profiles/wgrad_hgemm_ab_r2.txt).
  if (hgemm_1x1) {
    auto h = hargs();
    h.A = bp(dy); h.B = bp(x); h.C = dw.data_ptr();
    h.M = a.M; h.N = a.N; h.K = a.K;
    h.lda = g.K; h.ldb = g.C; h.ldc = g.C;
    h.a_dim = (int)((g.K + 7) / 8 * 8);
    h.alpha = (float)alpha;
    dpe_gemm::run(h, 0, 0, overwrite ? dpe::HE_F32 : dpe::HE_ACC_F32, true, 4, (hipStream_t)(uintptr_t)fin_stream);
    return;
  }
  // 3x3 weight grads with >= 256 output channels (layers 3-4): the persistent GEMM's TN layout with an
  // implicit-im2col B (hgemm.hip CV = 2); dense TN GEMMs of these shapes ran at 846-960 TF where the
  // LDS-DMA im2col weight grad ran them at 648-748 (profiles/wgrad_as_gemm_r4.jsonl).  Split-K partials
  // in slabs summed in a fixed order (no atomics).  Not with BN-on-load inputs (none at these shapes).
  if (g_hgemm_conv && g_hgemm_conv_wgrad && !is_pointwise(g) && g.K >= 256 && g.K % 8 == 0 && g.C >= 8 && (g.C & (g.C - 1)) == 0 &&
      a.K % 64 == 0 && a.K < (1 << 24) && g.R * g.S <= 32 &&
      (((int64_t)g.N * g.H * g.W * g.C) + ((int64_t)g.ph * g.W + g.pw) * g.C) * 2 < (1ll << 31) - 4096) {
    auto h = hargs();
    h.A = bp(dy); h.B = bp(x); h.C = dw.data_ptr();
    h.M = a.M; h.N = a.N; h.K = a.K;
    h.lda = g.K; h.ldb = a.N; h.ldc = a.N;
    h.alpha = (float)alpha;
    h.conv = 2; h.conv_g = g; h.conv_smagic = (65536 + g.S - 1) / g.S;
    dpe_gemm::run_conv_wgrad(h, (hipStream_t)(uintptr_t)fin_stream);
    return;
  }
  if (det_1x1) {
    TORCH_CHECK(igemm_dma_on(), "conv_wgrad: a deterministic 1x1 weight grad needs the LDS-DMA kernel");
    run_igemm(a, dpe::A_DENSE_M, dpe::B_DENSE_N, dpe::EPI_ATOMIC_F32, true, true, true, overwrite);
    return;
  }
  run_igemm(a, dpe::A_DENSE_M, is_pointwise(g) ? dpe::B_DENSE_N : dpe::B_CONV_WGRAD, dpe::EPI_ATOMIC_F32, true, true);
}

}  // namespace

void register_conv(pybind11::module& m) {
  namespace py = pybind11;
  m.def("linear_fwd", &linear_fwd, py::arg("x"), py::arg("w"), py::arg("bias") = py::none(), py::arg("act") = 0,
        py::arg("out_f32") = false, py::arg("residual") = py::none(), py::arg("out") = py::none(),
        py::arg("aux_out") = py::none());
  m.def("linear_dgrad", &linear_dgrad, py::arg("dy"), py::arg("w"), py::arg("residual") = py::none(),
        py::arg("alpha_t") = py::none(), py::arg("gelu_in") = py::none());
  m.def("linear_wgrad", &linear_wgrad, py::arg("dy"), py::arg("x"), py::arg("dw"), py::arg("alpha") = 1.0,
        py::arg("alpha_t") = py::none(), py::arg("dbias") = py::none(), py::arg("fin_stream") = 0,
        py::arg("overwrite") = false,
        "dw (+)= alpha dy^T x (+ db += alpha colsum(dy)); fin_stream: run a K-split's slab reduction on that HIP "
        "stream (the caller orders dw's consumers after it); overwrite: dw = instead of dw +=");
  m.def("conv_fwd", &conv_fwd, py::arg("x"), py::arg("w"), py::arg("stride"), py::arg("pad"), py::arg("dil"),
        py::arg("want_stats") = false, py::arg("bias") = py::none(), py::arg("in_coef") = py::none());
  m.def("row_bn_on_load", [](std::vector<int64_t> xs, std::vector<int64_t> ws, std::vector<int64_t> stride,
                             std::vector<int64_t> pad, std::vector<int64_t> dil) {
          // the row-walking 64-channel 3x3 kernels (fwd + wgrad) take the pre-BN input (in_coef)
          if (xs.size() != 4 || ws.size() != 4 || stride.size() != 2 || pad.size() != 2 || dil.size() != 2) return false;
          dpe::ConvGeom g{};
          g.N = (int)xs[0]; g.H = (int)xs[1]; g.W = (int)xs[2]; g.C = (int)xs[3];
          g.K = (int)ws[0]; g.R = (int)ws[1]; g.S = (int)ws[2];
          g.sh = (int)stride[0]; g.sw = (int)stride[1]; g.ph = (int)pad[0]; g.pw = (int)pad[1];
          g.dh = (int)dil[0]; g.dw = (int)dil[1];
          g.OH = (g.H + 2 * g.ph - g.dh * (g.R - 1) - 1) / g.sh + 1;
          g.OW = (g.W + 2 * g.pw - g.dw * (g.S - 1) - 1) / g.sw + 1;
          return ws[3] == xs[3] && rowconv_geom(g) && dpe_wgrad3x3_rows_blocks(g.N, g.H, g.W) > 0;
        }, py::arg("x_shape"), py::arg("w_shape"), py::arg("stride"), py::arg("pad"), py::arg("dil"));
  m.def("pw_bn_on_load", [](std::vector<int64_t> xs, int64_t cout) {
          // a 1x1 / stride-1 conv over a pre-BN input [N, H, W, C]: the streaming pointwise forward and the
          // LDS-DMA weight grad (K = pixels % 32, M = Cout, N = C) take the BN coefficients (in_coef)
          if (xs.size() != 4) return false;
          const int64_t M = xs[0] * xs[1] * xs[2], C = xs[3];
          static const int cmax = [] { const char* e = getenv("DPE_PW_BNIN_CMAX"); return e ? atoi(e) : 128; }();
          return pw_stream_on() && (C == 64 || C == 128) && C <= cmax && cout % 8 == 0 && M % 32 == 0 &&
                 dpe_pw_rowgroups(M, cout, C, dpe::PW_FWD) > 0;
        }, py::arg("x_shape"), py::arg("cout"));
  m.def("pw_dgrad_strided_residual_ok", [](std::vector<int64_t> xshape, int64_t k) {
          // a downsample block's conv1 data grad (1x1, K = k -> N = xshape[3]) on the streaming kernel,
          // which can take the stride-2 branch's compact data grad as its residual
          if (xshape.size() != 4 || xshape[1] % 2 || xshape[2] % 2 || !pw_stream_on()) return false;
          return dpe_pw_rowgroups(xshape[0] * xshape[1] * xshape[2], xshape[3], k, dpe::PW_DGRAD) > 0;
        }, py::arg("xshape"), py::arg("k"));
  m.def("pw_dgrad_fused_p_ok", [](std::vector<int64_t> xshape, int64_t k, int64_t k2) {
          // conv_dgrad_bn(..., sum_mask, p_src) of a 1x1 conv k -> xshape[3] forms P = dx^T a2 (k2 columns) in the
          // streaming data grad's epilogue (else: by the deterministic weight grad over the stored dx)
          if (xshape.size() != 4 || !pw_stream_on()) return false;
          return dpe_pw_p_rowgroups(xshape[0] * xshape[1] * xshape[2], xshape[3], k, k2) > 0;
        }, py::arg("xshape"), py::arg("k"), py::arg("k2"));
  m.def("conv_dgrad_acc", &conv_dgrad_acc, py::arg("dy"), py::arg("w"), py::arg("dx"), py::arg("stride"), py::arg("pad"),
        py::arg("dil"), "dx += data grad of conv(w) in place (parities without taps untouched)");
  m.def("conv_dgrad_bn", [](const Tensor& dy, const Tensor& w, std::vector<int64_t> xshape, std::vector<int64_t> stride,
                            std::vector<int64_t> pad, std::vector<int64_t> dil, const c10::optional<Tensor>& residual,
                            const c10::optional<Tensor>& bn_x, const c10::optional<Tensor>& bn_coef,
                            const c10::optional<Tensor>& bn_mask, const c10::optional<Tensor>& residual_mask,
                            bool residual_stride2, const c10::optional<Tensor>& sum_mask,
                            const c10::optional<Tensor>& p_src, const c10::optional<Tensor>& p_coef) {
          return conv_dgrad_impl(dy, w, xshape, stride, pad, dil, residual, bn_x, bn_coef, nullptr, bn_mask, residual_mask,
                                 residual_stride2, sum_mask, p_src, p_coef);
        }, py::arg("dy"), py::arg("w"), py::arg("xshape"), py::arg("stride"),
        py::arg("pad"), py::arg("dil"), py::arg("residual") = py::none(), py::arg("bn_x") = py::none(),
        py::arg("bn_coef") = py::none(), py::arg("bn_mask") = py::none(), py::arg("residual_mask") = py::none(),
        py::arg("residual_stride2") = false, py::arg("sum_mask") = py::none(), py::arg("p_src") = py::none(),
        py::arg("p_coef") = py::none(),
        "with sum_mask and p_src (+ p_coef): a third result P = dx^T relu(BN(p_src)) [C, 1, 1, k2] fp32 (fixed order); "
        "data grad; with bn_x/bn_coef also the BN-backward partials of the BN+ReLU that produced the conv input; "
        "with bn_mask (BN + residual + ReLU) the mask is bn_mask > 0 and dx is stored masked");
  m.def("conv_dgrad", &conv_dgrad, py::arg("dy"), py::arg("w"), py::arg("xshape"), py::arg("stride"), py::arg("pad"),
        py::arg("dil"), py::arg("residual") = py::none(), py::arg("residual_mask") = py::none());
  m.def("set_weight_epoch", [](int64_t e) { g_weight_epoch = e; }, py::arg("epoch"),
        "bf16 weight shadows changed (optimizer step / re-cast): cached flipped filters are refreshed at next use");
  m.def("conv_wgrad", &conv_wgrad, py::arg("dy"), py::arg("x"), py::arg("dw"), py::arg("stride"), py::arg("pad"),
        py::arg("dil"), py::arg("alpha") = 1.0, py::arg("in_coef") = py::none(), py::arg("fin_stream") = 0,
        py::arg("deterministic") = false, py::arg("overwrite") = false,
        "dw (+)= alpha dW; fin_stream: a K-split hgemm's slab reduction runs on that stream (caller orders consumers); "
        "deterministic: 1x1 weight grads on the LDS-DMA kernel (pre-BN or plain input, < 256 channels on a side) and the "
        "persistent GEMM's sum their K splits in a fixed order (no atomics); "
        "overwrite: dw = alpha dW (dw's old contents, e.g. torch.empty, are never read)");
  m.def("set_pw_stream", &set_pw_stream, "streaming pointwise-conv kernel on/off (pwconv.hip)");
  m.def("set_row_wgrad", &set_row_wgrad, "64-channel 3x3 weight grads on the row-walking kernel (rowconv.hip) on/off");
  m.def("set_rowconv", &set_rowconv, "64-channel 3x3 convs on the row-walking kernel (rowconv.hip) on/off");
  m.def("set_stem_kernel", &set_stem_kernel, "s2d stem conv on its row-walking kernel (stem.hip) on/off");
  m.def("set_wgrad_hgemm", &set_wgrad_hgemm, "1x1 conv weight grads on the persistent hgemm kernel on/off");
  m.def("set_hgemm_conv", &set_hgemm_conv,
        "3x3 forward-form convs with >= 256 output channels on the persistent GEMM (implicit im2col A) on/off");
  m.def("set_wgrad_wide", [](int64_t v) { g_wgrad_wide = (int)v; },
        "64x256 tile for Cout = 64 weight grads: 0 off, 1 when C <= 16 (default), 2 always");
  m.def("set_phase_group", [](bool on) { g_phase_group = on; },
        "strided data grads: all parity sub-GEMMs in one grid, or one launch per parity (default)");
  m.def("set_conv_tile", [](int64_t mode) { g_dma_tile = (int)mode; },
        "LDS-DMA conv tile: 0 auto, 1 128-tile, 2 256x128, 3 256x256 (8 waves)");
  m.def("pick_gemm_cfg", [](int64_t M, int64_t N, int64_t K, bool split) {
    auto c = pick_cfg(M, N, K, split);
    return std::make_tuple(c.bm, c.bn, c.splits, c.k_split);
  });
}

}  // namespace dpe_ops
