// The one declaration of every host launcher that takes plain pointers, included by the .hip file that defines it
// and by every caller: a prototype that disagrees with its definition is a compile error ("conflicting types"), not
// a call that links and passes garbage.  Launchers with argument structs: igemm.h, hgemm.h, pwconv.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// ---- comm.cpp
int dpe_cu_reserve();  // slots to leave to in-flight collectives
// ---- bngram.hip
int dpe_gram_blocks(int64_t M, int C);
int64_t dpe_gram_ws_floats(int64_t M, int C);
int dpe_gram(const uint16_t* x, const float* coef, const float* scoef, int64_t M, int C, float* ws, float* G, float* s,
             hipStream_t st, int sh, int sw);
int dpe_gram_pilot(const uint16_t* x, int64_t M, int C, float* coef, hipStream_t st, int sh, int sw);
int dpe_gram_u(const float* G, const uint16_t* w, int Cin, int Cout, float* u, hipStream_t st);
int dpe_gram_coef(const float* G, const float* s, const uint16_t* w, int Cin, int Cout, int64_t M, const float* gamma,
                  const float* beta, float* rmean, float* rvar, float momentum, float eps, float* coef, float* u,
                  hipStream_t st);
int64_t dpe_gram_bwd_ws_floats(int Cin, int Cout);
int dpe_gram_bwd(const float* part, int rg, const float* P, const uint16_t* w, const float* u, const float* s,
                 const float* coef3, const float* gamma, int Cin, int Cout, int64_t M, float* dgamma, float* dbeta,
                 float* dw, uint16_t* bcat, float* abc, float* ebias, float* qws, hipStream_t st);
// ---- bn.hip
int dpe_bn_stats_nblocks(int64_t M, int C);
int dpe_bn_bwd_nblocks(int64_t M, int C);
int dpe_bn_stats(const uint16_t* x, int64_t M, int C, int nb, float* part, hipStream_t st);
int dpe_bn_finalize(const float* part, int nb, int C, int64_t M, const float* gamma, const float* beta, float* rmean,
                    float* rvar, float momentum, float eps, float* coef, hipStream_t st);
int dpe_bn_eval_coeff(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar, float eps,
                      float* coef, hipStream_t st);
int dpe_bn_apply(const uint16_t* x, const uint16_t* res, uint16_t* y, int64_t M, int C, const float* coef, int relu,
                 hipStream_t st);
int dpe_bn_apply2(const uint16_t* x, const float* coef, const uint16_t* x2, const float* coef2, uint16_t* y, int64_t M, int C,
                  int relu, uint8_t* mbits, hipStream_t st);
int dpe_bn_apply_m(const uint16_t* x, const uint16_t* res, uint16_t* y, int64_t M, int C, const float* coef, int relu,
                   uint8_t* mbits, hipStream_t st);
int dpe_bn_bwd_reduce(const uint16_t* dy, const uint16_t* y, const uint8_t* ybits, const uint16_t* x, const float* coef, int64_t M, int C, int nb,
                      float* part, hipStream_t st);
int dpe_bn_bwd_reduce_apply(const uint16_t* dz, const uint16_t* x, const float* coef, const uint16_t* ax, const float* abcoef,
                            uint16_t* adx, int64_t M, int C, int nb, float* part, hipStream_t st);
int dpe_bn_bwd_finalize(const float* part, int nb, int C, int64_t M, const float* gamma, const float* coef, float* dgamma,
                        float* dbeta, float* bcoef, hipStream_t st);
int dpe_bn_bwd_apply(const uint16_t* dy, const uint16_t* y, const uint8_t* ybits, const uint16_t* x, const float* bcoef, uint16_t* dx,
                     uint16_t* dz_out, int64_t M, int C, const float* mcoef, hipStream_t st);
// ---- pool.hip
void dpe_set_pool_legacy(int on);
int dpe_maxpool_fwd(const uint16_t* x, uint16_t* y, uint8_t* idx, int N, int H, int W, int C, int OH, int OW, int k, int s,
                    int p, hipStream_t st);
int dpe_bnrelu_maxpool_fwd(const uint16_t* h, const float* coef, uint16_t* y, uint8_t* idx, int N, int H, int W, int C, int OH,
                           int OW, int k, int s, int p, hipStream_t st);
int dpe_maxpool_bn_bwd_reduce(const uint16_t* dy, const uint8_t* idx, const uint16_t* x, const float* coef, int N, int H, int W,
                              int C, int OH, int OW, int k, int s, int p, int nb, float* part, hipStream_t st);
int dpe_maxpool_bn_bwd_apply(const uint16_t* dy, const uint8_t* idx, const uint16_t* x, const float* coef, const float* bcoef,
                             uint16_t* dx, int N, int H, int W, int C, int OH, int OW, int k, int s, int p, hipStream_t st);
int dpe_maxpool_bwd(const uint16_t* dy, const uint8_t* idx, uint16_t* dx, int N, int H, int W, int C, int OH, int OW, int k,
                    int s, int p, hipStream_t st);
int dpe_gavgpool_fwd(const uint16_t* x, uint16_t* y, int N, int HW, int C, hipStream_t st);
int dpe_gavgpool_bwd(const uint16_t* dy, uint16_t* dx, int N, int HW, int C, hipStream_t st);
// ---- stem.hip
int dpe_stem_blocks(int N, int H, int W);
int dpe_stem_launch(const uint16_t* x, const uint16_t* w, uint16_t* y, float* stats, int N, int H, int W, hipStream_t st);
int64_t dpe_stem_wgrad_scratch(int N, int H, int W);
int dpe_stem_wgrad_launch(const uint16_t* x, const uint16_t* dy, float* dw, float* scratch, int N, int H, int W,
                          float alpha, hipStream_t st);
int dpe_stem_wgrad_launch2(const uint16_t* x, const uint16_t* dy, float* dw, float* scratch, int N, int H, int W,
                           float alpha, const uint16_t* dyp, const uint8_t* idx, const uint16_t* h, const float* coef,
                           const float* bcoef, hipStream_t st);
// ---- rowconv.hip
int dpe_conv3x3_rows_blocks(int N, int H, int W);
int dpe_conv3x3_rows_launch(const uint16_t* x, const uint16_t* w, uint16_t* y, float* stats, const uint16_t* st_x,
                            const float* st_coef, int N, int H, int W, int nb, int bnb, const float* in_coef, hipStream_t st);
int dpe_wgrad3x3_rows_blocks(int N, int H, int W);
int64_t dpe_wgrad3x3_rows_scratch(int nb);
int dpe_wgrad3x3_rows_launch(const uint16_t* x, const uint16_t* dy, float* dw, float* scratch, int N, int H, int W, int nb,
                             float alpha, const float* in_coef, hipStream_t st);
// ---- loss.hip
int dpe_cross_entropy(const void* logits, int in_bf16, const int64_t* labels, int B, int V, int64_t ld, float grad_scale,
                      void* dlogits, int out_bf16, float* loss_rows, float* loss_sum, float* correct, int ignore_index,
                      hipStream_t st);
int dpe_cross_entropy_mean(const void* logits, int in_bf16, const int64_t* labels, int B, int V, int64_t ld,
                           float grad_scale, void* dlogits, int out_bf16, float* loss_rows, float* out4, int ignore_index,
                           hipStream_t st);
// label smoothing eps in [0, 1) and z-loss weight zl >= 0 (the REG instantiations of the CE kernels)
int dpe_cross_entropy_mean_reg(const void* logits, int in_bf16, const int64_t* labels, int B, int V, int64_t ld,
                               float grad_scale, void* dlogits, int out_bf16, float* loss_rows, float* out4,
                               int ignore_index, float eps, float zl, hipStream_t st);
// two labels per row (the MIX instantiations): labels2[row] == ignore_index means no partner; the weight of
// labels[row] is w[row * w_stride] (w_stride 0: one weight for the batch, 1: one per row), read on the device
int dpe_cross_entropy_mean_mix(const void* logits, int in_bf16, const int64_t* labels, const int64_t* labels2, const float* w,
                               int w_stride, int B, int V, int64_t ld, float grad_scale, void* dlogits, int out_bf16,
                               float* loss_rows, float* out4, int ignore_index, float eps, float zl, hipStream_t st);
int dpe_ce_grad_scale(const void* d, void* o, int64_t n, int bf16, const float* g, const float* inv_n, hipStream_t st);
// ---- mix.hip
int dpe_mix_draw(const int64_t* rng, uint32_t stream, int H, int W, float mixup_alpha, float cutmix_alpha, float prob,
                 float switch_prob, int count, float* out, hipStream_t st);
int dpe_mix_pack(const float* x, const float* prm, uint16_t* y, int N, int C, int H, int W, int layout, int Cp,
                 hipStream_t st);
// ---- eltwise.hip
int dpe_cast_f32_bf16(const float* x, uint16_t* y, int64_t n, hipStream_t st);
int dpe_cast_bf16_f32(const uint16_t* x, float* y, int64_t n, hipStream_t st);
int dpe_act(const void* a, const void* b, void* out, int64_t n, int op, int bf16, hipStream_t st);
int dpe_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, uint64_t offset, int bf16, hipStream_t st);
// rng = device int64[2] (seed, offset); element n keeps iff philox4x32(seed, offset + n/4, stream)[n % 4] >= p * 2^32
int dpe_dropout_add(const float* res, const void* y, int y_bf16, float* out, int64_t n, float p, const int64_t* rng,
                    uint32_t stream, hipStream_t st);
int dpe_dropout_cast(const float* g, uint16_t* out, int64_t n, float p, const int64_t* rng, uint32_t stream, hipStream_t st);
int dpe_add(const void* a, const void* b, void* out, int64_t n, float alpha, int bf16, hipStream_t st);
int dpe_colsum(const void* dy, int64_t M, int N, int64_t ld, float* db, int accumulate, int bf16, hipStream_t st);
int dpe_nchw_to_s2d(const float* x, uint16_t* y, int N, int C, int H, int W, hipStream_t st);
int dpe_nchw_to_nhwc(const float* x, uint16_t* y, int N, int C, int HW, int Cp, hipStream_t st);
// x NCHW f32 -> y bf16 [N, (H/p)(W/p), C p p], rows ordered (c, py, px); p % 8 == 0, H % p == W % p == 0
int dpe_patchify(const float* x, uint16_t* y, int N, int C, int H, int W, int p, hipStream_t st);
int dpe_conv_w_flipT(const uint16_t* w, uint16_t* wt, int K, int R, int S, int C, int r0, int rs, int Rp, int s0, int ss,
                     int Sp, hipStream_t st);
int dpe_flip_desc_bytes();
int dpe_flip_blocks(int K, int C, int Rp, int Sp);
int dpe_conv_w_flipT_multi(const void* desc, const int* start, int n, int total_blocks, hipStream_t st);
// pos: position id per row (int32 [rows]); null = r % T
int dpe_embedding_fwd(const int64_t* idx, const uint16_t* wte, const uint16_t* wpe, float* out, int64_t rows, int T, int D,
                      const int32_t* pos, hipStream_t st);
int dpe_embedding_bwd(const int64_t* idx, const float* dout, float* dwte, float* dwpe, int64_t rows, int T, int D,
                      const int32_t* pos, hipStream_t st);
int64_t dpe_cu_hog_buf_floats(int nblocks);
int dpe_cu_hog(int nblocks, int threads, int lds_bytes, double us, int vgprs, const unsigned* stop, float* sink,
               int sleepy, float* buf, hipStream_t st);
int dpe_hog_stop(unsigned* stop, unsigned v, hipStream_t st);
// ---- optim.hip
int dpe_optim_chunk_size();
int dpe_optim_desc_bytes();
int dpe_optim_step(int kind, const void* desc, const void* chunks, int nchunks, const float* hp, const float* steps,
                   hipStream_t st);
int dpe_optim_grad_norm(const void* desc, const void* chunks, int nchunks, float* partials, float* out, const float* max_norm,
                        float* hp, int ngroups, int skip, hipStream_t st);
int dpe_optim_grad_scale(const void* desc, const void* chunks, int nchunks, const float* out, hipStream_t st);
int dpe_optim_clip_coef(const float* partials, int nchunks, float* out, const float* max_norm, float* hp, int ngroups, int skip,
                        hipStream_t st);
int dpe_optim_sched_header();  // doubles in the schedule block before the per-group base lrs
int dpe_optim_lr_schedule(float* hp, int ngroups, double* sched, float* cur, hipStream_t st);
int dpe_optim_trust_partials(int kind, const void* desc, const void* chunks, int nchunks, const float* hp, const float* steps,
                             float* part_w, float* part_x, hipStream_t st);
int dpe_optim_trust_ratio(int kind, const void* desc, int ntensors, const int* first_chunk, int nchunks, const float* part_w,
                          const float* part_x, const float* hp, float* stats, hipStream_t st);
int dpe_optim_trust_step(int kind, const void* desc, const void* chunks, int nchunks, const float* hp, const float* steps,
                         const float* stats, hipStream_t st);
// the weight EMA (ema: device array of one fp32 pointer per tensor of the table; blk: fp64 [3] n, decay, warm-up)
int dpe_optim_step_ema(int kind, const void* desc, const void* chunks, int nchunks, const float* hp, const float* steps,
                       const void* ema, hipStream_t st);
int dpe_optim_trust_step_ema(int kind, const void* desc, const void* chunks, int nchunks, const float* hp, const float* steps,
                             const float* stats, const void* ema, hipStream_t st);
int dpe_optim_ema_decay(float* hp, int ngroups, double* blk, float* cur, hipStream_t st);
int dpe_optim_ema_swap(const void* desc, const void* chunks, int nchunks, const void* ema, hipStream_t st);
// ---- norm.hip
int dpe_layernorm_fwd(const void* x, int x_bf16, const float* w, const float* b, uint16_t* y, float* mean, float* rstd,
                      int64_t rows, int D, float eps, hipStream_t st);
int dpe_layernorm_bwd_nblocks(int64_t rows);
int64_t dpe_layernorm_bwd_scratch(int64_t rows, int D);
int dpe_layernorm_bwd(const uint16_t* dy, const void* x, int x_bf16, const float* w, const float* mean, const float* rstd,
                      void* dx, int dx_accumulate_f32, const float* res_in, uint16_t* dx_bf16, float* dw, float* db,
                      float* part, int64_t rows, int D, hipStream_t st);
int dpe_layernorm_bwd_finalize_group(const float* const* parts, const int64_t* rows, const int* Ds, float* const* dws,
                                     float* const* dbs, int n, hipStream_t st);
// ---- attn.hip
// doc_start / doc_end: the packed-document mask (int32 [B, T], both or neither; null = plain causal)
int dpe_attn_fwd(const uint16_t* qkv, uint16_t* out, float* lse, int B, int T, int H, int D, float scale, int causal,
                 const int32_t* doc_start, const int32_t* doc_end, hipStream_t st);
int dpe_attn_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, float* delta,
                 float* dq_acc, uint16_t* dqkv, int B, int T, int H, int D, float scale, int causal, const int32_t* doc_start,
                 const int32_t* doc_end, hipStream_t st);
int dpe_set_attn_staged(int on);
// dropout on P (LDS-DMA kernels only): rng = device int64[2] (seed, offset), stream = call site, drop rate thr / 256
int dpe_attn_fwd_drop(const uint16_t* qkv, uint16_t* out, float* lse, int B, int T, int H, int D, float scale, int causal,
                      const int32_t* doc_start, const int32_t* doc_end, const int64_t* rng, uint32_t stream, uint32_t thr,
                      hipStream_t st);
int dpe_attn_bwd_drop(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, float* delta,
                      uint16_t* dqkv, int B, int T, int H, int D, float scale, int causal, const int32_t* doc_start,
                      const int32_t* doc_end, const int64_t* rng, uint32_t stream, uint32_t thr, hipStream_t st);
// bidirectional attention over the first seq_len rows (1 <= seq_len <= T; out / dqkv rows from seq_len on are zeros);
// LDS-DMA kernels only, no doc_start, no dropout
int dpe_attn_fwd_bidir(const uint16_t* qkv, uint16_t* out, float* lse, int B, int T, int H, int D, float scale, int seq_len,
                       hipStream_t st);
int dpe_attn_bwd_bidir(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, float* delta,
                       uint16_t* dqkv, int B, int T, int H, int D, float scale, int seq_len, hipStream_t st);
// ---- decode.hip
// one query per (b, h) against the head-major cache kc / vc [B, H, Tmax, 64]; qkv_step [B, 3, H, 64]; len int32 [B]
// (clamped into [0, Tmax - 1]); S key splits (ws: dpe_attn_decode_ws_floats fp32, unused for S = 1); out [B, H * 64]
int dpe_attn_decode_splits(int BH, int Tmax);  // the default S: a function of the launch shape only
int64_t dpe_attn_decode_ws_floats(int BH, int S);
int dpe_attn_decode(const uint16_t* qkv_step, uint16_t* kc, uint16_t* vc, const int32_t* len, int B, int H, int Tmax, int S,
                    float scale, float* ws, uint16_t* out, hipStream_t st);
// y[M, N] = x[M, K] w[N, K]^T, M <= 16, K % 32 == 0, N % 16 == 0, row strides % 8 == 0.  bf16 out (+ bias, GELU) or
// fp32 out (+ bias, + fp32 residual that may alias y).  ksplit > 1: ws of ksplit * M * N floats.
int dpe_linear_skinny_ok(int M, int N, int K, int64_t ldx, int64_t ldw);
int dpe_linear_skinny_ksplit(int M, int N, int K);  // the default K split over blocks
int dpe_linear_skinny_waves();                      // K partials summed inside a block
int dpe_linear_skinny(const uint16_t* x, int64_t ldx, const uint16_t* w, int64_t ldw, int M, int N, int K, const float* bias,
                      int gelu, int out_f32, const float* res, int64_t ldr, void* y, int64_t ldy, int ksplit, float* ws,
                      hipStream_t st);
// one token per row: temperature (0 = argmax), top_k (0 = off), top_p (1 = off), Gumbel-max from rng = device
// int64[2] (seed, offset); done int32 [B] or null; eos_id -1 = none
int dpe_sample_logits(const void* logits, int in_bf16, int B, int V, int64_t ld, float temperature, int top_k, float top_p,
                      const int64_t* rng, uint32_t stream, int eos_id, int32_t* done, int64_t* out, hipStream_t st);
// ---- gemm_f32.hip
int dpe_gemm_f32(const float* A, const float* B, float* C, int64_t sam, int64_t sak, int64_t sbk, int64_t sbn,
                 int64_t ldc, int M, int N, int K, const float* bias, float alpha, int relu, float drop_p,
                 uint64_t seed, uint64_t offset, const float* mask_src, float mask_scale, int accumulate,
                 hipStream_t st);
}
