// Host-visible argument block of the flash-attention kernels (attn.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dpe {

// One attention call, forward or backward.  Every mode is a field here, and dpe_attn_route is the only place that
// knows which combinations exist.
struct AttnArgs {
  const uint16_t* qkv;       // bf16 [B, T, 3, H, D], or [B, T, H + 2 Hkv, D] with Hkv (query, key, value heads)
  uint16_t* out;             // bf16 [B, T, H, D]: written by the forward, read by the backward
  const uint16_t* dout;      // backward: bf16 [B, T, H, D]
  float* lse;                // f32 [B, H, T]: written by the forward, read by the backward
  float* delta;              // backward scratch f32 [B, H, T]: rowsum(dO * O), dQ kernel -> dK/dV kernel
  uint16_t* dqkv;            // backward: bf16, qkv's layout
  int B, T, H;
  int Hkv;                   // grouped-query attention: K / V heads, H % Hkv == 0 (causal, no dropout); 0 = [3, H]
  int D;                     // head dim (64)
  float scale;
  int causal;                // 0: bidirectional over the first seq_len rows (no doc_start, no dropout)
  int seq_len;               // causal == 0: keys and queries < seq_len (0 = T); out / dqkv rows from there on are zeros
  const int32_t* doc_start;  // packed documents (int32 [B, T], both or neither): query i sees doc_start[i] <= j <= i
  const int32_t* doc_end;
  int window;                // sliding window W >= 1 (causal, no dropout): query i sees max(doc_start[i], i - W + 1) <= j <= i;
                             // 0 = no window, W >= T is plain causal attention
  const int64_t* rng;        // dropout on P: device int64[2] (seed, offset)
  uint32_t stream;           // the call site (Philox counter_lo)
  uint32_t thr;              // drop rate thr / 256, 1 .. 255; 0 = no dropout
};

// The kernel family that serves a call.
enum AttnRoute : int {
  AR_NONE = 0,    // refused
  AR_STAGED = 1,  // register-staged kernels: plain causal only
  AR_DMA = 2,     // LDS-DMA kernels: plain causal, packed documents, dropout, bidirectional
  AR_GQA = 3,     // LDS-DMA kernels, grouped K / V heads: causal, packed documents
};

}  // namespace dpe

// The route of `a` from its integers and from which of doc_start, doc_end, rng are null (nothing is dereferenced, no
// HIP call).  AR_NONE: *why (when given) names the argument that is refused.
extern "C" int dpe_attn_route(const dpe::AttnArgs& a, const char** why);
// Returns 0, or -1 where dpe_attn_route refuses.  The backward launches dQ (which writes delta), then dK/dV.
extern "C" int dpe_attn_fwd(const dpe::AttnArgs& a, hipStream_t st);
extern "C" int dpe_attn_bwd(const dpe::AttnArgs& a, hipStream_t st);
