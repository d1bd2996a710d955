// The body of the LDS-DMA dQ kernel: included (not compiled alone) inside each of its entry points in attn.hip, which
// set the scope it reads -- PACKED, DROP, BIDIR, GQA, WINDOW (constexpr bool) and qkv, o, dout, lse2, delta, dqkv, B, T, H, sl2, scale, doc_start, dr, L, Hkv, window.
// Text inclusion, not a shared device function: the entry points from before GQA then compile to exactly the
// instructions they had (an inlined body function changes the schedule), and the GQA entry points can carry their own
// target attribute (DPE_NO_PK_F32).
  static_assert(!BIDIR || (!PACKED && !DROP), "the bidirectional mode has no packed or dropout form");
  static_assert(!GQA || (!DROP && !BIDIR), "grouped K / V heads have no dropout or bidirectional form");
  static_assert(!WINDOW || (!DROP && !BIDIR), "the sliding window has no dropout or bidirectional form");
  // per buffer: K (two d-halves, K-contig) 8K | V (same) 8K | K permuted-row image 8K
  constexpr int KI = 0, VI = 2 * AKV * 64, KP = 4 * AKV * 64, STG = KP + AKV * 128;
  __shared__ __attribute__((aligned(16))) char smem[2 * STG];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, li = lane & 15;
  const int nq = (T + FQ - 1) / FQ, BH = B * H;
  const int qt = nq - 1 - (int)(blockIdx.x / BH);  // heaviest query tiles first
  const int bh = blockIdx.x % BH, b = bh / H, h = bh % H;
  const int64_t RS = GQA ? (int64_t)(H + 2 * Hkv) * AD : 3LL * H * AD;
  const int64_t ORS = (int64_t)H * AD;
  const uint16_t* qb = qkv + (int64_t)b * T * RS + (int64_t)h * AD;
  const uint16_t* kb = GQA ? qkv + (int64_t)b * T * RS + (int64_t)(H + h / (H / Hkv)) * AD : qb + H * AD;
  const int q0w = qt * FQ + 32 * w;
  const bool live = q0w < T;
  const int ktw = live ? (q0w + 31) / AKV : -1;
  int kd = BIDIR ? L / AKV : (q0w + 1) / AKV;  // key tiles below kd need no mask (bidirectional: are full)
  if constexpr (BIDIR) asm volatile("" : "+v"(kd));  // a per-wave branch, as in attn_fwd_dma_kernel (222 -> 195 VGPRs)
  const int nkt = BIDIR ? (L + AKV - 1) / AKV : min((qt * FQ + FQ - 1) / AKV, T / AKV - 1) + 1;
  if constexpr (BIDIR) {
    if (qt * FQ >= L) {  // every query of the workgroup is padding (workgroup-uniform: no barrier is left behind)
      if (live) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int myq = q0w + 16 * r + li;
          uint16_t* dq = dqkv + ((int64_t)b * T + myq) * RS + (int64_t)h * AD;
#pragma unroll
          for (int d = 0; d < 4; ++d) *(u32x2*)(dq + 16 * d + 4 * g) = u32x2{0u, 0u};
          if (g == 0) delta[(int64_t)bh * T + myq] = 0.f;
        }
      }
      return;
    }
  }

  // the wave's Q / dO rows as B operands; delta = rowsum(dO * O) from the same lanes (the
  // lane's 16 d-values, then the 4-group permlane reduce), published for the dK/dV kernel
  bf16x8 qf[2][2], of[2][2];
  float lq[2], ndl[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int myq = live ? q0w + 16 * r + li : 0;
    float dot = 0.f;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int64_t oo = ((int64_t)b * T + myq) * ORS + (int64_t)h * AD + 32 * kk + 8 * g;
      const u32x4 dov = *(const u32x4*)(dout + oo);
      qf[r][kk] = __builtin_bit_cast(bf16x8, *(const u32x4*)(qb + (int64_t)myq * RS + 32 * kk + 8 * g));
      of[r][kk] = __builtin_bit_cast(bf16x8, dov);
      float fa[8], fb[8];
      unpack8(dov, fa);
      unpack8(*(const u32x4*)(o + oo), fb);
#pragma unroll
      for (int e = 0; e < 8; ++e) dot = fmaf(fa[e], fb[e], dot);
    }
    dot = rowsum4(dot);
    if constexpr (BIDIR) dot = myq < L ? dot : 0.f;
    if (live && g == 0) delta[(int64_t)bh * T + myq] = dot;
    lq[r] = lse2[(int64_t)bh * T + myq];
    ndl[r] = -dot;
  }

  // packed: first key tile of the workgroup / of the wave, first key no lower mask is needed from, the lane's bounds
  int kt0 = 0, klo = 0, dshi = 0, ds[2] = {0, 0};
  if constexpr (PACKED) {
    const int* dsb = doc_start + (int64_t)b * T;
    kt0 = min(max(__builtin_amdgcn_readfirstlane(dsb[qt * FQ]) / AKV, 0), nkt - 1);
    if (live) {
      klo = __builtin_amdgcn_readfirstlane(dsb[q0w]) / AKV;
      dshi = __builtin_amdgcn_readfirstlane(dsb[q0w + 31]);
      ds[0] = dsb[q0w + li];
      ds[1] = dsb[q0w + 16 + li];
    }
  }
  // window: the forward's walk (attn_dma_fwd_body) -- the bounds also hold i - window + 1, computed, not loaded
  if constexpr (WINDOW) {
    kt0 = max(kt0, max(qt * FQ - window + 1, 0) / AKV);
    klo = max(klo, max(q0w - window + 1, 0) / AKV);
    dshi = max(dshi, q0w + 32 - window);
    ds[0] = max(ds[0], q0w + li - window + 1);
    ds[1] = max(ds[1], q0w + 16 + li - window + 1);
  }

  // the sequence's qkv rows from K of head h on: one buffer resource, tile advance in soffset
  // dropout: the forward's counters (attn_fwd_dma_kernel)
  [[maybe_unused]] uint64_t dseed = 0, dctr[2] = {0, 0};
  [[maybe_unused]] float dscale = 1.f;
  if constexpr (DROP) {
    const uint64_t n4 = (uint64_t)(T >> 2);
    dseed = (uint64_t)dr.rng[0];
    dscale = 256.f / (float)(256u - dr.thr);
#pragma unroll
    for (int r = 0; r < 2; ++r)
      dctr[r] = (uint64_t)dr.rng[1] + ((uint64_t)bh * n4 + (uint64_t)((q0w + 16 * r + li) >> 2)) * n4 + (uint64_t)(4 * (li & 3) + g);
  }
  const __amdgpu_buffer_rsrc_t rkv =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(kb), (short)0, (int)(T * RS * 2), 0x00020000);
  uint32_t voff[6];  // piece w + 4 i of the 24 KiB image set: [K halves | V halves | K permuted-row]
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int oo = ((w + 4 * i) * 1024 + lane * 16) & 8191;
    int row, dc;
    if (i < 4) {  // (dc >> 2) * 4096 + kimg(row, dc & 3)
      const int o2 = oo & 4095;
      row = o2 >> 6;
      dc = 4 * (oo >> 12) + (((o2 >> 4) & 3) ^ ((0x78 >> (((row >> 2) & 3) << 1)) & 3));
    } else {      // pimg(row, dc)
      row = oo >> 7;
      dc = ((oo >> 4) & 7) ^ (((row >> 1) & 3) << 1);
    }
    voff[i] = (uint32_t)(((int64_t)row * RS + ((i & 6) == 2 ? (GQA ? Hkv : H) * AD : 0) + dc * 8) * 2);
  }
  auto dma_tile = [&](int kt, int buf) {
    char* base = smem + buf * STG;
    const uint32_t so = (uint32_t)((int64_t)kt * AKV * RS * 2);
#pragma unroll
    for (int i = 0; i < 6; ++i) attn_dma16(rkv, base + (w + 4 * i) * 1024, voff[i], so);
  };

  f32x4 acc[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int d = 0; d < 4; ++d) acc[r][d] = f32x4{0.f, 0.f, 0.f, 0.f};
  dma_tile(kt0, 0);
  attn_vm_drain();
  wg_barrier();
  // the tile loop unrolled by two: the LDS buffer of each step is a compile-time constant, so every
  // fragment address is a hoisted per-lane offset plus an immediate
  auto step = [&](int kt, auto bufc) {
    constexpr int cur = decltype(bufc)::value;
    const bool more = kt + 1 < nkt;
    if (more) dma_tile(kt + 1, cur ^ 1);  // cur ^ 1 last read before the previous barrier
    // maskc: 0 no mask, 1 causal mask, 2 (packed only) causal and document-start mask, 3 (bidirectional only) key < L
    auto compute = [&](const char* s, auto maskc) __attribute__((always_inline)) {
      constexpr int MK = decltype(maskc)::value;
      constexpr bool MASK = MK == 1;
      f32x4 sc[2][4], dp[2][4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const bf16x8 k0 = kfrag64(s + KI, 16 * nt), k1 = kfrag64(s + KI + AKV * 64, 16 * nt);
        const bf16x8 v0 = kfrag64(s + VI, 16 * nt), v1 = kfrag64(s + VI + AKV * 64, 16 * nt);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          sc[r][nt] = MFMA(k1, qf[r][1], MFMA(k0, qf[r][0], (f32x4{0.f, 0.f, 0.f, 0.f})));
          const float c0 = DROP ? 0.f : ndl[r];
          dp[r][nt] = MFMA(v1, of[r][1], MFMA(v0, of[r][0], (f32x4{c0, c0, c0, c0})));
        }
      }
      bf16x8 dd[2][2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int myq = q0w + 16 * r + li;
        [[maybe_unused]] uint32_t dw[4];
        if constexpr (DROP) drop_words_q(dw, dseed, dctr[r], (uint32_t)kt * (AKV / 4), dr.stream, li & 3);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float p = __builtin_amdgcn_exp2f(fmaf(sc[r][nt][e], sl2, -lq[r]));
            if constexpr (MASK)
              if (kt * AKV + 16 * nt + 4 * g + e > myq) p = 0.f;
            if constexpr (MK == 2) {
              const int key = kt * AKV + 16 * nt + 4 * g + e;
              p = ((key > myq) | (key < ds[r])) ? 0.f : p;
            }
            if constexpr (DROP)  // dS^T = P (M s dP^T - delta); dP^T started from 0
              dp[r][nt][e] = p * fmaf(dp[r][nt][e], drop_keep(dw[nt], e, dr.thr) ? dscale : 0.f, ndl[r]);
            else if constexpr (MK == 3)  // a padding key: dS is 0 by select, whatever its K / V rows hold
              dp[r][nt][e] = (kt * AKV + 16 * nt + 4 * g + e < L) ? p * dp[r][nt][e] : 0.f;
            else
              dp[r][nt][e] = p * dp[r][nt][e];  // dS^T (unscaled); dP^T started from -delta
          }
        dd[r][0] = pack_frag(dp[r][0], dp[r][1]);
        dd[r][1] = pack_frag(dp[r][2], dp[r][3]);
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const bf16x8 a0 = trfrag(s + KP, 0, 16 * d), a1 = trfrag(s + KP, 32, 16 * d);
#pragma unroll
        for (int r = 0; r < 2; ++r) acc[r][d] = MFMA(a1, dd[r][1], MFMA(a0, dd[r][0], acc[r][d]));
      }
    };
    if constexpr (PACKED || WINDOW) {
      if (kt >= klo && kt <= ktw) {
        if (kt * AKV < dshi) compute(smem + cur * STG, std::integral_constant<int, 2>{});
        else if (kt < kd) compute(smem + cur * STG, std::integral_constant<int, 0>{});
        else compute(smem + cur * STG, std::integral_constant<int, 1>{});
      }
    } else if constexpr (BIDIR) {
      if (q0w < L) {  // a wave past L only stages its pieces of the tiles
        if (kt < kd) compute(smem + cur * STG, std::integral_constant<int, 0>{});
        else compute(smem + cur * STG, std::integral_constant<int, 3>{});
      }
    } else {
      if (kt < kd) compute(smem + cur * STG, std::integral_constant<int, 0>{});
      else if (kt <= ktw) compute(smem + cur * STG, std::integral_constant<int, 1>{});
    }
    if (more) attn_vm_drain();
    wg_barrier();
  };
  for (int kt = kt0; kt < nkt; kt += 2) {
    step(kt, std::integral_constant<int, 0>{});
    if (kt + 1 < nkt) step(kt + 1, std::integral_constant<int, 1>{});
  }
  if (!live) return;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    uint16_t* o = dqkv + ((int64_t)b * T + q0w + 16 * r + li) * RS + (int64_t)h * AD;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      u32x2 pk;
      pk[0] = pack_bf2(acc[r][d][0] * scale, acc[r][d][1] * scale);
      pk[1] = pack_bf2(acc[r][d][2] * scale, acc[r][d][3] * scale);
      if constexpr (BIDIR) pk = q0w + 16 * r + li < L ? pk : u32x2{0u, 0u};
      *(u32x2*)(o + 16 * d + 4 * g) = pk;
    }
  }
