// The body of the LDS-DMA forward kernel: included (not compiled alone) inside each of its entry points in attn.hip, which
// set the scope it reads -- PACKED, DROP, BIDIR, GQA, WINDOW (constexpr bool) and qkv, out, lse2, B, T, H, sl2, doc_start, dr, L, Hkv, window.
// Text inclusion, not a shared device function: the entry points from before GQA then compile to exactly the
// instructions they had (an inlined body function changes the schedule), and the GQA entry points can carry their own
// target attribute (DPE_NO_PK_F32).
  static_assert(!BIDIR || (!PACKED && !DROP), "the bidirectional mode has no packed or dropout form");
  static_assert(!GQA || (!DROP && !BIDIR), "grouped K / V heads have no dropout or bidirectional form");
  static_assert(!WINDOW || (!DROP && !BIDIR), "the sliding window has no dropout or bidirectional form");
  constexpr int KB = 2 * AKV * 64, STG = KB + AKV * 128;
  __shared__ __attribute__((aligned(16))) char smem[2 * STG];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, li = lane & 15;
  const int nq = (T + FQ - 1) / FQ, BH = B * H;
  const int qt = nq - 1 - (int)(blockIdx.x / BH);
  const int bh = blockIdx.x % BH, b = bh / H, h = bh % H;
  const int64_t RS = GQA ? (int64_t)(H + 2 * Hkv) * AD : 3LL * H * AD;
  const uint16_t* qb = qkv + (int64_t)b * T * RS + (int64_t)h * AD;
  const uint16_t* kb = GQA ? qkv + (int64_t)b * T * RS + (int64_t)(H + h / (H / Hkv)) * AD : qb + H * AD;
  const int q0w = qt * FQ + 32 * w;
  const bool live = q0w < T;
  const int ktw = live ? (q0w + 31) / AKV : -1;
  const int nkt = BIDIR ? (L + AKV - 1) / AKV : min((qt * FQ + FQ - 1) / AKV, T / AKV - 1) + 1;
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
  // window: query i's lower bound is also i - window + 1.  It is affine in the lane's query, so the pure-window form
  // loads nothing; the workgroup starts at its first query's window edge, a wave at its own, and only the tiles that
  // hold a key below the wave's last query's edge (at most two) take the both-bounds path
  if constexpr (WINDOW) {
    kt0 = max(kt0, max(qt * FQ - window + 1, 0) / AKV);
    klo = max(klo, max(q0w - window + 1, 0) / AKV);
    dshi = max(dshi, q0w + 32 - window);
    ds[0] = max(ds[0], q0w + li - window + 1);
    ds[1] = max(ds[1], q0w + 16 + li - window + 1);
  }
  if constexpr (BIDIR) {
    if (qt * FQ >= L) {  // every query of the workgroup is padding (workgroup-uniform: no barrier is left behind)
      if (live) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int myq = q0w + 16 * r + li;
          uint16_t* o = out + ((int64_t)(b * T + myq) * H + h) * AD;
#pragma unroll
          for (int d = 0; d < 4; ++d) *(u32x2*)(o + 16 * d + 4 * g) = u32x2{0u, 0u};
          if (g == 0) lse2[(int64_t)bh * T + myq] = 0.f;
        }
      }
      return;
    }
  }

  bf16x8 qf[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      qf[r][kk] = live ? __builtin_bit_cast(bf16x8, *(const u32x4*)(qb + (int64_t)(q0w + 16 * r + li) * RS + 32 * kk + 8 * g))
                       : bf16x8{};

  // the sequence's qkv rows from K of head h on: one buffer resource, tile advance in soffset
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(kb), (short)0, (int)(T * RS * 2), 0x00020000);
  uint32_t voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = (w + 4 * i) * 1024 + lane * 16;  // this lane's byte slot in the 16 KiB tile image
    int key, dc, vo;
    if (i < 2) {  // K halves: kimg(key, c) = key * 64 + ((c ^ sw(key)) << 4), half dc >> 2
      const int dh = o >> 12, oo = o & 4095;
      key = oo >> 6;
      dc = 4 * dh + (((oo >> 4) & 3) ^ ((0x78 >> (((key >> 2) & 3) << 1)) & 3));
      vo = 0;
    } else {      // V: pimg(key, c) = key * 128 + ((c ^ h(key)) << 4)
      const int oo = o - KB;
      key = oo >> 7;
      dc = ((oo >> 4) & 7) ^ (((key >> 1) & 3) << 1);
      vo = (GQA ? Hkv : H) * AD;
    }
    voff[i] = (uint32_t)(((int64_t)key * RS + vo + dc * 8) * 2);
  }
  auto dma_tile = [&](int kt, char* s) {
    const uint32_t so = (uint32_t)((int64_t)kt * AKV * RS * 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) attn_dma16(rs, s + (w + 4 * i) * 1024, voff[i], so);
  };

  f32x4 acc[2][4], accl[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    accl[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 4; ++d) acc[r][d] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float m[2] = {-INFINITY, -INFINITY};
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const bf16x8 ones = __builtin_bit_cast(bf16x8, u32x4{0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u});
  // bidirectional: the key tiles below kd are full.  kd is then workgroup-uniform; the empty asm keeps it in a VGPR so the
  // choice between the two compute paths stays a per-wave (exec) branch as in the causal kernel -- as scalar control flow
  // the compiler hoists across both paths and spills 36 registers under the 168-VGPR cap
  int kd = BIDIR ? L / AKV : (q0w + 1) / AKV;
  if constexpr (BIDIR) asm volatile("" : "+v"(kd));
  // dropout: the counter of the granule this lane draws (key group nt = li & 3) in key tile 0, per row block
  [[maybe_unused]] uint64_t dseed = 0, dctr[2] = {0, 0};
  if constexpr (DROP) {
    const uint64_t n4 = (uint64_t)(T >> 2);
    dseed = (uint64_t)dr.rng[0];
#pragma unroll
    for (int r = 0; r < 2; ++r)
      dctr[r] = (uint64_t)dr.rng[1] + ((uint64_t)bh * n4 + (uint64_t)((q0w + 16 * r + li) >> 2)) * n4 + (uint64_t)(4 * (li & 3) + g);
  }

  // maskc: 0 no mask, 1 causal mask, 2 (packed only) causal and document-start mask, 3 (bidirectional only) key < L
  auto compute = [&](int kt, const char* s, auto maskc) __attribute__((always_inline)) {
    constexpr int MK = decltype(maskc)::value;
    constexpr bool MASK = MK == 1;
    f32x4 sc[2][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const bf16x8 k0 = kfrag64(s, 16 * nt), k1 = kfrag64(s + AKV * 64, 16 * nt);
#pragma unroll
      for (int r = 0; r < 2; ++r) sc[r][nt] = MFMA(k1, qf[r][1], MFMA(k0, qf[r][0], zero));
    }
    float mc[2];
    bool need[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if constexpr (MASK) {
        const int lim = q0w + 16 * r + li - kt * AKV - 4 * g;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (16 * nt + e > lim) sc[r][nt][e] = -INFINITY;
      }
      float mx;
      if constexpr (MK == 2) {  // the row max over the visible keys only; -inf for a row that sees none here
        const int lim = q0w + 16 * r + li - kt * AKV - 4 * g, lo = ds[r] - kt * AKV - 4 * g;
        mx = -INFINITY;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) mx = ((16 * nt + e <= lim) & (16 * nt + e >= lo)) ? fmaxf(mx, sc[r][nt][e]) : mx;
        mx = rowmax4(mx);
        mc[r] = mx == -INFINITY ? mx : mx * sl2;
        need[r] = mc[r] > (m[r] == -INFINITY ? m[r] : m[r] + RESCALE_TH);  // false for a row without a visible key
      } else if constexpr (MK == 3) {  // the row max over the keys < L; the tile's first key is one, so it is finite
        const int hi = L - kt * AKV - 4 * g;
        mx = -INFINITY;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) mx = (16 * nt + e < hi) ? fmaxf(mx, sc[r][nt][e]) : mx;
        mc[r] = rowmax4(mx) * sl2;
        need[r] = mc[r] > m[r] + RESCALE_TH;
      } else {
        mx = sc[r][0][0];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = (nt == 0); e < 4; ++e) mx = fmaxf(mx, sc[r][nt][e]);
        mc[r] = rowmax4(mx) * sl2;
        need[r] = mc[r] > m[r] + RESCALE_TH;
      }
    }
    if (__builtin_amdgcn_ballot_w64(need[0] || need[1])) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        float alpha;
        if constexpr (MK == 2)  // a first visible key: the accumulators are still 0, nothing to rescale
          alpha = (need[r] & (m[r] != -INFINITY)) ? __builtin_amdgcn_exp2f(m[r] - mc[r]) : 1.f;
        else
          alpha = need[r] ? __builtin_amdgcn_exp2f(m[r] - mc[r]) : 1.f;
        m[r] = need[r] ? mc[r] : m[r];
        accl[r] *= alpha;
#pragma unroll
        for (int d = 0; d < 4; ++d) acc[r][d] *= alpha;
      }
    }
    bf16x8 pk[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if constexpr (MK == 2) {  // a masked P is 0 by select after the exp2 (which may have overflowed), m = -inf or not
        const float nm = m[r] == -INFINITY ? 0.f : -m[r];
        const int lim = q0w + 16 * r + li - kt * AKV - 4 * g, lo = ds[r] - kt * AKV - 4 * g;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float pv = __builtin_amdgcn_exp2f(fmaf(sc[r][nt][e], sl2, nm));
            sc[r][nt][e] = ((16 * nt + e <= lim) & (16 * nt + e >= lo)) ? pv : 0.f;
          }
      } else if constexpr (MK == 3) {  // a masked P is 0 by select after the exp2 (which may have overflowed)
        const float nm = -m[r];
        const int hi = L - kt * AKV - 4 * g;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float pv = __builtin_amdgcn_exp2f(fmaf(sc[r][nt][e], sl2, nm));
            sc[r][nt][e] = (16 * nt + e < hi) ? pv : 0.f;
          }
      } else {
        const float nm = -m[r];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) sc[r][nt][e] = __builtin_amdgcn_exp2f(fmaf(sc[r][nt][e], sl2, nm));
      }
      pk[r][0] = pack_frag(sc[r][0], sc[r][1]);
      pk[r][1] = pack_frag(sc[r][2], sc[r][3]);
      accl[r] = MFMA(ones, pk[r][1], MFMA(ones, pk[r][0], accl[r]));
      if constexpr (DROP) {  // l summed the undropped P above; O takes the dropped fragments
        uint32_t dw[4];
        drop_words_q(dw, dseed, dctr[r], (uint32_t)kt * (AKV / 4), dr.stream, li & 3);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) sc[r][nt][e] = drop_keep(dw[nt], e, dr.thr) ? sc[r][nt][e] : 0.f;
        pk[r][0] = pack_frag(sc[r][0], sc[r][1]);
        pk[r][1] = pack_frag(sc[r][2], sc[r][3]);
      }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const bf16x8 v0 = trfrag(s + KB, 0, 16 * d), v1 = trfrag(s + KB, 32, 16 * d);
#pragma unroll
      for (int r = 0; r < 2; ++r) acc[r][d] = MFMA(v1, pk[r][1], MFMA(v0, pk[r][0], acc[r][d]));
    }
  };

  dma_tile(kt0, smem);
  attn_vm_drain();
  wg_barrier();
  // the tile loop unrolled by two: each step's LDS buffer is a compile-time constant
  auto step = [&](int kt, auto bufc) {
    constexpr int cur = decltype(bufc)::value;
    const bool more = kt + 1 < nkt;
    if (more) dma_tile(kt + 1, smem + (cur ^ 1) * STG);  // read last in step kt - 1, before its barrier
    if constexpr (PACKED || WINDOW) {
      if (kt >= klo && kt <= ktw) {
        if (kt * AKV < dshi) compute(kt, smem + cur * STG, std::integral_constant<int, 2>{});
        else if (kt < kd) compute(kt, smem + cur * STG, std::integral_constant<int, 0>{});
        else compute(kt, smem + cur * STG, std::integral_constant<int, 1>{});
      }
    } else if constexpr (BIDIR) {
      if (q0w < L) {  // a wave past L only stages its pieces of the tiles
        if (kt < kd) compute(kt, smem + cur * STG, std::integral_constant<int, 0>{});
        else compute(kt, smem + cur * STG, std::integral_constant<int, 3>{});
      }
    } else {
      if (kt < kd) compute(kt, smem + cur * STG, std::integral_constant<int, 0>{});
      else if (kt <= ktw) compute(kt, smem + cur * STG, std::integral_constant<int, 1>{});
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
    const int myq = q0w + 16 * r + li;
    const float l = accl[r][0];  // every row of the all-ones product is the sum over keys for query li
    const float inv = (DROP ? 256.f / (float)(256u - dr.thr) : 1.f) / l;
    uint16_t* o = out + ((int64_t)(b * T + myq) * H + h) * AD;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      u32x2 pk2;
      pk2[0] = pack_bf2(acc[r][d][0] * inv, acc[r][d][1] * inv);
      pk2[1] = pack_bf2(acc[r][d][2] * inv, acc[r][d][3] * inv);
      if constexpr (BIDIR) pk2 = myq < L ? pk2 : u32x2{0u, 0u};
      *(u32x2*)(o + 16 * d + 4 * g) = pk2;
    }
    float ls = m[r] + __log2f(l);
    if constexpr (BIDIR) ls = myq < L ? ls : 0.f;
    if (g == 0) lse2[(int64_t)bh * T + myq] = ls;
  }
