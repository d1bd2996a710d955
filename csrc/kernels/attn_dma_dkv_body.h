// The body of the LDS-DMA dK / dV kernel: included (not compiled alone) inside each of its entry points in attn.hip, which
// set the scope it reads -- PACKED, DROP, BIDIR, GQA, WINDOW (constexpr bool) and qkv, dout, lse2, delta, dqkv, B, T, H, sl2, scale, doc_start, doc_end, dr, L, Hkv, window.
// Text inclusion, not a shared device function: the entry points from before GQA then compile to exactly the
// instructions they had (an inlined body function changes the schedule), and the GQA entry points can carry their own
// target attribute (DPE_NO_PK_F32).
  static_assert(!BIDIR || (!PACKED && !DROP), "the bidirectional mode has no packed or dropout form");
  static_assert(!GQA || (!DROP && !BIDIR), "grouped K / V heads have no dropout or bidirectional form");
  static_assert(!WINDOW || (!DROP && !BIDIR), "the sliding window has no dropout or bidirectional form");
  // per buffer: Qk Qm dOk dOm (8 KB each) + lse, delta (512 B) (+ packed: doc_start, 256 B)
  constexpr int BUF = 4 * 8192 + 512 + (PACKED ? 256 : 0);
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, li = lane & 15;
  // GQA: bh runs over (b, KV head); h is the first query head of the workgroup's group, hk its K / V head
  const int nqt = T / AQ, BH = B * (GQA ? Hkv : H);
  const int kt = (int)(blockIdx.x / BH);  // heaviest key tiles (most query tiles) first
  const int bh = blockIdx.x % BH, b = bh / (GQA ? Hkv : H), h = GQA ? (bh % Hkv) * (H / Hkv) : bh % H;
  [[maybe_unused]] const int hk = GQA ? bh % Hkv : h;
  const int64_t RS = GQA ? (int64_t)(H + 2 * Hkv) * AD : 3LL * H * AD;
  const uint16_t* qb = qkv + (int64_t)b * T * RS + (int64_t)h * AD;
  const uint16_t* kb = GQA ? qkv + (int64_t)b * T * RS + (int64_t)(H + hk) * AD : qb + H * AD;
  const uint16_t* vb = GQA ? kb + Hkv * AD : qb + 2 * H * AD;
  const int64_t ORS = (int64_t)H * AD;  // dO / O row stride
  const uint16_t* ob = dout + (int64_t)b * T * ORS + (int64_t)h * AD;
  const int k0w = kt * BKW + 32 * w;  // the wave's first key
  const bool live = k0w < T;
  const int qtw = k0w / AQ;           // first query tile that reaches the wave's keys
  if constexpr (BIDIR) {
    if (kt * BKW >= L) {  // every key of the workgroup is padding (workgroup-uniform: no barrier is left behind)
      if (live) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          uint16_t* dkb = dqkv + (int64_t)b * T * RS + (int64_t)(k0w + 16 * r + li) * RS + H * AD + (int64_t)h * AD;
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            *(u32x2*)(dkb + 16 * d + 4 * g) = u32x2{0u, 0u};
            *(u32x2*)(dkb + H * AD + 16 * d + 4 * g) = u32x2{0u, 0u};
          }
        }
      }
      return;
    }
  }

  // wave's own 32 keys as B operands (key on lane)
  bf16x8 kf[2][2], vf[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int64_t off = (int64_t)(k0w + 16 * r + li) * RS + 32 * kk + 8 * g;
      kf[r][kk] = live ? __builtin_bit_cast(bf16x8, *(const u32x4*)(kb + off)) : bf16x8{};
      vf[r][kk] = live ? __builtin_bit_cast(bf16x8, *(const u32x4*)(vb + off)) : bf16x8{};
    }
  // dropout: the counter of the granule this lane draws (query group mt = li & 3) in query tile 0, per row block
  [[maybe_unused]] uint64_t dseed = 0, dn4 = 0, dctr[2] = {0, 0};
  [[maybe_unused]] float dscale = 1.f;
  if constexpr (DROP) {
    dn4 = (uint64_t)(T >> 2);
    dseed = (uint64_t)dr.rng[0];
    dscale = 256.f / (float)(256u - dr.thr);
#pragma unroll
    for (int r = 0; r < 2; ++r)
      dctr[r] = (uint64_t)dr.rng[1] + ((uint64_t)bh * dn4 + (uint64_t)(4 * (li & 3) + g)) * dn4 + (uint64_t)((k0w + 16 * r + li) >> 2);
  }
  // Q / dO of a query tile: LDS-DMA into [Qk | Qm | Ok | Om] (8 KiB each); lse / -delta via registers
  float lv = 0.f;
  [[maybe_unused]] int dsv = 0;
  const float* pl = (tid < 64 ? lse2 + tid : delta + (tid - 64)) + (GQA ? ((int64_t)b * H + h) * T : (int64_t)bh * T);
  [[maybe_unused]] uint32_t hoff = 0;  // GQA: the walk's current query head inside the group, as a byte offset in a row
  const __amdgpu_buffer_rsrc_t rq =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(qb), (short)0, (int)(T * RS * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rdo =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(ob), (short)0, (int)(T * ORS * 2), 0x00020000);
  uint32_t voff[8];  // piece w + 4 i of the 32 KiB image set: i < 4 Q, else dO; (i & 2) permuted-row image
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int oo = ((w + 4 * i) * 1024 + lane * 16) & 8191;  // byte slot inside its 8 KiB image
    int row, dc;
    if ((i & 2) == 0) {  // K-contiguous halves: (dc >> 2) * 4096 + kimg(row, dc & 3)
      const int o2 = oo & 4095;
      row = o2 >> 6;
      dc = 4 * (oo >> 12) + (((o2 >> 4) & 3) ^ ((0x78 >> (((row >> 2) & 3) << 1)) & 3));
    } else {             // permuted-row image: pimg(row, dc)
      row = oo >> 7;
      dc = ((oo >> 4) & 7) ^ (((row >> 1) & 3) << 1);
    }
    voff[i] = (uint32_t)(((int64_t)row * (i < 4 ? RS : ORS) + dc * 8) * 2);
  }
  auto dma_tile = [&](int qt, int buf) {
    char* base = smem + buf * BUF;
    const uint32_t sq = (uint32_t)((int64_t)qt * AQ * RS * 2) + (GQA ? hoff : 0u);
    const uint32_t so = (uint32_t)((int64_t)qt * AQ * ORS * 2) + (GQA ? hoff : 0u);
#pragma unroll
    for (int i = 0; i < 8; ++i) attn_dma16(i < 4 ? rq : rdo, base + (w + 4 * i) * 1024, voff[i], i < 4 ? sq : so);
    if (tid < 128) lv = pl[qt * AQ];
    if constexpr (PACKED)
      if (tid >= 128 && tid < 192) dsv = doc_start[(int64_t)b * T + qt * AQ + (tid - 128)];
  };
  auto stash = [&](int buf) {  // after the tile's DMA has landed (attn_vm_drain)
    if (tid < 128) ((float*)(smem + buf * BUF + 4 * 8192))[tid] = tid < 64 ? lv : -lv;  // [0,64) lse, [64,128) -delta
    if constexpr (PACKED)
      if (tid >= 128 && tid < 192) ((int*)(smem + buf * BUF + 4 * 8192 + 512))[tid - 128] = dsv;
  };
  const int qs = BIDIR ? 0 : (kt * BKW) / AQ;
  // packed: the exclusive end of the workgroup's query-tile loop (clamped into the causal walk) and the wave's last tile
  // (bidirectional: the tiles that hold a query < L)
  int qend = BIDIR ? (L + AQ - 1) / AQ : nqt, qhiw = nqt;
  if constexpr (PACKED) {
    const int* deb = doc_end + (int64_t)b * T;
    const int ew = __builtin_amdgcn_readfirstlane(deb[min(kt * BKW + BKW - 1, T - 1)]);
    qend = min(max((max(ew, 1) - 1) / AQ + 1, qs + 1), nqt);
    if (live) qhiw = (max(__builtin_amdgcn_readfirstlane(deb[k0w + 31]), 1) - 1) / AQ;
  }
  // window: key j is seen by the queries j .. j + window - 1 (a query's lower bound is an upper bound on the query per key),
  // so the workgroup's loop ends at the tile of its last key's last query, a wave's at its own
  if constexpr (WINDOW) {
    qend = min(qend, min(T - 1, kt * BKW + BKW - 1 + window - 1) / AQ + 1);
    qhiw = min(qhiw, (k0w + 31 + window - 1) / AQ);
  }
  // GQA: tiles of the flattened (head, query tile) walk that are still to be computed
  [[maybe_unused]] int left = GQA ? (H / Hkv) * (qend - qs) : 0;
  dma_tile(qs, 0);
  attn_vm_drain();
  stash(0);
  f32x4 dk[2][4], dv[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int d = 0; d < 4; ++d) { dk[r][d] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[r][d] = dk[r][d]; }
  wg_barrier();

  // the tile loop unrolled by two: the LDS buffer of each step is a compile-time constant, so every
  // fragment address is a hoisted per-lane offset plus an immediate
  auto step = [&](int qt, auto bufc) {
    constexpr int cur = decltype(bufc)::value;
    [[maybe_unused]] int qn = qt + 1;
    if constexpr (GQA) {
      --left;
      if (qn == qend && left > 0) {  // the head's last tile: the next head's first tile goes into the other buffer
        qn = qs;
        hoff += AD * 2;
        pl += T;
      }
    }
    const bool more = GQA ? left > 0 : qt + 1 < qend;
    if (more) dma_tile(GQA ? qn : qt + 1, cur ^ 1);  // in flight during this tile's MFMAs (cur ^ 1 last read before the previous barrier)
    // maskc: 0 no mask, 1 causal mask, 2 (packed only) causal and document-start mask, 3 (bidirectional only) query < L
    auto compute = [&](const char* base, auto maskc) __attribute__((always_inline)) {
      constexpr int MK = decltype(maskc)::value;
      constexpr bool MASK = MK == 1;
      const char* Qk = base;
      const char* Qm = base + 8192;
      const char* Ok = base + 2 * 8192;
      const char* Om = base + 3 * 8192;
      const float* sl = (const float*)(base + 4 * 8192);
      const float* snd = sl + 64;
      // S[q][key], dP[q][key] - delta[q]: lane = key, rows q = 16mt + 4g + e (the dP chain starts
      // from -delta, so dS = P * dP' needs no subtraction)
      // dropout: key on the lane, so of each of its 8 granules the lane needs byte (key % 4) of all four words.
      // Lane c of the quad draws the granule of query group mt = c (per row block) and turns its bytes (word c' :=
      // byte c' of words 0..3); the quad transpose then leaves dm[r][mt] = the lane's four bytes of granule mt.
      [[maybe_unused]] uint32_t dm[2][4];
      if constexpr (DROP) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const u32x4 a = philox4x32(dseed, dctr[r] + (uint64_t)(uint32_t)(qt * (AQ / 4)) * dn4, dr.stream);
#pragma unroll
          for (int c = 0; c < 4; ++c)
            dm[r][c] = ((a[0] >> (8 * c)) & 0xffu) | (((a[1] >> (8 * c)) & 0xffu) << 8) | (((a[2] >> (8 * c)) & 0xffu) << 16) |
                       (((a[3] >> (8 * c)) & 0xffu) << 24);
          quad_transpose(dm[r], li & 3);
        }
      }
      f32x4 ps[2][4], dp[2][4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const bf16x8 q0 = kfrag64(Qk, 16 * mt), q1 = kfrag64(Qk + 4096, 16 * mt);
        const bf16x8 o0 = kfrag64(Ok, 16 * mt), o1 = kfrag64(Ok + 4096, 16 * mt);
        f32x4 nd4 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (!DROP) nd4 = *(const f32x4*)(snd + 16 * mt + 4 * g);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          ps[r][mt] = MFMA(q1, kf[r][1], MFMA(q0, kf[r][0], (f32x4{0.f, 0.f, 0.f, 0.f})));
          dp[r][mt] = MFMA(o1, vf[r][1], MFMA(o0, vf[r][0], nd4));
        }
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const f32x4 l4 = *(const f32x4*)(sl + 16 * mt + 4 * g);
        [[maybe_unused]] u32x4 d4;
        if constexpr (MK == 2 && PACKED) d4 = *(const u32x4*)(base + 4 * 8192 + 512 + 4 * (16 * mt + 4 * g));
        [[maybe_unused]] f32x4 ndd;
        if constexpr (DROP) ndd = *(const f32x4*)(snd + 16 * mt + 4 * g);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float p = __builtin_amdgcn_exp2f(fmaf(ps[r][mt][e], sl2, -l4[e]));
            if constexpr (MASK)
              if (k0w + 16 * r + li > qt * AQ + 16 * mt + 4 * g + e) p = 0.f;
            if constexpr (MK == 2) {  // the key is behind the query, or the query's document starts behind the key
              const int key = k0w + 16 * r + li;
              if constexpr (PACKED) p = ((key > qt * AQ + 16 * mt + 4 * g + e) | ((int)d4[e] > key)) ? 0.f : p;
              if constexpr (WINDOW) {  // the window's edge of the query is behind the key (with the causal bound when not packed)
                const int q = qt * AQ + 16 * mt + 4 * g + e;
                p = ((!PACKED & (key > q)) | (q - window + 1 > key)) ? 0.f : p;
              }
            }
            if constexpr (DROP) {
              const bool keep = drop_keep(dm[r][mt], e, dr.thr);
              ps[r][mt][e] = keep ? p : 0.f;                                   // P o M (s in the final dV)
              dp[r][mt][e] = p * fmaf(dp[r][mt][e], keep ? dscale : 0.f, ndd[e]);  // dS = P (M s dP - delta)
            } else if constexpr (MK == 3) {  // a padding query: P and dS are 0 by select, whatever its lse / dO hold
              const bool vis = qt * AQ + 16 * mt + 4 * g + e < L;
              ps[r][mt][e] = vis ? p : 0.f;
              dp[r][mt][e] = vis ? p * dp[r][mt][e] : 0.f;
            } else {
              ps[r][mt][e] = p;                        // P
              dp[r][mt][e] = p * dp[r][mt][e];  // dS (unscaled)
            }
          }
      }
      // dV^T += dO^T . P ; dK^T += Q^T . dS   (k = q, permuted order matches the accumulators)
      bf16x8 pp[2][2], ss[2][2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        pp[r][0] = pack_frag(ps[r][0], ps[r][1]); pp[r][1] = pack_frag(ps[r][2], ps[r][3]);
        ss[r][0] = pack_frag(dp[r][0], dp[r][1]); ss[r][1] = pack_frag(dp[r][2], dp[r][3]);
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const bf16x8 a0 = trfrag(Om, 0, 16 * d), a1 = trfrag(Om, 32, 16 * d);
        const bf16x8 c0 = trfrag(Qm, 0, 16 * d), c1 = trfrag(Qm, 32, 16 * d);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          dv[r][d] = MFMA(a1, pp[r][1], MFMA(a0, pp[r][0], dv[r][d]));
          dk[r][d] = MFMA(c1, ss[r][1], MFMA(c0, ss[r][0], dk[r][d]));
        }
      }
    };
    // query tiles whose first query is past the wave's last key need no causal mask
    if constexpr (PACKED || WINDOW) {
      if (live && qt >= qtw && qt <= qhiw) {
        // doc_start is monotone: the tile's last query has the largest (and the latest window edge)
        int dlast = 0;
        if constexpr (PACKED) dlast = __builtin_amdgcn_readfirstlane(((const int*)(smem + cur * BUF + 4 * 8192 + 512))[AQ - 1]);
        if constexpr (WINDOW) dlast = max(dlast, qt * AQ + AQ - window);
        if (dlast > k0w) compute(smem + cur * BUF, std::integral_constant<int, 2>{});
        else if (qt * AQ >= k0w + 31) compute(smem + cur * BUF, std::integral_constant<int, 0>{});
        else compute(smem + cur * BUF, std::integral_constant<int, 1>{});
      }
    } else if constexpr (BIDIR) {
      if (k0w < L) {  // a wave past L only stages its pieces of the tiles
        // the query tiles below qfull are full; kept in a VGPR for a per-wave branch, as kd in attn_fwd_dma_kernel
        // (306 -> 234 VGPRs: two waves per SIMD)
        int qfull = L / AQ;
        asm volatile("" : "+v"(qfull));
        if (qt < qfull) compute(smem + cur * BUF, std::integral_constant<int, 0>{});
        else compute(smem + cur * BUF, std::integral_constant<int, 3>{});
      }
    } else if (live && qt >= qtw) {
      if (qt * AQ >= k0w + 31) compute(smem + cur * BUF, std::integral_constant<int, 0>{});
      else compute(smem + cur * BUF, std::integral_constant<int, 1>{});
    }
    if (more) {
      attn_vm_drain();
      stash(cur ^ 1);
    }
    wg_barrier();
    if constexpr (GQA) return qn;
  };
  if constexpr (GQA) {
    for (int qt = qs; left > 0;) {
      qt = step(qt, std::integral_constant<int, 0>{});
      if (left > 0) qt = step(qt, std::integral_constant<int, 1>{});
    }
  } else {
    for (int qt = qs; qt < qend; qt += 2) {
      step(qt, std::integral_constant<int, 0>{});
      if (qt + 1 < qend) step(qt + 1, std::integral_constant<int, 1>{});
    }
  }
  if (!live) return;
  // dK, dV (bf16) -> dqkv[b, key, 1|2, h, :] (GQA: the K / V head hk behind the Hq query heads)
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    uint16_t* dkb = dqkv + (int64_t)b * T * RS + (int64_t)(k0w + 16 * r + li) * RS + H * AD + (int64_t)(GQA ? hk : h) * AD;
    uint16_t* dvb = dkb + (GQA ? Hkv : H) * AD;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      u32x2 a, c;
      a[0] = pack_bf2(dk[r][d][0] * scale, dk[r][d][1] * scale);
      a[1] = pack_bf2(dk[r][d][2] * scale, dk[r][d][3] * scale);
      if constexpr (DROP) dv[r][d] *= dscale;
      c[0] = pack_bf2(dv[r][d][0], dv[r][d][1]);
      c[1] = pack_bf2(dv[r][d][2], dv[r][d][3]);
      if constexpr (BIDIR) {
        const bool vis = k0w + 16 * r + li < L;
        a = vis ? a : u32x2{0u, 0u};
        c = vis ? c : u32x2{0u, 0u};
      }
      *(u32x2*)(dkb + 16 * d + 4 * g) = a;
      *(u32x2*)(dvb + 16 * d + 4 * g) = c;
    }
  }
