// The body of gram_sia_kernel (gram.hip, which documents it), kept as text so that the kernel on an
// fp32-stored A (gram_sia_ta_kernel) is the same statements over another element type.  In scope at
// the point of inclusion: TA (element type of A), PIPE, TI, CM, AV, BND and the kernel's parameters.
// Only the staging depends on TA: gload keeps the pairs as loaded and swrite widens them (exactly) on
// their way to LDS; column-major operands are fp64.
  static_assert(!(AV && CM), "the fused Aᵀv runs on the panel-blocked A only");
  static_assert(!CM || sizeof(TA) == sizeof(double), "column-major operands are fp64");
  constexpr int GTI = 64 * TI;        // tile rows (A1 features)
  constexpr int NT = 128 * TI;        // threads
  constexpr int FS = NT / 8;          // features per staging sweep
  constexpr int NTI = 4;              // 16-row MFMA tiles per wave along i
  constexpr int NA = GTI / FS;        // A1 staging chunks per thread per stage (4)
  constexpr int NB = GT / FS;         // A2 staging chunks per thread per stage (4 or 2)
  constexpr int NMM = 2 * NTI * 4;    // MFMAs per fragment set (2 u x NTI x 4)
  constexpr int NRD = NTI + 4;        // ds_read_b128 per fragment set
  constexpr int TAIL = NMM / 4;       // MFMAs left for phase 2b (1/8 and 3/8 measured within noise)
  // PIPE >= 8: the interleaved schedule with the issue order at the stage barriers changed (the MFMA
  // order per accumulator is untouched), one bit per edge:
  //   1 (E1) phase 1: each fragment read ahead of its MFMA group (the last read has a group behind
  //          it before lgkmcnt(0), not the barrier);
  //   2 (E2) phase 2a head: one MFMA group ahead of the vmcnt wait, the w products and the addresses;
  //   4 (E3) phase 2a tail: each ds_write ahead of its MFMA group.
  // PIPE bit 16 (with 8 + bits) keeps the staging loads on per-lane 64-bit addresses (SB below).
  constexpr int EP = PIPE & 15;
  constexpr bool E1 = EP >= 8 && (EP & 1), E2 = EP >= 8 && (EP & 2), E3 = EP >= 8 && (EP & 4);
  // pair items (gram_tiles.h: the D1 blocks of two row blocks in one 256 x 128 tile) are decoded by
  // the panel-blocked 256 x 128 kernels; their A2 stage block is the A1 block times w (256 rows)
  constexpr bool PAIRT = TI == 4 && !CM && !BND;
  constexpr int LBR = PAIRT ? GTI : GT;   // rows of the A2 stage block
  constexpr int NAV = PAIRT ? NA : NB;    // Aᵀv chunks per thread per stage
  const int packed = flags & GRAM_PACKED, accumulate = flags & GRAM_ACCUMULATE, upper = flags & GRAM_UPPER;
  __shared__ __attribute__((aligned(16))) double lds[(GTI + LBR) * GBK];
  const int orig = blockIdx.x;
  const int xcd = orig % 8;
  int bi, bj, tix, part = -1, piece = 0;
  __shared__ int s_claim;
  if constexpr (BND) {   // counters in scnt, skip mask in sob (bnd_first)
    tix = bnd_first(scnt, (unsigned)sob, ntiles, &s_claim);
    if (tix < 0 || tix >= ntiles) return;
    bi = tiles[tix].x;
    bj = tiles[tix].y;
  } else if (work) {
    const int4 it = work[xcd * seglen + orig / 8];
    if (it.x < 0) return;
    bi = it.x;
    bj = it.y;
    tix = it.w;
    if (it.z >= 0) {
      piece = it.z;
      const int64_t L = ((Nk - k0 + (int64_t)nsplit * GBK - 1) / ((int64_t)nsplit * GBK)) * GBK;
      part = it.w;
      k0 = k0 + it.z * L;
      Nk = k0 + L < Nk ? k0 + L : Nk;
      if (Nk < k0) Nk = k0;
    }
  } else {
    const int q8 = ntiles / 8, r8 = ntiles % 8;
    tix = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + orig / 8;
    const int2 tl = tiles[tix];
    bi = tl.x;
    bj = tl.y;
  }
bnd_tile:
  // the A1 panels of the tile: 2 bi, 2 bi + 1 (bi at 128 rows), or the two diagonal panels of a pair
  // item, which then runs as tile "column panel pa" of rows [pa; pb]
  int pa = (GTI / GT) * bi, pb = pa + 1;
  bool pair = false;
  if constexpr (PAIRT) {
    if (gram_item_is_pair(bj)) {
      pair = true;
      gram_item_panels(bi, bj, &pa, &pb);
      bj = pa;
    }
  }
  int tid_ = threadIdx.x;
  if constexpr (BND) asm volatile("" : "+v"(tid_));   // per tile: nothing derived from it is hoisted out of the loop
  const int tid = tid_, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int sc = tid & 7, sf0 = tid >> 3;
  const int64_t st0 = k0 / GBK;
  // this thread's 16-B chunks of a stage: feature sf0 + FS i of the A1 rows (panel
  // pa or pb by f/128) and of the A2 rows (panel bj), samples 2 sc, 2 sc + 1.
  const TA* srcA = CM ? A + ((int64_t)bi * GTI + sf0) * S + k0 + 2 * sc
                      : A + ((int64_t)pa * S + st0) * GT * GBK + sf0 * GBK + 2 * sc;
  const int64_t pd = (int64_t)(pb - pa) * S * GT * GBK;   // from panel pa to panel pb
  // CM with A2: the A2 panels from a second column-major matrix (leading dimension S2; the LU's and
  // the QR's two-operand products, the Cholesky's strip solves), else from A
  const TA* B2 = (CM && A2) ? (const TA*)A2 : A;
  const int64_t SB2 = (CM && A2) ? S2 : S;
  const TA* srcB = CM ? B2 + ((int64_t)bj * GT + sf0) * SB2 + k0 + 2 * sc
                      : A + ((int64_t)bj * S + st0) * GT * GBK + sf0 * GBK + 2 * sc;
  const double* srcW = w + k0 + 2 * sc;
  const double* srcV = AV ? v + k0 + 2 * sc : nullptr;
  // SB, the panel-blocked kernels' staging: nothing in a staging address differs between the lanes
  // from stage to stage, so the 64-bit bases of the tile (panels pa, pb, bj, w, v at stage st0) stay
  // in SGPRs and advance by scalar adds, each load is a raw buffer load through a descriptor built
  // on its stage window (one 128 x 16 block of a panel; 128 B of w / v), and a lane adds one
  // constant 32-bit byte offset (vo for A, vw for w / v) and the chunk's uniform offset (soffset).
  // No offset grows with K: a panel passes 4 GiB above 4 M rows.  The loop then holds no VALU
  // address arithmetic; the values loaded, and all that follows them, are the pointer form's.  The
  // bases pass through readfirstlane, so that no load is wrapped in a waterfall loop.
  constexpr bool SB = !CM && !(PIPE & 16);
  constexpr int STB = GT * GBK * (int)sizeof(TA);   // bytes of one panel's stage block
  auto uni = [](const void* p) {
    const uint64_t x = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
    return (const char*)((uint64_t)hi << 32 | lo);
  };
  const char* const ubA = SB ? uni(A + ((int64_t)pa * S + st0) * GT * GBK) : nullptr;
  const char* const ubP = SB ? uni(A + ((int64_t)pb * S + st0) * GT * GBK) : nullptr;
  const char* const ubB = SB ? uni(A + ((int64_t)bj * S + st0) * GT * GBK) : nullptr;
  const char* const ubW = SB ? uni(w + k0) : nullptr;
  const char* const ubV = SB && AV ? uni(v + k0) : nullptr;
  const int vo = (sf0 * GBK + 2 * sc) * (int)sizeof(TA), vw = 2 * sc * (int)sizeof(double);
  auto window = [](const char* p, int bytes) {   // 0x00020000: the gfx9 raw-buffer word 3
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p), 0, bytes, 0x00020000);
  };
  double* la = lds;
  double* lb = lds + GTI * GBK;
  int woff[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int f = sf0 + FS * i;
    woff[i] = f * GBK + 2 * (sc ^ swz(f));
  }
  // the staged chunks as loaded (TA pairs): an fp32-stored A is widened when they are written to LDS
  typedef typename pair_of<TA>::type PR;
  PR ra[NA], rb[NB];
  v2d rw, rv;
  double av[NAV];
#pragma unroll
  for (int i = 0; i < NAV; ++i) av[i] = 0.0;
  // fa: std::bool_constant -- the designated tiles of an AV launch run the loop with the Aᵀv
  // products (FA), every other tile the plain loop (no extra loads or VALU)
  // pt: std::bool_constant -- a pair tile (no A2 loads: its A2 rows are its A1 rows)
  auto gload = [&](int64_t st, auto fa, auto pt) {
    constexpr bool FA = decltype(fa)::value, PT = decltype(pt)::value;
    if (PIPE == 3 && st >= 2) return;   // timing build: no global loads after the prologue
    if (CM) {
#pragma unroll
      for (int i = 0; i < NA; ++i) ra[i] = *(const PR*)(srcA + st * GBK + (int64_t)FS * i * S);
#pragma unroll
      for (int i = 0; i < NB; ++i) rb[i] = *(const PR*)(srcB + st * GBK + (int64_t)FS * i * SB2);
    } else if constexpr (SB) {
      auto bload = [](auto d, int voff, int soff) {   // b128 for fp64 pairs, b64 for fp32 pairs
        if constexpr (sizeof(PR) == 16) return __builtin_bit_cast(PR, __builtin_amdgcn_raw_buffer_load_b128(d, voff, soff, 0));
        else return __builtin_bit_cast(PR, __builtin_amdgcn_raw_buffer_load_b64(d, voff, soff, 0));
      };
      const int64_t so = st * STB;
      const auto da = window(ubA + so, STB), dp = window(ubP + so, STB);
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int f = FS * i;   // + sf0 (in vo): the panel of f is f / 128 (FS divides 128)
        ra[i] = bload((f >> 7) ? dp : da, vo, (f & 127) * GBK * (int)sizeof(TA));
      }
      if (!PT) {
        const auto db = window(ubB + so, STB);
#pragma unroll
        for (int i = 0; i < NB; ++i) rb[i] = bload(db, vo, FS * GBK * i * (int)sizeof(TA));
      }
      constexpr int WB = GBK * (int)sizeof(double);
      rw = __builtin_bit_cast(v2d, __builtin_amdgcn_raw_buffer_load_b128(window(ubW + st * WB, WB), vw, 0, 0));
      if (FA) rv = __builtin_bit_cast(v2d, __builtin_amdgcn_raw_buffer_load_b128(window(ubV + st * WB, WB), vw, 0, 0));
      return;
    } else {
      const int64_t so = st * GT * GBK;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int f = FS * i;   // + sf0 (in srcA): the panel of f is f / 128 (FS divides 128)
        ra[i] = *(const PR*)(srcA + so + (f >> 7) * pd + (f & 127) * GBK);
      }
      if (!PT) {
#pragma unroll
        for (int i = 0; i < NB; ++i) rb[i] = *(const PR*)(srcB + so + FS * GBK * i);
      }
    }
    rw = *(const v2d*)(srcW + st * GBK);
    if (FA) rv = *(const v2d*)(srcV + st * GBK);
  };
  auto swrite = [&](auto fa, auto pt) {
    constexpr bool FA = decltype(fa)::value, PT = decltype(pt)::value;
#pragma unroll
    for (int i = 0; i < NA; ++i) *(v2d*)(la + woff[i]) = widen(ra[i]);
    if constexpr (PT) {   // lb = the same chunks times w; chunk i is today's rb[i % NB] of its panel
#pragma unroll
      for (int i = 0; i < NA; ++i) *(v2d*)(lb + woff[i]) = widen(ra[i]) * rw;
      if (FA) {
#pragma unroll
        for (int i = 0; i < NAV; ++i) {
          const v2d b = widen(ra[i]);
          av[i] = __builtin_fma(b[1], rv[1], __builtin_fma(b[0], rv[0], av[i]));
        }
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) *(v2d*)(lb + woff[i]) = widen(rb[i]) * rw;
    if (FA) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const v2d b = widen(rb[i]);
        av[i] = __builtin_fma(b[1], rv[1], __builtin_fma(b[0], rv[0], av[i]));
      }
    }
  };
  const int fl = lane & 15, g = lane >> 4, s = swz(fl);
  // this wave's A2 rows: column half wc of the tile; in a pair tile, of the D block its rows lie in
  const int brow = wc * 64 + (pair ? (wr >> 1) * GT : 0);
  struct Frag {
    v2d a[NTI], b[4];
  };
  auto fread = [&](int p, Frag& F) {
    const int pc = ((4 * p + g) ^ s) * 2;
#pragma unroll
    for (int t = 0; t < NTI; ++t) F.a[t] = *(const v2d*)(la + (wr * 64 + 16 * t + fl) * GBK + pc);
#pragma unroll
    for (int t = 0; t < 4; ++t) F.b[t] = *(const v2d*)(lb + (brow + 16 * t + fl) * GBK + pc);
  };
  v4d acc[NTI][4];
#pragma unroll
  for (int i = 0; i < NTI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
  // MFMAs n in [n0, n1) of a fragment set, n = 4 NTI u + 4 ti + tj (the plain loop's order)
  auto mm = [&](const Frag& F, int n0, int n1) {
#pragma unroll
    for (int n = n0; n < n1; ++n) {
      const int u = n / (4 * NTI), ti = (n / 4) % NTI, tj = n & 3;
      acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(F.a[ti][u], F.b[tj][u], acc[ti][tj], 0, 0, 0);
    }
  };
  auto barrier = [&]() {   // also a scheduling fence: nothing (e.g. the w products) crosses a phase
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): this wave's LDS traffic is done
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  const int nk = (int)((Nk - k0) / GBK);
  Frag F0, F1;
  auto run = [&](auto fa, auto pt) {
    constexpr int NW = decltype(pt)::value ? 2 * NA : NA + NB;   // ds_write_b128 per stage
    if (nk > 0) {
      gload(0, fa, pt);
      swrite(fa, pt);
      if (nk > 1) gload(1, fa, pt);
      barrier();
      fread(0, F0);
    }
    auto body = [&](int k, bool has1, bool has2) {
      // phase 1
      __builtin_amdgcn_sched_barrier(0);
      fread(1, F1);
      mm(F0, 0, NMM);
      if (PIPE) {
#pragma unroll
        for (int i = 0; i < NRD; ++i) {
          if (!E1) __builtin_amdgcn_sched_group_barrier(0x008, NMM / NRD, 0);   // MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                    // DS read
          if (E1) __builtin_amdgcn_sched_group_barrier(0x008, NMM / NRD, 0);
        }
      }
      barrier();
      // phase 2a
      if (has1) swrite(fa, pt);
      if (has2) gload(k + 2, fa, pt);
      mm(F1, 0, NMM - TAIL);
      if (PIPE) {
        if (has1) {
          constexpr int HEAD = E2 ? NMM / NRD : 0, Q = (NMM - TAIL - HEAD) / NW;
          if (E2) {
            __builtin_amdgcn_sched_group_barrier(0x008, HEAD, 0);   // MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 64, 0);     // VALU: all of the phase's
          }
#pragma unroll
          for (int i = 0; i < NW; ++i) {
            if (!E3) __builtin_amdgcn_sched_group_barrier(0x008, Q, 0);    // MFMA
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);             // DS write
            if (has2) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
            if (E3) __builtin_amdgcn_sched_group_barrier(0x008, Q, 0);
          }
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NMM, 0);
      }
      // phase 2b
      if (has1) {
        barrier();
        fread(0, F0);
      }
      mm(F1, NMM - TAIL, NMM);
      if (PIPE && has1) {
#pragma unroll
        for (int i = 0; i < NRD; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, TAIL / NRD > 0 ? TAIL / NRD : 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
      }
    };
    int k = 0;
    for (; k + 2 < nk; ++k) body(k, true, true);
    if (k + 1 < nk) {
      body(k, true, false);
      ++k;
    }
    if (k < nk) body(k, false, false);
  };
  // this tile owns panel bj's Aᵀv rows; a pair tile those of both its panels
  const bool dav = AV && (pair || (int64_t)bj * GT / GTI == bi);
  if constexpr (PAIRT) {
    if (pair) run(std::bool_constant<AV>{}, std::true_type{});
    else if (dav) run(std::bool_constant<AV>{}, std::false_type{});
    else run(std::false_type{}, std::false_type{});
  } else if constexpr (AV) {
    if (dav) run(std::true_type{}, std::false_type{});
    else run(std::false_type{}, std::false_type{});
  } else {
    run(std::false_type{}, std::false_type{});
  }

  if (dav) {   // lanes 8q .. 8q+7 share a feature
#pragma unroll
    for (int i = 0; i < NAV; ++i) {
      if (i >= NB && !pair) continue;   // chunks NB.. : panel pb of a pair tile (bj = pa there)
      double t = av[i];
      t += __shfl_xor(t, 1);
      t += __shfl_xor(t, 2);
      t += __shfl_xor(t, 4);
      const int64_t row = i < NB ? (int64_t)bj * GT + sf0 + FS * i : (int64_t)pb * GT + sf0 + FS * (i - NB);
      if (sc == 0) VP[(int64_t)piece * vps + row] = t;
    }
  }

  // epilogue (the C/D map of gram_f64_kernel): element (il, jl) of the GTI x 128 tile, at
  // (grow + il, gcol + jl); the rows of a pair tile go to block (pa, pa) or (pb, pb) by their half
  const int pw = (wr >> 1) ? pb : pa;
  const int64_t grow = pair ? (int64_t)(pw - (wr >> 1)) * GT : (int64_t)bi * GTI;
  const int64_t gcol = pair ? (int64_t)pw * GT : (int64_t)bj * GT;
  if constexpr (BND || CM) {   // the persistent and gen-form launches: old values loaded ahead of the stores
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti)
      gram_tile_store_row(acc[ti], ti, wr, wc, g, fl, part, P, GTI, packed, upper, accumulate, G, ldg, tix, bi, bj);
  } else {
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti)
#pragma unroll
      for (int tj = 0; tj < 4; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int il = wr * 64 + 16 * ti + g + 4 * r;
          const int jl = wc * 64 + 16 * tj + fl;
          double* dst;
          if (part >= 0) {
            P[((int64_t)part * GT + jl) * GTI + il] = acc[ti][tj][r];
            continue;
          }
          if (packed) dst = G + ((int64_t)tix * (GTI / GT) + il / GT) * GT * GT + jl * GT + (il % GT);
          else if (upper) dst = G + (grow + il) * ldg + gcol + jl;
          else dst = G + (gcol + jl) * ldg + grow + il;
          if (accumulate) *dst += acc[ti][tj][r];
          else *dst = acc[ti][tj][r];
        }
  }
  // strip completion (scsopt.cpp gram_factor_pipelined, one-launch mode): this tile's rows lie in
  // outer strip bj / sob; each thread's stores are released to device scope before one count
  if (!BND && scnt && part < 0) {
    __threadfence();
    __syncthreads();
    if (tid == 0) atomicAdd(scnt + bj / sob, 1u);
  }
  if constexpr (BND) {
    tix = bnd_next(scnt, ntiles, &s_claim);
    if (tix >= ntiles) return;
    bi = tiles[tix].x;
    bj = tiles[tix].y;
    goto bnd_tile;
  }
