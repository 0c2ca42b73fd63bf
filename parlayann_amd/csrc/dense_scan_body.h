// dense_scan_body.h -- the body of dense_scan_mfma_kernel (dense.hip), included once per form: DT, NR and LIST are the including
// kernel's constants, A / bnorm / gtau its arguments.  Not a translation unit and not a header of its own.
  constexpr bool L2 = scan_is_l2(DT);
  extern __shared__ __align__(16) uint8_t smem[];
  const uint32_t nch = (A.dbytes + 15) / 16;                              // 16-byte chunks that hold data: 1 .. 32 (the launcher checks)
  const uint32_t nseg = (nch + 15) / 16;
  uint8_t* Bt0 = smem;                                                    // [2][64][GT_BSTRIDE], slots swizzled (gt_swz)
  float2* Bm = reinterpret_cast<float2*>(smem + 2 * GT_BT_BYTES);         // [2][64] (|b|^2 bits, id bits)
  int* An = reinterpret_cast<int*>(Bm + 2 * DT_B);                        // [64] |a|^2 (L2)
  uint8_t* At = reinterpret_cast<uint8_t*>(An + DT_A);                    // [nseg][64][GT_BSTRIDE], swizzled like B
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4;
  const TileGeom g = LIST ? dense_geom(A, DT_B) : tile_geom(A.na, A.nb, piece_rows(A.nb, A.nsplit, DT_B));
  const uint64_t a0 = g.a0, bs = g.bs, be = g.be; const uint32_t na_tile = g.na_tile;
  const uint32_t ntile = (uint32_t)((be - bs + DT_B - 1) / DT_B);
  const int r0 = tid >> 4, c = tid & 15;
  // the A tile -> LDS (rows beyond the tile and bytes beyond the row: zeros), PANN_U8 moved; |a|^2 of the bytes the k steps cover
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int ss = 0;
    for (uint32_t sg = 0; sg < nseg; sg++) {
      uint4 v = dense_a_load(A, g, r0 + 16 * k, sg * DT_SEG + c * 16);
      if (L2 && sg * 16u + (uint32_t)c < nch) ss += scan_chunk_sq<DT>(v);
      if constexpr (DT == PANN_U8) v = scan_flip7(v);
      *reinterpret_cast<uint4*>(At + sg * GT_BT_BYTES + gt_swz((uint32_t)(r0 + 16 * k), (uint32_t)c * 16u)) = v;
    }
    if constexpr (L2) { ss = group_sum<16>(ss) + scan_pad_sq<DT>(nch); if (c == 0) An[r0 + 16 * k] = ss; }
  }
  GtSel<NR> S;
  gt_sel_init<NR>(S, A.m, (uint32_t)(wave * DT_AW + q * 4), na_tile, lane);
  // pipeline step u = (tile u / nseg, segment u % nseg), buffer u & 1 (dense_gt_valu_kernel): with two segments buffer b always
  // holds segment b.  A chunk column that holds no data is never staged: it is zeroed here, once, in both buffers.
  const bool cv0 = (uint32_t)c < nch, cv1 = nseg == 2 && 16u + (uint32_t)c < nch;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (!((nseg == 2 && (k >> 2)) ? cv1 : cv0))
      *reinterpret_cast<uint4*>(Bt0 + (k >> 2) * GT_BT_BYTES + gt_swz((uint32_t)(r0 + 16 * (k & 3)), (uint32_t)c * 16u)) = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();
  int an[4] = {0, 0, 0, 0};
  if constexpr (L2) {
#pragma unroll
    for (int r = 0; r < 4; r++) an[r] = An[wave * DT_AW + q * 4 + r];
  }
  const uint32_t pplace = 16u * NR - A.m + (A.m + A.nsplit - 1) / A.nsplit - 1;
  const uint32_t skip[4] = {SENTINEL, SENTINEL, SENTINEL, SENTINEL};
  const uint32_t tau_period = GT_TAU_PERIOD * ((A.nsplit + 7) / 8);
  uint32_t tau_wait = tau_period;
  uint32_t* gtau_mine = gtau + (a0 + wave * DT_AW + q * 4) * A.nsplit + blockIdx.y;

  const uint32_t nunits = ntile * nseg;
  const uint32_t last_row = (uint32_t)(be - 1);                           // (read only where a load is issued: be > bs there)
  const uint8_t* cb0 = A.points + min((uint32_t)c, nch - 1u) * 16u;
  const uint8_t* cb1 = A.points + min(16u + (uint32_t)c, nch - 1u) * 16u;
  uint4 pre0, pre1, pre2, pre3;
  int pn = 0;
  auto unit_bt = [&](uint32_t u) -> uint32_t { return (uint32_t)bs + (nseg == 2 ? (u >> 1) : u) * DT_B; };
  [[maybe_unused]] uint32_t nid0 = 0, nid1 = 0, nid2 = 0, nid3 = 0, pid = 0;      // LIST: the row ids load_pre turns into addresses; the id of Bm
  [[maybe_unused]] auto load_ids = [&](uint32_t u) {      // LIST: requested one step before the rows they address; clamped positions
    const uint32_t bt = unit_bt(u);
    nid0 = A.b_ids[min(bt + (uint32_t)r0, last_row)];
    nid1 = A.b_ids[min(bt + (uint32_t)r0 + 16u, last_row)];
    nid2 = A.b_ids[min(bt + (uint32_t)r0 + 32u, last_row)];
    nid3 = A.b_ids[min(bt + (uint32_t)r0 + 48u, last_row)];
  };
  auto load_pre = [&](uint32_t u) {          // requests only: clamped rows, no branch around a load
    const uint32_t bt = unit_bt(u);
    const uint8_t* cb = (nseg == 2 && (u & 1)) ? cb1 : cb0;
    if constexpr (LIST) {
      pre0 = *reinterpret_cast<const uint4*>(cb + (uint64_t)nid0 * A.pstride);
      pre1 = *reinterpret_cast<const uint4*>(cb + (uint64_t)nid1 * A.pstride);
      pre2 = *reinterpret_cast<const uint4*>(cb + (uint64_t)nid2 * A.pstride);
      pre3 = *reinterpret_cast<const uint4*>(cb + (uint64_t)nid3 * A.pstride);
      pid = A.b_ids[min(bt + (uint32_t)lane, last_row)];
    } else {
      pre0 = *reinterpret_cast<const uint4*>(cb + (uint64_t)min(bt + (uint32_t)r0, last_row) * A.pstride);
      pre1 = *reinterpret_cast<const uint4*>(cb + (uint64_t)min(bt + (uint32_t)r0 + 16u, last_row) * A.pstride);
      pre2 = *reinterpret_cast<const uint4*>(cb + (uint64_t)min(bt + (uint32_t)r0 + 32u, last_row) * A.pstride);
      pre3 = *reinterpret_cast<const uint4*>(cb + (uint64_t)min(bt + (uint32_t)r0 + 48u, last_row) * A.pstride);
    }
    if (L2) pn = bnorm[min(bt + (uint32_t)lane, last_row)];
  };
  auto store_pre = [&](uint32_t u) {
    const int buf = (int)(u & 1);
    gt_store_tile(Bt0 + buf * GT_BT_BYTES, Bm + buf * DT_B, (nseg == 2 && (u & 1)) ? cv1 : cv0, pre0, pre1, pre2, pre3, __int_as_float(pn),
                  unit_bt(u), be, tid);
    // LIST: a row is labelled with its id, not its position (a position at or beyond `be` stays SENTINEL)
    if constexpr (LIST) { if (tid < DT_B && (uint64_t)unit_bt(u) + tid < be) Bm[buf * DT_B + tid].y = __uint_as_float(pid); }
  };
  if (nunits > 0) {
    if constexpr (LIST) load_ids(0);
    load_pre(0); store_pre(0);
    if constexpr (LIST) load_ids(1);
    load_pre(1);
    if constexpr (LIST) load_ids(2);
  }
  lds_barrier();

  mf_int4 acc[4];
  const uint32_t arow = (uint32_t)(wave * DT_AW + (lane & 15));
  for (uint32_t u = 0; u < nunits; u++) {
    const int buf = (int)(u & 1);
    const uint32_t sg = nseg == 2 ? (u & 1) : 0u;
    if (sg == 0 && A.nsplit > 1 && --tau_wait == 0) { tau_wait = tau_period; gt_sel_refresh<NR>(S, gtau + a0 * A.nsplit, (uint32_t)(wave * DT_AW + q * 4), na_tile, A.nsplit, lane); }
    store_pre(u + 1);                                          // (beyond the last step: the piece's last row again, into a dead buffer)
    load_pre(u + 2);
    if constexpr (LIST) load_ids(u + 3);
    if (sg == 0) {
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = mf_int4{0, 0, 0, 0};
    }
    const uint8_t* Bt = Bt0 + buf * GT_BT_BYTES;
    const uint8_t* Ap = At + sg * GT_BT_BYTES;
    const uint32_t nks = (min(16u, nch - sg * 16u) + 3u) / 4u;              // k steps of 64 row bytes that reach data in this segment
    for (uint32_t ks = 0; ks < nks; ks++) {
      const uint32_t off = ks * 64u + (uint32_t)q * 16u;
      uint4 braw[4];
#pragma unroll
      for (int t = 0; t < 4; t++) braw[t] = *reinterpret_cast<const uint4*>(Bt + gt_swz((uint32_t)(t * 16 + (lane & 15)), off));
      scan_mfma_step<DT>(*reinterpret_cast<const uint4*>(Ap + gt_swz(arow, off)), braw, acc);
    }
    if (sg == nseg - 1) {
      // ---- epilogue: acc[t][r] = a(row wave*16 + 4q + r) . b(column t*16 + (lane & 15)) ----
      int bn[4]; uint32_t bid[4];
#pragma unroll
      for (int t = 0; t < 4; t++) { const float2 m2 = Bm[buf * DT_B + t * 16 + (lane & 15)]; bn[t] = __float_as_int(m2.x); bid[t] = __float_as_uint(m2.y); }
      float dist[4][4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
          if constexpr (L2) dist[r][t] = (float)(an[r] + bn[t] - 2 * acc[t][r]);
          else dist[r][t] = -(float)acc[t][r];
        }
      }
      gt_select<NR>(S, dist, bid, skip, pplace, gtau_mine, A.nsplit, lane);
    }
    lds_barrier();
  }
  gt_sel_write<NR>(S, A.partial + ((a0 + wave * DT_AW + q * 4) * A.nsplit + blockIdx.y) * A.m, A.m, A.nsplit, lane);
