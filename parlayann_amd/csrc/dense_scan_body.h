// dense_scan_body.h -- the body of dense_scan_mfma_kernel (dense.hip), included once per form: DT, NR, LIST and PQ are the including
// kernel's constants, A / bnorm / gtau / F its arguments.  Not a translation unit and not a header of its own.
// PQ (DESIGN.md "Per-query filtered scan"): MASK_NONE, or every A row has a filter of its own -- MASK_BITMAP: row a0 + r of F.allow
// (F.stride words apart), MASK_LABELS: predicate a0 + r of F.preds over F.labels -- that decides per (row, column) cell, between the
// accumulators and gt_select, whether the cell may enter the row's list.  Contiguous B only.
  constexpr bool L2 = scan_is_l2(DT);
  extern __shared__ __align__(16) uint8_t smem[];
  const uint32_t nch = (A.dbytes + 15) / 16;                              // 16-byte chunks that hold data: 1 .. 32 (the launcher checks)
  const uint32_t nseg = (nch + 15) / 16;
  uint8_t* Bt0 = smem;                                                    // [2][64][GT_BSTRIDE], slots swizzled (gt_swz)
  float2* Bm = reinterpret_cast<float2*>(smem + 2 * GT_BT_BYTES);         // [2][64] (|b|^2 bits, id bits)
  int* An = reinterpret_cast<int*>(Bm + 2 * DT_B);                        // [64] |a|^2 (L2)
  uint8_t* At = reinterpret_cast<uint8_t*>(An + DT_A);                    // [nseg][64][GT_BSTRIDE], swizzled like B
  // PQ: MASK_BITMAP [2][64][SCAN_MROW] bitmap words of the 64 A rows, SCAN_MBLOCK columns per buffer; MASK_LABELS [2][64] labels of a B tile
  [[maybe_unused]] uint32_t* Mk = reinterpret_cast<uint32_t*>(At + nseg * GT_BT_BYTES);
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
  // PQ == MASK_BITMAP.  The words of a row arrive SCAN_MBLOCK = 512 columns at a time: thread (r0, c) asks for word c of the block of
  // rows r0 + 16 k (16 lanes: 64 contiguous bytes of one row), with the look-ahead loads of the block's first unit in this piece,
  // and stores them with that unit's tile.  Blocks are counted in ABSOLUTE columns (bt >> 9: a piece starts at a multiple of 64),
  // buffer = block & 1: the block of the tile in the epilogue and the block being stored are never the same.  Rows are clamped to
  // the tile's last row, words to the row's last word; the row offset is 64-bit.
  [[maybe_unused]] uint32_t mp0 = 0, mp1 = 0, mp2 = 0, mp3 = 0, plab = 0;      // bitmap words / (MASK_LABELS) the label of row bt + lane
  [[maybe_unused]] const uint32_t* mrow0 = nullptr; [[maybe_unused]] const uint32_t* mrow1 = nullptr;
  [[maybe_unused]] const uint32_t* mrow2 = nullptr; [[maybe_unused]] const uint32_t* mrow3 = nullptr;
  [[maybe_unused]] const uint32_t mwords = (uint32_t)((A.nb + 31) / 32);
  [[maybe_unused]] uint32_t pa[4] = {0, 0, 0, 0}, pb[4] = {0, 0, 0, 0};          // MASK_LABELS: the predicates of rows 4q + r
  if constexpr (PQ == MASK_BITMAP) {
    const uint32_t rl = na_tile - 1u;
    mrow0 = F.allow + (a0 + min((uint32_t)r0, rl)) * F.stride;
    mrow1 = F.allow + (a0 + min((uint32_t)r0 + 16u, rl)) * F.stride;
    mrow2 = F.allow + (a0 + min((uint32_t)r0 + 32u, rl)) * F.stride;
    mrow3 = F.allow + (a0 + min((uint32_t)r0 + 48u, rl)) * F.stride;
  }
  if constexpr (PQ == MASK_LABELS) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const pann_label_pred p = F.preds[a0 + min((uint32_t)(wave * DT_AW + q * 4 + r), na_tile - 1u)];
      pa[r] = p.a; pb[r] = p.b;
    }
  }
  auto unit_bt = [&](uint32_t u) -> uint32_t { return (uint32_t)bs + (nseg == 2 ? (u >> 1) : u) * DT_B; };
  [[maybe_unused]] uint32_t nid0 = 0, nid1 = 0, nid2 = 0, nid3 = 0, pid = 0;      // LIST: the row ids load_pre turns into addresses; the id of Bm
  [[maybe_unused]] auto load_ids = [&](uint32_t u) {      // LIST: requested one step before the rows they address; clamped positions
    const uint32_t bt = unit_bt(u);
    nid0 = A.b_ids[min(bt + (uint32_t)r0, last_row)];
    nid1 = A.b_ids[min(bt + (uint32_t)r0 + 16u, last_row)];
    nid2 = A.b_ids[min(bt + (uint32_t)r0 + 32u, last_row)];
    nid3 = A.b_ids[min(bt + (uint32_t)r0 + 48u, last_row)];
  };
  [[maybe_unused]] auto mask_unit = [&](uint32_t u) -> bool {      // the first unit of a bitmap block in this piece (wave-uniform)
    return (nseg == 2 ? (u & 1u) == 0u : true) && (u < nseg || (unit_bt(u) & (SCAN_MBLOCK - 1u)) == 0u);
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
    if constexpr (PQ == MASK_BITMAP) {
      if (mask_unit(u)) {
        const uint32_t w = min((bt >> 9) * 16u + (uint32_t)c, mwords - 1u);
        mp0 = mrow0[w]; mp1 = mrow1[w]; mp2 = mrow2[w]; mp3 = mrow3[w];
      }
    }
    if constexpr (PQ == MASK_LABELS) plab = F.labels[min(bt + (uint32_t)lane, last_row)];
  };
  auto store_pre = [&](uint32_t u) {
    const int buf = (int)(u & 1);
    gt_store_tile(Bt0 + buf * GT_BT_BYTES, Bm + buf * DT_B, (nseg == 2 && (u & 1)) ? cv1 : cv0, pre0, pre1, pre2, pre3, __int_as_float(pn),
                  unit_bt(u), be, tid);
    // LIST: a row is labelled with its id, not its position (a position at or beyond `be` stays SENTINEL)
    if constexpr (LIST) { if (tid < DT_B && (uint64_t)unit_bt(u) + tid < be) Bm[buf * DT_B + tid].y = __uint_as_float(pid); }
    if constexpr (PQ == MASK_BITMAP) {
      if (mask_unit(u)) {
        uint32_t* dst = Mk + ((unit_bt(u) >> 9) & 1u) * (DT_A * SCAN_MROW) + (uint32_t)r0 * SCAN_MROW + (uint32_t)c;
        dst[0] = mp0; dst[16 * SCAN_MROW] = mp1; dst[32 * SCAN_MROW] = mp2; dst[48 * SCAN_MROW] = mp3;
      }
    }
    if constexpr (PQ == MASK_LABELS) { if (tid < DT_B) Mk[buf * DT_B + tid] = plab; }
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
      // PQ: a cell its row's filter does not allow becomes a quiet NaN -- every test gt_select makes on a distance is dist <= tau,
      // so the cell is never pending and never inserted.  Once per tile: here, in the last segment's epilogue.
      if constexpr (PQ == MASK_BITMAP) {
        const uint32_t bt = unit_bt(u);      // the tile's 64 bits of row 4q + r: two words, read by the 16 lanes of a quarter as a broadcast
        const uint32_t* mq = Mk + ((bt >> 9) & 1u) * (DT_A * SCAN_MROW) + (uint32_t)(wave * DT_AW + q * 4) * SCAN_MROW + ((bt >> 5) & 15u);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const uint2 w = *reinterpret_cast<const uint2*>(mq + r * SCAN_MROW);
          const uint32_t lo = w.x >> (lane & 15), hi = w.y >> (lane & 15);      // column t * 16 + (lane & 15): bit (t & 1) * 16 of word t >> 1
          dist[r][0] = (lo & 1u) ? dist[r][0] : __builtin_nanf("");
          dist[r][1] = (lo & 0x10000u) ? dist[r][1] : __builtin_nanf("");
          dist[r][2] = (hi & 1u) ? dist[r][2] : __builtin_nanf("");
          dist[r][3] = (hi & 0x10000u) ? dist[r][3] : __builtin_nanf("");
        }
      }
      if constexpr (PQ == MASK_LABELS) {
        uint32_t lab[4];
#pragma unroll
        for (int t = 0; t < 4; t++) lab[t] = Mk[buf * DT_B + t * 16 + (lane & 15)];
        const uint32_t kind = (uint32_t)F.kind;      // uniform: one branch per tile, not one per cell
        if (kind == PANN_PRED_ANY) {
#pragma unroll
          for (int r = 0; r < 4; r++)
#pragma unroll
            for (int t = 0; t < 4; t++) dist[r][t] = (lab[t] & pa[r]) != 0u ? dist[r][t] : __builtin_nanf("");
        } else if (kind == PANN_PRED_MATCH) {
#pragma unroll
          for (int r = 0; r < 4; r++)
#pragma unroll
            for (int t = 0; t < 4; t++) dist[r][t] = (lab[t] & pa[r]) == pb[r] ? dist[r][t] : __builtin_nanf("");
        } else {
#pragma unroll
          for (int r = 0; r < 4; r++)
#pragma unroll
            for (int t = 0; t < 4; t++) dist[r][t] = (lab[t] >= pa[r] && lab[t] <= pb[r]) ? dist[r][t] : __builtin_nanf("");
        }
      }
      gt_select<NR>(S, dist, bid, skip, pplace, gtau_mine, A.nsplit, lane);
    }
    lds_barrier();
  }
  gt_sel_write<NR>(S, A.partial + ((a0 + wave * DT_AW + q * 4) * A.nsplit + blockIdx.y) * A.m, A.m, A.nsplit, lane);
