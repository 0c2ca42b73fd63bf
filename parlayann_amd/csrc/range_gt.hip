// range_gt.hip -- dense radius join on gfx950: every (query, point) pair with distance <= radius, as CSR.
//
//   compute_range_groundtruth  data_tools/compute_range_groundtruth.cpp:13-29  all base points with dist <= r per query
//
// Tiling is the one of dense.hip: a 256-thread workgroup owns 64 query rows (16 per wave) and streams one PIECE of the
// base (blockIdx.y of nsplit contiguous ranges) through LDS in tiles of 64 rows (matrix cores) or 128 rows (VALU), staged
// in 256-byte segments of the dimension.  What differs is the epilogue: no top-k lists, no tile barrier for them -- a
// distance is compared with the radius, one __ballot per (query row, tile column group) and a popcount give the number of
// matches and, in ascending id order, the place of every match.
//
// Output order without atomics and without a sort: the SAME kernel runs twice (template flag FILL).
//   pass 1  counts[query][piece] = matches of the query in the piece
//   scan    pos = exclusive prefix sum of counts in (query, piece) order, 64-bit
//   pass 2  recomputes the tiles (the same instructions, so the same bits) and writes the ids of (query, piece) from
//           pos[query][piece] on: a wave owns its 16 query rows for the whole piece, so its running positions are private.
// Pieces are ascending ranges of the base and a tile is walked in ascending id order, so the ids of a query come out
// ascending, each once, whatever nsplit is.  A write is additionally refused at or beyond the total.
//
// Arithmetic per element type (default mode):
//   f16 / bf16  v_mfma_f32_16x16x32_{f16,bf16} dot products, L2 as |a|^2 + |b|^2 - 2 a.b clamped at 0 (the norm form of
//               dense_topk_mfma_f16_kernel), MIPS as -a.b
//   u8 / i8     v_dot4 dot products in int32 (exact), L2 as |a|^2 + |b|^2 - 2 a.b with the row norms summed while the
//               tiles are staged (exact), one cast to float at the end like dist_finish
//   f32         dist_accum: fma register tile, sum (a-b)^2 (difference form)
// Exact float order (all three float types): dist_accum_exact, one sequential f32 sum per pair, strictly left to right.
#include <algorithm>

#include "dense_tile.h"

namespace pann {

// (DT_A = 64 query rows per workgroup, DT_AW = 16 per wave, DT_SEG, DT_BSTRIDE, DT_B = 64 base rows per matrix-core tile: dense_tile.h)
constexpr int RJ_VB = 128;        // VALU kernel: base rows per tile (two per lane)
constexpr uint64_t RJ_PIECE_ALIGN = 128;    // a piece is a whole number of tiles of either kernel

struct RangeJoinArgs {
  const uint8_t* points; uint32_t pstride; uint32_t dbytes;
  const uint8_t* q; uint64_t q_stride;      // external query rows (device)
  uint64_t nq, n;
  uint32_t nsplit; uint64_t per;            // pieces of the base, rows per piece (a multiple of RJ_PIECE_ALIGN)
  float radius; uint32_t exact;
  uint32_t* counts;                         // [nq][nsplit]: written by the count pass
  const uint64_t* pos;                      // [nq * nsplit + 1]: exclusive scan of counts, read by the fill pass
  uint32_t* out_ids;
};

// ---- VALU tiles: one-byte types (dot4), f32 (fma), and every float type in exact-float-order mode ----
template <int DT, int METRIC, bool FILL>
__global__ void __launch_bounds__(256) range_join_valu_kernel(RangeJoinArgs A) {
  extern __shared__ __align__(16) uint8_t smem[];
  constexpr bool INTEGER = !is_float_dt<DT>();
  constexpr int ACC_METRIC = INTEGER ? PANN_MIPS : METRIC;      // one-byte types accumulate a.b only; L2 adds the norms
  constexpr bool EXACT_ONLY = DT == PANN_F16 || DT == PANN_BF16;   // two-byte types come here in exact-float-order mode only
  uint8_t* At = smem;                                           // [64][DT_SEG]
  uint8_t* Bt = At + DT_A * DT_SEG;                             // [128][DT_BSTRIDE]
  int* An = reinterpret_cast<int*>(Bt + RJ_VB * DT_BSTRIDE);    // [64]  |a|^2 (one-byte types, L2)
  int* Bn = An + DT_A;                                          // [128] |b|^2
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);    // uniform: the per-row counters and positions below stay scalar
  const TileGeom g = tile_geom(A.nq, A.n, A.per);
  const uint64_t a0 = g.a0, bs = g.bs, be = g.be; const uint32_t na_tile = g.na_tile;
  const uint32_t nseg = (A.pstride + DT_SEG - 1) / DT_SEG;
  const int r0 = tid >> 4, c = tid & 15;                        // staging: 16 threads x 16 B per row, 16 rows per sweep

  uint32_t cnt[DT_AW];                                          // matches of the wave's rows in this piece so far (both passes)
  uint64_t total = 0;                                           // no write lands at or beyond it, whatever happens
  if constexpr (FILL) total = A.pos[A.nq * A.nsplit];
#pragma unroll
  for (int a = 0; a < DT_AW; a++) cnt[a] = 0;

  auto stage_a = [&](uint32_t sg) {
#pragma unroll
    for (int k = 0; k < DT_A / 16; k++) {
      const int r = r0 + 16 * k;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (r < (int)na_tile) v = load16_unaligned(A.q + (a0 + r) * A.q_stride, sg * DT_SEG + c * 16, A.dbytes);
      *reinterpret_cast<uint4*>(At + (size_t)r * DT_SEG + c * 16) = v;
      if constexpr (INTEGER && METRIC == PANN_L2) {
        const int ss = group_sum<16>(sumsq16_i8<DT>(v));
        if (c == 0) An[r] = sg == 0 ? ss : An[r] + ss;
      }
    }
  };
  auto stage_b = [&](uint64_t bt, uint32_t nb_tile, uint32_t sg) {
#pragma unroll
    for (int k = 0; k < RJ_VB / 16; k++) {
      const int r = r0 + 16 * k;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (r < (int)nb_tile) v = load16_guarded(A.points + (bt + r) * A.pstride, sg * DT_SEG + c * 16, A.pstride);
      *reinterpret_cast<uint4*>(Bt + (size_t)r * DT_BSTRIDE + c * 16) = v;
      if constexpr (INTEGER && METRIC == PANN_L2) {
        const int ss = group_sum<16>(sumsq16_i8<DT>(v));
        if (c == 0) Bn[r] = sg == 0 ? ss : Bn[r] + ss;
      }
    }
  };

  if (nseg == 1) stage_a(0);                                    // the query tile is fixed: staged once

  for (uint64_t bt = bs; bt < be; bt += RJ_VB) {
    const uint32_t nb_tile = (uint32_t)min((uint64_t)RJ_VB, be - bt);
    Acc<DT> acc[DT_AW][2];
#pragma unroll
    for (int a = 0; a < DT_AW; a++) { acc[a][0].clear(); acc[a][1].clear(); }
    for (uint32_t sg = 0; sg < nseg; sg++) {
      __syncthreads();                                          // the previous step's readers are done with the tiles
      stage_b(bt, nb_tile, sg);
      if (nseg > 1) stage_a(sg);
      __syncthreads();
      // chunks that hold only the rows' zero padding add nothing: skip them
      const uint32_t seg_bytes = min((uint32_t)DT_SEG, A.pstride - sg * DT_SEG);
      const uint32_t seg_valid = A.dbytes > sg * DT_SEG ? min(seg_bytes, A.dbytes - sg * DT_SEG) : 0u;
      const uint32_t nchunk = (seg_valid + 15) / 16;
      for (uint32_t ch = 0; ch < nchunk; ch++) {
        const uint4 braw0 = *reinterpret_cast<const uint4*>(Bt + (size_t)lane * DT_BSTRIDE + ch * 16);
        const uint4 braw1 = *reinterpret_cast<const uint4*>(Bt + (size_t)(lane + 64) * DT_BSTRIDE + ch * 16);
        if constexpr (!INTEGER) {
          if (EXACT_ONLY || A.exact) {      // strictly left to right, unfused, one accumulator per pair (s.y stays 0)
#pragma unroll
            for (int a = 0; a < DT_AW; a++) {
              const uint4 q = *reinterpret_cast<const uint4*>(At + (size_t)(wave * DT_AW + a) * DT_SEG + ch * 16);
              float t0 = acc[a][0].s.x, t1 = acc[a][1].s.x;
              dist_accum_exact<DT, METRIC>(t0, q, braw0);
              dist_accum_exact<DT, METRIC>(t1, q, braw1);
              acc[a][0].s.x = t0; acc[a][1].s.x = t1;
              asm volatile("" ::: "memory");                    // one query row at a time: 16 widened rows in flight would spill
            }
            continue;
          }
        }
        if constexpr (!EXACT_ONLY) {
          const QReg<DT> b0 = make_qreg<DT>(braw0), b1 = make_qreg<DT>(braw1);
#pragma unroll
          for (int a = 0; a < DT_AW; a++) {
            const uint4 q = *reinterpret_cast<const uint4*>(At + (size_t)(wave * DT_AW + a) * DT_SEG + ch * 16);
            dist_accum<DT, ACC_METRIC>(acc[a][0], q, b0);
            dist_accum<DT, ACC_METRIC>(acc[a][1], q, b1);
          }
        }
      }
    }
    // ---- epilogue: compare with the radius; ballot order is id order ----
#pragma unroll
    for (int a = 0; a < DT_AW; a++) {
      const uint32_t ar = wave * DT_AW + a;
#pragma unroll
      for (int rb = 0; rb < 2; rb++) {
        const uint32_t brow = lane + 64 * rb;
        float dist;
        if constexpr (INTEGER) {
          const int dot = (int)acc[a][rb].aq;
          if constexpr (METRIC == PANN_L2) dist = (float)(An[ar] + Bn[brow] - 2 * dot);
          else dist = -(float)dot;
        } else {
          dist = dist_finish<DT, METRIC>(acc_lane_value<DT, METRIC>(acc[a][rb]));
        }
        const bool inside = (brow < nb_tile) && (ar < na_tile) && (dist <= A.radius);
        const uint64_t mask = __ballot(inside);
        if constexpr (FILL) {       // (the start of the row's range: a scalar load, a padding row reads the tile's last real one)
          const uint64_t start = A.pos[(a0 + min(ar, na_tile - 1)) * A.nsplit + blockIdx.y];
          const uint64_t p = start + cnt[a] + lanes_below(mask, lane);
          if (inside && p < total) A.out_ids[p] = (uint32_t)(bt + brow);
        }
        cnt[a] += __popcll(mask);
      }
    }
  }
  if constexpr (!FILL) {
#pragma unroll
    for (int a = 0; a < DT_AW; a++) {
      const uint32_t ar = wave * DT_AW + a;
      if (lane == 0 && ar < na_tile) A.counts[(a0 + ar) * A.nsplit + blockIdx.y] = cnt[a];
    }
  }
}

// ---- matrix-core tiles: f16 / bf16 in default mode ----
// Each wave owns 16 query rows and computes the 16 x 64 block of dot products against the tile with four MFMAs per 32
// elements of the dimension (fragments are plain ds_read_b128 from the padded LDS rows, as in dense_topk_mfma_f16_kernel);
// acc[t][r] = a(row wave*16 + 4*(lane>>4) + r) . b(column t*16 + (lane & 15)).  The base rows of step i+1 (a step = one
// 256-byte segment of one tile) are requested from HBM before step i is multiplied and written to LDS after it; the
// barriers order LDS only.  With single-segment rows (d <= 128) the query fragments stay in registers for the whole launch.
template <int METRIC, bool BF, bool FILL>
__global__ void __launch_bounds__(256) range_join_mfma_kernel(RangeJoinArgs A) {
  extern __shared__ __align__(16) uint8_t smem[];
  uint8_t* At = smem;                                           // [64][DT_BSTRIDE]
  uint8_t* Bt = At + DT_A * DT_BSTRIDE;                         // [64][DT_BSTRIDE]
  float* An = reinterpret_cast<float*>(Bt + DT_B * DT_BSTRIDE);   // [64] |a|^2
  float* Bn = An + DT_A;                                        // [64] |b|^2
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const TileGeom g = tile_geom(A.nq, A.n, A.per);
  const uint64_t a0 = g.a0, bs = g.bs, be = g.be; const uint32_t na_tile = g.na_tile;
  const uint32_t nseg = (A.pstride + DT_SEG - 1) / DT_SEG;
  const int r0 = tid >> 4, c = tid & 15;
  const int q = lane >> 4, col = lane & 15;

  uint32_t cnt[4];
  uint64_t wpos[4];
  uint64_t total = 0;                                           // no write lands at or beyond it, whatever happens
  if constexpr (FILL) total = A.pos[A.nq * A.nsplit];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    cnt[r] = 0; wpos[r] = 0;
    if constexpr (FILL) {
      const uint32_t ar = wave * DT_AW + q * 4 + r;
      if (ar < na_tile) wpos[r] = A.pos[(a0 + ar) * A.nsplit + blockIdx.y];
    }
  }
  if (bs >= be) {                                               // an empty piece (uniform): nothing to count, nothing to write
    if constexpr (!FILL) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t ar = wave * DT_AW + q * 4 + r;
        if (col == 0 && ar < na_tile) A.counts[(a0 + ar) * A.nsplit + blockIdx.y] = 0;
      }
    }
    return;
  }

  // query tile: segment sg to LDS; norms = true also leaves |a|^2 of the segments seen so far in An
  float anorm[4] = {0.f, 0.f, 0.f, 0.f};
  auto stage_a = [&](uint32_t sg, bool norms) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int r = r0 + 16 * k;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (r < (int)na_tile) v = load16_unaligned(A.q + (a0 + r) * A.q_stride, sg * DT_SEG + c * 16, A.dbytes);
      *reinterpret_cast<uint4*>(At + (size_t)r * DT_BSTRIDE + c * 16) = v;
      if (norms) {
        anorm[k] += group_sum<16>(sumsq16<BF>(v));
        if (c == 0) An[r] = anorm[k];
      }
    }
  };
  // |a|^2 over all segments; the last one staged stays in LDS (nseg == 1: the whole tile, for the whole launch)
  for (uint32_t sg = 0; sg < nseg; sg++) {
    if (sg > 0) __syncthreads();
    stage_a(sg, true);
  }

  // base rows one step ahead, in registers
  const uint64_t last = be - 1;
  uint4 pre[4];
  auto load_b = [&](uint64_t bt, uint32_t sg) {
    const uint32_t off = sg * DT_SEG + c * 16;
    const uint32_t offc = min(off, A.pstride - 16u);            // a chunk beyond the row re-reads its last one and is zeroed
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint64_t row = min(bt + (uint64_t)(r0 + 16 * k), last);     // a row beyond the piece re-reads its last one and is masked
      pre[k] = *reinterpret_cast<const uint4*>(A.points + row * A.pstride + offc);
    }
  };
  float bnorm[4] = {0.f, 0.f, 0.f, 0.f};
  auto store_b = [&](uint32_t sg) {
    const bool cvalid = sg * DT_SEG + c * 16 < A.pstride;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int r = r0 + 16 * k;
      const uint4 v = cvalid ? pre[k] : make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4*>(Bt + (size_t)r * DT_BSTRIDE + c * 16) = v;
      if constexpr (METRIC == PANN_L2) {
        const float ss = group_sum<16>(sumsq16<BF>(v));
        bnorm[k] = sg == 0 ? ss : bnorm[k] + ss;
        if (c == 0) Bn[r] = bnorm[k];
      }
    }
  };

  // single-segment rows: the wave's query fragments, read once
  uint4 afrag[4];
  if (nseg == 1) {
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ks++)
      afrag[ks] = *reinterpret_cast<const uint4*>(At + (size_t)(wave * DT_AW + col) * DT_BSTRIDE + ks * 64 + q * 16);
  }

  load_b(bs, 0);
  for (uint64_t bt = bs; bt < be; bt += DT_B) {
    const uint32_t nb_tile = (uint32_t)min((uint64_t)DT_B, be - bt);
    mf_float4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = mf_float4{0.f, 0.f, 0.f, 0.f};
    for (uint32_t sg = 0; sg < nseg; sg++) {
      lds_barrier();                                         // the previous step's multiply and epilogue have read the tiles
      store_b(sg);
      if (nseg > 1) stage_a(sg, false);
      {                                                         // next step: the next segment of this tile, or the next tile
        const bool wrap = sg + 1 == nseg;
        load_b(wrap ? bt + DT_B : bt, wrap ? 0u : sg + 1);
      }
      lds_barrier();
      const uint32_t ksteps = min((uint32_t)DT_SEG, A.pstride - sg * DT_SEG) / 64;      // 32 two-byte elements per MFMA
#pragma unroll
      for (uint32_t ks = 0; ks < 4; ks++) {                     // (unrolled: afrag stays in registers)
        if (ks >= ksteps) break;
        const uint32_t koff = ks * 64 + q * 16;
        uint4 araw;
        if (nseg == 1) araw = afrag[ks];
        else araw = *reinterpret_cast<const uint4*>(At + (size_t)(wave * DT_AW + col) * DT_BSTRIDE + koff);
#pragma unroll
        for (int t = 0; t < 4; t++)
          acc[t] = mfma_step<BF>(araw, *reinterpret_cast<const uint4*>(Bt + (size_t)(t * 16 + col) * DT_BSTRIDE + koff), acc[t]);
      }
    }
    // ---- epilogue: the ballot of (r, t) holds row 4 q' + r in its bits 16 q' .. 16 q' + 15, columns t*16 .. t*16 + 15 in order ----
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint32_t ar = wave * DT_AW + q * 4 + r;
      const float an = An[ar];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const uint32_t bc = t * 16 + col;
        float dist;
        if constexpr (METRIC == PANN_L2) dist = fmaxf(fmaf(-2.0f, acc[t][r], an + Bn[bc]), 0.f);   // (norm form: never below 0)
        else dist = -acc[t][r];
        const bool inside = (bc < nb_tile) && (ar < na_tile) && (dist <= A.radius);
        const uint64_t mask = __ballot(inside);
        const uint32_t slice = (uint32_t)(mask >> (16 * q)) & 0xFFFFu;
        if constexpr (FILL) {
          const uint64_t p = wpos[r] + __popc(slice & ((1u << col) - 1u));
          if (inside && p < total) A.out_ids[p] = (uint32_t)(bt + bc);
          wpos[r] += __popc(slice);
        } else {
          cnt[r] += __popc(slice);
        }
      }
    }
  }
  if constexpr (!FILL) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint32_t ar = wave * DT_AW + q * 4 + r;
      if (col == 0 && ar < na_tile) A.counts[(a0 + ar) * A.nsplit + blockIdx.y] = cnt[r];
    }
  }
}

// ---- exclusive 64-bit prefix sum of m 32-bit counts (one workgroup: m = queries x pieces is small), pos[m] = total ----
__device__ __forceinline__ uint64_t rj_shfl_up64(uint64_t v, int delta) {
  const uint32_t lo = __shfl_up((uint32_t)v, delta), hi = __shfl_up((uint32_t)(v >> 32), delta);
  return ((uint64_t)hi << 32) | lo;
}
__global__ void __launch_bounds__(1024) range_join_scan_kernel(const uint32_t* __restrict__ cnt, uint64_t m, uint64_t* __restrict__ pos) {
  __shared__ uint64_t wtot[16];
  constexpr int PER = 8;                                        // consecutive counts per thread
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t carry = 0;
  for (uint64_t base = 0; base < m; base += 1024 * PER) {
    const uint64_t i0 = base + (uint64_t)tid * PER;
    uint32_t v[PER];
    uint64_t s = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) { v[j] = i0 + j < m ? cnt[i0 + j] : 0u; s += v[j]; }
    uint64_t inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint64_t t = rj_shfl_up64(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint64_t woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) { const uint64_t x = wtot[w]; woff += w < wave ? x : 0ull; tot += x; }
    uint64_t p = carry + woff + inc - s;
#pragma unroll
    for (int j = 0; j < PER; j++) { if (i0 + j < m) pos[i0 + j] = p; p += v[j]; }
    carry += tot;
    __syncthreads();
  }
  if (tid == 0) pos[m] = carry;
}

// offsets[q] = pos[q * nsplit] for q in 0 .. nq (offsets[nq] = the total)
__global__ void __launch_bounds__(256) range_join_offsets_kernel(const uint64_t* __restrict__ pos, uint64_t nq, uint32_t nsplit, uint64_t* __restrict__ offsets) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i <= nq) offsets[i] = pos[i * nsplit];
}

template <bool FILL>
static int range_join_launch(const DeviceIndex& ix, hipStream_t st, const RangeJoinArgs& A, dim3 grid) {
  dispatch_type_metric(ix.dtype, ix.metric, [&](auto dt, auto mt) {
    constexpr int DT = decltype(dt)::value, MT = decltype(mt)::value;
    if constexpr (is_two_byte(DT)) {
      if (!ix.exact)
        return launch_lds(range_join_mfma_kernel<MT, DT == PANN_BF16, FILL>, grid, dim3(256),
                          (size_t)(DT_A + DT_B) * DT_BSTRIDE + (DT_A + DT_B) * sizeof(float), st, A);
    }
    launch_lds(range_join_valu_kernel<DT, MT, FILL>, grid, dim3(256),
               (size_t)DT_A * DT_SEG + (size_t)RJ_VB * DT_BSTRIDE + (DT_A + RJ_VB) * sizeof(int), st, A);
  });
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

// The arguments of both passes, with the two arrays of `ws`: a count per (query, piece) and their scan.  The count call grows ws
// here; the fill call, with the same arguments, finds it large enough, so the buffer stays where it was.
static int range_join_args(const DeviceIndex& ix, Workspace& ws, const uint8_t* d_q, uint64_t q_stride, uint64_t nq,
                           float radius, uint32_t nsplit, RangeJoinArgs& A) {
  A = RangeJoinArgs{};
  A.points = ix.points; A.pstride = ix.pstride; A.dbytes = ix.dbytes;
  A.q = d_q; A.q_stride = q_stride; A.nq = nq; A.n = ix.n;
  A.nsplit = nsplit;
  A.per = ((ix.n + nsplit - 1) / nsplit + RJ_PIECE_ALIGN - 1) / RJ_PIECE_ALIGN * RJ_PIECE_ALIGN;
  A.radius = radius; A.exact = ix.exact;
  const size_t slots = (size_t)nq * nsplit;
  return carve_into(ws, 0, [&](Carve& c) { A.counts = c.take<uint32_t>(slots); A.pos = c.take<uint64_t>(slots + 1); });
}

// pieces of the base per query tile: enough workgroups to fill the 256 CUs several times over (a workgroup keeps no state
// between tiles, so small pieces cost nothing but their share of the scan), never less than one tile per piece
uint32_t range_join_pieces(const DeviceIndex& ix, uint64_t nq, uint32_t wanted) {
  const uint64_t ntiles = (nq + DT_A - 1) / DT_A;
  uint64_t p = wanted ? wanted : (2048 + ntiles - 1) / ntiles;
  p = std::min<uint64_t>(p, (ix.n + 255) / 256);
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(p, 64));
}

// pass 1 + scan: d_offsets (device, nq + 1 entries) = the CSR offsets.  The workspace keeps what the fill pass needs:
// nothing else may use `ws` between the two calls.
int range_join_count_dev(const DeviceIndex& ix, Workspace& ws, hipStream_t st, const uint8_t* d_q, uint64_t q_stride, uint64_t nq,
                         float radius, uint32_t nsplit, uint64_t* d_offsets) {
  if (nq == 0) return PANN_OK;
  const size_t slots = (size_t)nq * nsplit;
  RangeJoinArgs A;
  if (int rc = range_join_args(ix, ws, d_q, q_stride, nq, radius, nsplit, A)) return rc;
  const dim3 grid((uint32_t)((nq + DT_A - 1) / DT_A), nsplit);
  if (int rc = range_join_launch<false>(ix, st, A, grid)) return rc;
  hipLaunchKernelGGL(range_join_scan_kernel, dim3(1), dim3(1024), 0, st, A.counts, (uint64_t)slots, const_cast<uint64_t*>(A.pos));
  PANN_HIP(hipGetLastError());
  hipLaunchKernelGGL(range_join_offsets_kernel, dim3((uint32_t)((nq + 1 + 255) / 256)), dim3(256), 0, st, A.pos, nq, nsplit, d_offsets);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

// pass 2: d_out_ids holds at least offsets[nq] entries; same arguments as the count call before it
int range_join_fill_dev(const DeviceIndex& ix, Workspace& ws, hipStream_t st, const uint8_t* d_q, uint64_t q_stride, uint64_t nq,
                        float radius, uint32_t nsplit, uint32_t* d_out_ids) {
  if (nq == 0) return PANN_OK;
  RangeJoinArgs A;
  if (int rc = range_join_args(ix, ws, d_q, q_stride, nq, radius, nsplit, A)) return rc;
  A.out_ids = d_out_ids;
  const dim3 grid((uint32_t)((nq + DT_A - 1) / DT_A), nsplit);
  return range_join_launch<true>(ix, st, A, grid);
}

}  // namespace pann
