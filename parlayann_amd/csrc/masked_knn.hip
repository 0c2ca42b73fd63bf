// masked_knn.hip -- exact kNN under an allow bitmap (DESIGN.md "Exact masked kNN"): what a caller falls back to when a mask is
// so selective that the masked beam search sees too few allowed points.  Two routes, both on the bitmap format of
// pann_batch_search_masked (ceil(n / 32) words per row, bits at positions >= n ignored):
//
//   shared bitmap      allow_block_count_kernel   popcount of every block of 256 words
//                      allow_block_scan_kernel    exclusive scan over the blocks (one workgroup), total = allowed points
//                      allow_scatter_kernel       every word's set bits to their ranks: the ascending list of allowed ids
//                      the list then is the b_ids of dense_topk_dev (dense.hip), the queries its external A rows.
//   per-query bitmaps  masked_scan_kernel         one wave per query walks its row 64 words (2 048 positions) at a time, ranks
//                                                 the set bits, scores the allowed ids with gather_tile -- the arithmetic of
//                                                 query_distances_kernel, exact-float-order mode included -- and keeps the best
//                                                 k <= 64 keys as one sorted (dist, id) key per lane.
//
// allow_count_kernel (pann_allow_count_dev) is the count half alone, per row.
//
// Grouped route (DESIGN.md "Exact kNN by predicate group"): a table of G filters and one table index per query.
//   group_hist_kernel / group_colscan_kernel / group_place_kernel   stable counting sort of the queries by table index: the
//                                                 queries of a table entry one after the other, ascending inside an entry
//   the compaction kernels above with rows on grid.y      the ascending id list of every used entry of a chunk, one after the
//                                                 other (CSR): the b_ids / b_off of ONE segmented dense_topk_dev launch
//   gather_query_rows_kernel / scatter_knn_rows_kernel    the queries into a slab in group order (its external A rows), the
//                                                 result rows back into the caller's order
//
// Label predicates (DESIGN.md "Label predicates"): one uint32 label per point and a two-word predicate per query stand for the
// bitmap row { i : pred(label[i]) }.
//   labels_to_allow_kernel   materialises such rows in the bitmap format (the bridge to everything above)
//   label_count_kernel       counts them without materialising anything
//   masked_scan_kernel<.., LABELS = true>   the per-query scan with its 64 words per step built from 2 048 labels
#include "dense_tile.h"

namespace pann {
namespace {

constexpr uint32_t MK_BLOCK = 256;                 // words (= threads) of one compaction block: 8 192 positions
constexpr uint32_t MK_CHUNK = PANN_WAVE * 32;      // positions one step of the per-query scan covers

// word w of a bitmap row of `words` words over n points: bits at positions >= n cleared, 0 past the row
__device__ __forceinline__ uint32_t allow_word(const uint32_t* __restrict__ row, uint64_t w, uint64_t words, uint64_t n) {
  if (w >= words) return 0u;
  uint32_t v = row[w];
  if (w == words - 1 && (n & 31)) v &= (1u << (n & 31)) - 1u;
  return v;
}

// exclusive prefix sum over the lanes of the wave; *total: the sum of all 64
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, int lane, uint32_t* total) {
  uint32_t s = v;
#pragma unroll
  for (int o = 1; o < PANN_WAVE; o <<= 1) {
    const uint32_t t = __shfl_up(s, o);
    if (lane >= o) s += t;
  }
  *total = __shfl(s, PANN_WAVE - 1);
  return s - v;
}

// the thread's exclusive rank among the 256 threads of its block, *total: the block's sum (every thread must call)
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
  const int lane = threadIdx.x & (PANN_WAVE - 1), wave = threadIdx.x / PANN_WAVE;
  uint32_t wt;
  const uint32_t excl = wave_excl_scan(v, lane, &wt);
  __syncthreads();                                 // the previous use of wsum has been read
  if (lane == 0) wsum[wave] = wt;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < (int)(MK_BLOCK / PANN_WAVE); w++) { before += w < wave ? wsum[w] : 0u; all += wsum[w]; }
  *total = all;
  return before + excl;
}

// counts[row] += allowed points of row (counts zeroed by the caller); grid.x: blocks per row, grid.y strides over the rows
__global__ void __launch_bounds__(MK_BLOCK) allow_count_kernel(const uint32_t* __restrict__ allow, uint64_t n, uint64_t rows,
                                                               uint64_t stride, uint32_t* __restrict__ counts) {
  const uint64_t words = (n + 31) / 32;
  for (uint64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const uint32_t* row = allow + r * stride;
    uint32_t c = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x; w < words; w += (uint64_t)gridDim.x * MK_BLOCK)
      c += __popc(allow_word(row, w, words, n));
#pragma unroll
    for (int o = PANN_WAVE / 2; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & (PANN_WAVE - 1)) == 0 && c) atomicAdd(&counts[r], c);
  }
}

// Row r (blockIdx.y, striding over `rows`) is row rowidx[r] (null: r) of `allow`, rows `stride` words apart; its block b writes
// block_counts[r * gridDim.x + b].  One bitmap: rows = 1, rowidx = null.
__device__ __forceinline__ const uint32_t* compact_row(const uint32_t* __restrict__ allow, const uint32_t* __restrict__ rowidx,
                                                       uint64_t stride, uint32_t r) {
  return allow + (uint64_t)(rowidx ? rowidx[r] : r) * stride;
}
__global__ void __launch_bounds__(MK_BLOCK) allow_block_count_kernel(const uint32_t* __restrict__ allow, uint64_t n,
                                                                     const uint32_t* __restrict__ rowidx, uint64_t stride, uint32_t rows,
                                                                     uint32_t* __restrict__ block_counts) {
  __shared__ uint32_t wsum[MK_BLOCK / PANN_WAVE];
  const uint64_t words = (n + 31) / 32;
  for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y) {
    uint32_t total;
    (void)block_excl_scan(__popc(allow_word(compact_row(allow, rowidx, stride, r), (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x, words, n)),
                          wsum, &total);
    if (threadIdx.x == 0) block_counts[(uint64_t)r * gridDim.x + blockIdx.x] = total;
  }
}

// block_counts[0 .. nblk) -> their exclusive prefix sums, in place; block_counts[nblk] = the total.  One workgroup.
__global__ void __launch_bounds__(MK_BLOCK) allow_block_scan_kernel(uint32_t* __restrict__ block_counts, uint32_t nblk) {
  __shared__ uint32_t wsum[MK_BLOCK / PANN_WAVE];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nblk; base += MK_BLOCK) {
    const uint32_t i = base + threadIdx.x;
    uint32_t total;
    const uint32_t excl = block_excl_scan(i < nblk ? block_counts[i] : 0u, wsum, &total);
    if (i < nblk) block_counts[i] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) block_counts[nblk] = carry;
}

// ids[rank of bit] = position of the bit, for every set bit below n: ascending.  cap: entries of ids (the total of the scan).
// Rows as allow_block_count_kernel: block_off is the scan over all rows' blocks, so the lists lie one after the other.
__global__ void __launch_bounds__(MK_BLOCK) allow_scatter_kernel(const uint32_t* __restrict__ allow, uint64_t n,
                                                                 const uint32_t* __restrict__ rowidx, uint64_t stride, uint32_t rows,
                                                                 const uint32_t* __restrict__ block_off, uint32_t* __restrict__ ids,
                                                                 uint32_t cap) {
  __shared__ uint32_t wsum[MK_BLOCK / PANN_WAVE];
  const uint64_t words = (n + 31) / 32;
  const uint64_t w = (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
  for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y) {
    uint32_t v = allow_word(compact_row(allow, rowidx, stride, r), w, words, n);
    uint32_t total;
    uint32_t pos = block_off[(uint64_t)r * gridDim.x + blockIdx.x] + block_excl_scan(__popc(v), wsum, &total);
    const uint32_t first = (uint32_t)(w * 32);
    while (v) {
      const uint32_t j = __ffs(v) - 1;
      v &= v - 1;
      if (pos < cap) ids[pos] = first + j;
      pos++;
    }
  }
}

// rows of an answer that no kernel computed: pad != 0 fills ids / dists with 0xFFFFFFFF / +inf; counts (optional) = cnt
__global__ void __launch_bounds__(MK_BLOCK) knn_pad_kernel(uint32_t* __restrict__ ids, float* __restrict__ dists,
                                                           uint32_t* __restrict__ counts, uint64_t nq, uint32_t k, uint32_t cnt, int pad) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x, i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pad) for (uint64_t i = i0; i < nq * k; i += step) { ids[i] = SENTINEL; dists[i] = __builtin_inff(); }
  if (counts) for (uint64_t i = i0; i < nq; i += step) counts[i] = cnt;
}

// ---- label predicates ----
constexpr uint32_t LA_WAVE_LABELS = PANN_WAVE * PANN_WAVE;               // labels one wave turns into 128 words: 64 ballots
constexpr uint32_t LA_BLOCK_LABELS = LA_WAVE_LABELS * (MK_BLOCK / PANN_WAVE);
constexpr uint32_t LC_TILE = 4096;                                       // labels of one tile of label_count_kernel (16 KB of LDS)

__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the verdicts of 64 consecutive labels from `first` on (lane i: label first + i), as a ballot; positions >= n: 0
__device__ __forceinline__ uint64_t label_ballot(const uint32_t* __restrict__ labels, uint64_t first, uint64_t n, uint32_t kind,
                                                 uint32_t pa, uint32_t pb, int lane) {
  const uint64_t i = first + (uint64_t)lane;
  const bool in = i < n;
  const uint32_t l = in ? labels[i] : 0u;
  return __ballot(in && label_pred(kind, pa, pb, l));
}

// Row r = blockIdx.y (+ gridDim.y ...) of `allow` <- the bitmap of preds[r].  A wave covers 4 096 labels: 64 coalesced loads of 64
// labels and one ballot each; lane j keeps ballot j and writes it as the two whole words 2j, 2j + 1 of the wave's 128.  Bits at
// positions >= n are 0 (label_ballot), words at or past ceil(n / 32) are not written.
__global__ void __launch_bounds__(MK_BLOCK) labels_to_allow_kernel(const uint32_t* __restrict__ labels, uint64_t n, uint32_t kind,
                                                                   const pann_label_pred* __restrict__ preds, uint64_t npreds,
                                                                   uint32_t* __restrict__ allow, uint64_t stride) {
  const int lane = threadIdx.x & (PANN_WAVE - 1), wave = threadIdx.x / PANN_WAVE;
  const uint64_t words = (n + 31) / 32;
  const uint64_t base = (uint64_t)blockIdx.x * LA_BLOCK_LABELS + (uint64_t)wave * LA_WAVE_LABELS;   // first label of the wave
  if (base >= n) return;
  for (uint64_t r = blockIdx.y; r < npreds; r += gridDim.y) {
    const uint32_t pa = uniform_u32(preds[r].a), pb = uniform_u32(preds[r].b);
    uint64_t mine = 0ull;
#pragma unroll 8
    for (int j = 0; j < PANN_WAVE; j++) {
      const uint64_t bal = label_ballot(labels, base + (uint64_t)j * PANN_WAVE, n, kind, pa, pb, lane);
      if (lane == j) mine = bal;
    }
    const uint64_t w = base / 32 + 2u * (uint32_t)lane;
    uint32_t* row = allow + r * stride;
    if (w < words) row[w] = (uint32_t)mine;
    if (w + 1 < words) row[w + 1] = (uint32_t)(mine >> 32);
  }
}

// counts[p] += points of the tile that preds[p] allows (counts zeroed by the caller).  blockIdx.x: the tile of LC_TILE labels,
// staged in LDS once; blockIdx.y: a group of 256 predicates, one per thread, which reads the tile by broadcast (every lane the
// same address) and keeps its count in a register: one atomic per thread and tile.
__global__ void __launch_bounds__(MK_BLOCK) label_count_kernel(const uint32_t* __restrict__ labels, uint64_t n, uint32_t kind,
                                                               const pann_label_pred* __restrict__ preds, uint64_t npreds,
                                                               uint32_t* __restrict__ counts) {
  __shared__ uint32_t T[LC_TILE];
  const uint64_t first = (uint64_t)blockIdx.x * LC_TILE;
  const uint32_t m = (uint32_t)min((uint64_t)LC_TILE, n - first);        // the launch has no tile at or past n
  for (uint32_t i = threadIdx.x; i < m; i += MK_BLOCK) T[i] = labels[first + i];
  __syncthreads();
  for (uint64_t p = (uint64_t)blockIdx.y * MK_BLOCK + threadIdx.x; p < npreds; p += (uint64_t)gridDim.y * MK_BLOCK) {
    const uint32_t pa = preds[p].a, pb = preds[p].b;
    uint32_t c = 0;
    for (uint32_t i = 0; i < m; i++) c += label_pred(kind, pa, pb, T[i]) ? 1u : 0u;
    if (c) atomicAdd(&counts[p], c);
  }
}

struct MaskedScanArgs {
  PointsView pv; uint32_t dbytes;
  const uint8_t* q; uint64_t q_stride;
  const uint32_t* allow; uint64_t allow_stride; uint64_t n;
  const uint32_t* labels; const pann_label_pred* preds; uint32_t kind;   // LABELS form: the words come from these instead of `allow`
  uint32_t k;                                      // <= 64
  uint32_t* out_ids; float* out_dists; uint32_t* out_counts;
};

// Where the scan's words come from: word w0 + lane of the query's bitmap row (allow_word), or -- LABELS -- the same word built from
// the 32 labels it stands for.  The step's 2 048 labels are read as 32 coalesced loads of 64 with one ballot each: ballot j holds
// the step's words 2j and 2j + 1, which lanes 2j and 2j + 1 keep.  Positions >= n are cleared either way.
struct ScanSrc { const uint32_t* row; uint32_t kind, pa, pb; };
template <bool LABELS>
__device__ __forceinline__ uint32_t scan_word(const ScanSrc& S, uint64_t w0, int lane, uint64_t words, uint64_t n) {
  if constexpr (!LABELS) return allow_word(S.row, w0 + lane, words, n);
  else {
    uint32_t v = 0u;
    if (w0 >= words) return v;                      // wave-uniform: the prefetch past the last step
#pragma unroll 8
    for (int j = 0; j < PANN_WAVE / 2; j++) {
      const uint64_t bal = label_ballot(S.row, (w0 + 2u * (uint32_t)j) * 32, n, S.kind, S.pa, S.pb, lane);
      if ((lane >> 1) == j) v = (lane & 1) ? (uint32_t)(bal >> 32) : (uint32_t)bal;
    }
    return v;
  }
}

template <int DT, int METRIC, int LPC, bool NCH1, bool LABELS>
__global__ void __launch_bounds__(PANN_WAVE) masked_scan_kernel(MaskedScanArgs P) {
  const int lane = threadIdx.x;
  __shared__ uint32_t Lst[MK_CHUNK + PANN_WAVE];   // allowed ids waiting for their distance: < 64 left over + one step's
  __shared__ uint64_t K[PANN_WAVE];                // keys of the tile just scored
  extern __shared__ __align__(16) uint8_t smem[];
  uint4* qlds = reinterpret_cast<uint4*>(smem);
  const uint64_t qi = blockIdx.x;
  QReg<DT> qreg{};
  load_query<DT, LPC, NCH1>(P.q + qi * P.q_stride, P.dbytes, P.pv.nch, qreg, qlds, lane);
  __syncthreads();
  ScanSrc S{P.allow + qi * P.allow_stride, 0u, 0u, 0u};
  if constexpr (LABELS) S = ScanSrc{P.labels, P.kind, uniform_u32(P.preds[qi].a), uniform_u32(P.preds[qi].b)};
  const uint64_t words = (P.n + 31) / 32;
  uint64_t best = KEY_INF;                         // lane i: the i-th smallest key seen so far
  uint64_t tau = KEY_INF;                          // the k-th smallest: what a candidate has to beat
  uint32_t fill = 0, total = 0;
  uint32_t wnext = scan_word<LABELS>(S, 0, lane, words, P.n);
  for (uint64_t w0 = 0; w0 < words; w0 += PANN_WAVE) {
    uint32_t v = wnext;
    wnext = scan_word<LABELS>(S, w0 + PANN_WAVE, lane, words, P.n);   // bitmap: in flight while this step is scored
    const bool last = w0 + PANN_WAVE >= words;
    uint32_t step_total;
    uint32_t pos = fill + wave_excl_scan(__popc(v), lane, &step_total);
    if (step_total == 0 && !last) continue;        // wave-uniform
    const uint32_t first = (uint32_t)((w0 + lane) * 32);
    while (v) {
      const uint32_t j = __ffs(v) - 1;
      v &= v - 1;
      Lst[pos++] = first + j;
    }
    fill += step_total; total += step_total;
    wave_lds_sync();
    // whole tiles of 64 now; what is left waits for the next step, and the last step scores it as a partial tile
    uint32_t t0 = 0;
    while (t0 + PANN_WAVE <= fill || (last && t0 < fill)) {
      const uint32_t mm = min(fill - t0, (uint32_t)PANN_WAVE);
      gather_tile<DT, METRIC, LPC, NCH1, 4>(P.pv, qreg, qlds, Lst + t0, mm, lane,
        [&](bool has, uint32_t ci, uint32_t id, float dist) { if (has) K[ci] = make_key(dist, id); });
      wave_lds_sync();
      const uint64_t key = lane < (int)mm ? K[lane] : KEY_INF;
      wave_lds_sync();                             // K is free for the next tile
      uint64_t mask = __ballot(key < tau);
      while (mask) {
        const int src = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        const uint64_t x = readlane64(key, src);
        if (x < tau) {                             // sorted insert, one key per lane; ids are unique, so no key repeats
          const uint64_t prev = __shfl_up(best, 1);
          best = best < x ? best : ((lane == 0 || prev < x) ? x : prev);
          tau = readlane64(best, (int)P.k - 1);
        }
      }
      t0 += mm;
    }
    const uint32_t rem = fill - t0;                // < 64
    if (t0 && rem) {
      const uint32_t keep = lane < (int)rem ? Lst[t0 + lane] : 0u;
      wave_lds_sync();
      if (lane < (int)rem) Lst[lane] = keep;
      wave_lds_sync();
    }
    fill = rem;
  }
  const uint32_t cnt = min(total, P.k);
  if (lane < (int)P.k) {
    const bool ok = lane < (int)cnt;
    P.out_ids[qi * P.k + lane] = ok ? key_id(best) : SENTINEL;
    P.out_dists[qi * P.k + lane] = ok ? key_dist(best) : __builtin_inff();
  }
  if (lane == 0 && P.out_counts) P.out_counts[qi] = cnt;
}

inline uint32_t compaction_blocks(uint64_t n) { return (uint32_t)(((n + 31) / 32 + MK_BLOCK - 1) / MK_BLOCK); }

// ---- grouped route: the queries sorted by table index, stably ----
// A counting sort in three kernels.  Workgroup b owns the queries [b * per_block, (b + 1) * per_block), per_block a multiple of
// GQ_TILE, and row b of `part` (G words, zeroed by the caller):
//   group_hist_kernel     part[b][g] = queries of entry g in b's range; an index >= G raises *flag and is left out
//   group_colscan_kernel  part[b][g] <- the queries of g in the ranges before b; hist[g] = off[g] = all of them
//   (allow_block_scan_kernel turns off[0 .. G] into the first slot of every entry)
//   group_place_kernel    b walks its range a tile at a time: a query's slot is off[g] + part[b][g] + the queries of g before it
//                         in the tile; the last query of g in the tile adds the tile's share to part[b][g] for the next tile
constexpr uint32_t GQ_TILE = MK_BLOCK;

__global__ void __launch_bounds__(MK_BLOCK) group_hist_kernel(const uint32_t* __restrict__ group, uint64_t nq, uint64_t G,
                                                              uint64_t per_block, uint32_t* __restrict__ part, uint32_t* __restrict__ flag) {
  const uint64_t lo = (uint64_t)blockIdx.x * per_block, hi = min(nq, lo + per_block);
  uint32_t* row = part + (uint64_t)blockIdx.x * G;
  for (uint64_t q = lo + threadIdx.x; q < hi; q += MK_BLOCK) {
    const uint32_t g = group[q];
    if (g >= G) atomicOr(flag, 1u);
    else atomicAdd(&row[g], 1u);
  }
}

__global__ void __launch_bounds__(MK_BLOCK) group_colscan_kernel(uint32_t* __restrict__ part, uint64_t G, uint32_t nblocks,
                                                                 uint32_t* __restrict__ hist, uint32_t* __restrict__ off) {
  const uint64_t g = (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
  if (g >= G) return;
  uint32_t run = 0;
  for (uint32_t b = 0; b < nblocks; b++) {
    const uint32_t c = part[(uint64_t)b * G + g];
    part[(uint64_t)b * G + g] = run;
    run += c;
  }
  hist[g] = run;
  off[g] = run;
}

__global__ void __launch_bounds__(MK_BLOCK) group_place_kernel(const uint32_t* __restrict__ group, uint64_t nq, uint64_t G,
                                                               uint64_t per_block, uint32_t* __restrict__ part,
                                                               const uint32_t* __restrict__ off, uint32_t* __restrict__ perm) {
  __shared__ uint32_t Gs[GQ_TILE];
  const uint64_t lo = (uint64_t)blockIdx.x * per_block, hi = min(nq, lo + per_block);
  uint32_t* row = part + (uint64_t)blockIdx.x * G;
  for (uint64_t t0 = lo; t0 < hi; t0 += GQ_TILE) {
    const uint64_t q = t0 + threadIdx.x;
    uint32_t g = q < hi ? group[q] : SENTINEL;
    if (g >= G) g = SENTINEL;                      // past the range, or refused by group_hist_kernel: no slot
    __syncthreads();                               // the previous tile has been read, and its shares have been added
    Gs[threadIdx.x] = g;
    __syncthreads();
    uint32_t before = 0, after = 0;
    if (g != SENTINEL) {
      for (uint32_t s = 0; s < GQ_TILE; s++) {
        const bool same = Gs[s] == g;
        before += (same && s < threadIdx.x) ? 1u : 0u;
        after += (same && s > threadIdx.x) ? 1u : 0u;
      }
      const uint32_t base = __hip_atomic_load(&row[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint64_t slot = (uint64_t)off[g] + base + before;
      if (slot < nq) perm[slot] = (uint32_t)q;
    }
    __syncthreads();                               // every query of the tile has read its base
    if (g != SENTINEL && after == 0) atomicAdd(&row[g], before + 1u);
  }
}

// out[u] = preds[used[u]]
__global__ void __launch_bounds__(MK_BLOCK) gather_preds_kernel(const pann_label_pred* __restrict__ preds, const uint32_t* __restrict__ used,
                                                                uint64_t m, pann_label_pred* __restrict__ out) {
  const uint64_t u = (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
  if (u < m) out[u] = preds[used[u]];
}

// slab row r <- the row of query perm[r], as bytes: dbytes of them, zeros up to slab_stride (a multiple of 16).  A thread moves
// 16 bytes; the query rows may start anywhere.
__global__ void __launch_bounds__(MK_BLOCK) gather_query_rows_kernel(const uint8_t* __restrict__ q, uint64_t q_stride, uint32_t dbytes,
                                                                     const uint32_t* __restrict__ perm, uint64_t rows,
                                                                     uint8_t* __restrict__ slab, uint32_t slab_stride) {
  const uint32_t cpr = slab_stride / 16;
  const uint64_t i = (uint64_t)blockIdx.x * MK_BLOCK + threadIdx.x;
  const uint64_t r = i / cpr;
  const uint32_t c = (uint32_t)(i % cpr);
  if (r >= rows) return;
  const uint4 v = load16_unaligned(q + (uint64_t)perm[r] * q_stride, c * 16, dbytes);
  *reinterpret_cast<uint4*>(slab + r * slab_stride + (size_t)c * 16) = v;
}

// row perm[r] of the outputs <- staged row r; counts[perm[r]] = its entries that are not padding.  One wave per row, k <= 128.
__global__ void __launch_bounds__(PANN_WAVE) scatter_knn_rows_kernel(const uint32_t* __restrict__ sids, const float* __restrict__ sdists,
                                                                     const uint32_t* __restrict__ perm, uint32_t k,
                                                                     uint32_t* __restrict__ out_ids, float* __restrict__ out_dists,
                                                                     uint32_t* __restrict__ out_counts) {
  const uint64_t r = blockIdx.x, q = perm[r];
  uint32_t cnt = 0;
  for (uint32_t j0 = 0; j0 < k; j0 += PANN_WAVE) {
    const uint32_t j = j0 + threadIdx.x;
    const uint32_t id = j < k ? sids[r * k + j] : SENTINEL;
    if (j < k) { out_ids[q * k + j] = id; out_dists[q * k + j] = sdists[r * k + j]; }
    cnt += (uint32_t)__popcll(__ballot(id != SENTINEL));
  }
  if (threadIdx.x == 0 && out_counts) out_counts[q] = cnt;
}

}  // namespace

void group_sort_shape(uint64_t nq, uint64_t G, uint32_t* nblocks, uint64_t* per_block) {
  const uint64_t tiles = (nq + GQ_TILE - 1) / GQ_TILE;
  const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>(tiles, (1ull << 20) / std::max<uint64_t>(G, 1)));   // `part` stays at 4 MB
  *per_block = (tiles + want - 1) / want * GQ_TILE;
  *nblocks = (uint32_t)((nq + *per_block - 1) / *per_block);
}

int group_queries_dev(const uint32_t* d_group, uint64_t nq, uint64_t G, uint32_t* d_flag, uint32_t* d_hist, uint32_t* d_off,
                      uint32_t* d_part, uint32_t* d_perm, hipStream_t st) {
  uint32_t nblocks; uint64_t per_block;
  group_sort_shape(nq, G, &nblocks, &per_block);
  PANN_HIP(hipMemsetAsync(d_flag, 0, 4, st));
  PANN_HIP(hipMemsetAsync(d_part, 0, (size_t)nblocks * G * 4, st));
  hipLaunchKernelGGL(group_hist_kernel, dim3(nblocks), dim3(MK_BLOCK), 0, st, d_group, nq, G, per_block, d_part, d_flag);
  PANN_HIP(hipGetLastError());
  hipLaunchKernelGGL(group_colscan_kernel, dim3((uint32_t)((G + MK_BLOCK - 1) / MK_BLOCK)), dim3(MK_BLOCK), 0, st, d_part, G, nblocks,
                     d_hist, d_off);
  PANN_HIP(hipGetLastError());
  hipLaunchKernelGGL(allow_block_scan_kernel, dim3(1), dim3(MK_BLOCK), 0, st, d_off, (uint32_t)G);
  PANN_HIP(hipGetLastError());
  hipLaunchKernelGGL(group_place_kernel, dim3(nblocks), dim3(MK_BLOCK), 0, st, d_group, nq, G, per_block, d_part, d_off, d_perm);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

int gather_preds_dev(const pann_label_pred* d_preds, const uint32_t* d_used, uint64_t m, pann_label_pred* d_out, hipStream_t st) {
  if (m == 0) return PANN_OK;
  hipLaunchKernelGGL(gather_preds_kernel, dim3((uint32_t)((m + MK_BLOCK - 1) / MK_BLOCK)), dim3(MK_BLOCK), 0, st, d_preds, d_used, m, d_out);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

size_t allow_rows_compact_scratch_bytes(uint64_t n, uint64_t rows) { return ((size_t)compaction_blocks(n) * rows + 1) * 4; }

int allow_rows_compact_dev(const uint32_t* d_allow, uint64_t n, const uint32_t* d_rowidx, uint64_t stride, uint32_t rows,
                           uint32_t* d_scratch, uint32_t* d_ids, uint32_t cap, hipStream_t st) {
  if (rows == 0 || n == 0) return PANN_OK;
  const uint32_t nblk = compaction_blocks(n);
  const dim3 grid(nblk, std::min<uint32_t>(rows, 65535));
  hipLaunchKernelGGL(allow_block_count_kernel, grid, dim3(MK_BLOCK), 0, st, d_allow, n, d_rowidx, stride, rows, d_scratch);
  PANN_HIP(hipGetLastError());
  // (grid.y strides over the rows, so the counts of row r lie at r * nblk whatever grid.y is)
  hipLaunchKernelGGL(allow_block_scan_kernel, dim3(1), dim3(MK_BLOCK), 0, st, d_scratch, nblk * rows);
  PANN_HIP(hipGetLastError());
  hipLaunchKernelGGL(allow_scatter_kernel, grid, dim3(MK_BLOCK), 0, st, d_allow, n, d_rowidx, stride, rows, (const uint32_t*)d_scratch, d_ids, cap);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

int gather_query_rows_dev(const uint8_t* d_q, uint64_t q_stride, uint32_t dbytes, const uint32_t* d_perm, uint64_t rows, uint8_t* d_slab,
                          uint32_t slab_stride, hipStream_t st) {
  if (rows == 0) return PANN_OK;
  const uint64_t work = rows * (slab_stride / 16);
  hipLaunchKernelGGL(gather_query_rows_kernel, dim3((uint32_t)((work + MK_BLOCK - 1) / MK_BLOCK)), dim3(MK_BLOCK), 0, st, d_q, q_stride,
                     dbytes, d_perm, rows, d_slab, slab_stride);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

int scatter_knn_rows_dev(const uint32_t* d_sids, const float* d_sdists, const uint32_t* d_perm, uint64_t rows, uint32_t k,
                         uint32_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, hipStream_t st) {
  if (rows == 0) return PANN_OK;
  hipLaunchKernelGGL(scatter_knn_rows_kernel, dim3((uint32_t)rows), dim3(PANN_WAVE), 0, st, d_sids, d_sdists, d_perm, k, d_out_ids,
                     d_out_dists, d_out_counts);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}


int allow_count_dev(const uint32_t* d_allow, uint64_t n, uint64_t rows, uint64_t stride, uint32_t* d_counts, hipStream_t st) {
  if (rows == 0) return PANN_OK;
  PANN_HIP(hipMemsetAsync(d_counts, 0, rows * 4, st));
  if (n == 0) return PANN_OK;
  const uint64_t words = (n + 31) / 32;
  const uint32_t per_row = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((words + 8 * MK_BLOCK - 1) / (8 * MK_BLOCK), 1), 256);
  hipLaunchKernelGGL(allow_count_kernel, dim3(per_row, (uint32_t)std::min<uint64_t>(rows, 65535)), dim3(MK_BLOCK), 0, st, d_allow, n,
                     rows, stride, d_counts);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

size_t allow_compact_scratch_bytes(uint64_t n) { return ((size_t)compaction_blocks(n) + 1) * 4; }

int allow_compact_count_dev(const uint32_t* d_allow, uint64_t n, uint32_t* d_scratch, const uint32_t** d_total, hipStream_t st) {
  const uint32_t nblk = compaction_blocks(n);
  hipLaunchKernelGGL(allow_block_count_kernel, dim3(nblk), dim3(MK_BLOCK), 0, st, d_allow, n, (const uint32_t*)nullptr, (uint64_t)0, 1u,
                     d_scratch);
  PANN_HIP(hipGetLastError());
  hipLaunchKernelGGL(allow_block_scan_kernel, dim3(1), dim3(MK_BLOCK), 0, st, d_scratch, nblk);
  PANN_HIP(hipGetLastError());
  *d_total = d_scratch + nblk;
  return PANN_OK;
}

int allow_compact_scatter_dev(const uint32_t* d_allow, uint64_t n, const uint32_t* d_scratch, uint32_t* d_ids, uint32_t count,
                              hipStream_t st) {
  hipLaunchKernelGGL(allow_scatter_kernel, dim3(compaction_blocks(n)), dim3(MK_BLOCK), 0, st, d_allow, n, (const uint32_t*)nullptr,
                     (uint64_t)0, 1u, d_scratch, d_ids, count);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

int knn_pad_dev(uint32_t* d_ids, float* d_dists, uint32_t* d_counts, uint64_t nq, uint32_t k, uint32_t cnt, int pad, hipStream_t st) {
  if (nq == 0 || (!pad && !d_counts)) return PANN_OK;
  const uint64_t work = pad ? nq * k : nq;
  hipLaunchKernelGGL(knn_pad_kernel, dim3((uint32_t)std::min<uint64_t>((work + MK_BLOCK - 1) / MK_BLOCK, 4096)), dim3(MK_BLOCK), 0, st,
                     d_ids, d_dists, d_counts, nq, k, cnt, pad);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

// the per-query scan on bitmap rows or on the labels with one predicate per query
int filter_scan_dev(const DeviceIndex& ix, hipStream_t st, const uint8_t* d_q, uint64_t q_stride, uint64_t nq, const PointFilter& F,
                    uint32_t k, uint32_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts) {
  if (nq == 0) return PANN_OK;
  if (k == 0 || k > PANN_WAVE) { set_error("masked scan: k must be in [1,64]"); return PANN_ERR_UNSUPPORTED; }
  const size_t qb = query_lds_bytes(ix);
  if (qb > 48 * 1024) { set_error("masked scan: rows too long for the scan's LDS state"); return PANN_ERR_UNSUPPORTED; }
  const bool by_labels = F.mode == MASK_LABELS;
  MaskedScanArgs P{};
  P.pv = PointsView{ix.points, ix.pstride, ix.nch, ix.exact}; P.dbytes = ix.dbytes;
  P.q = d_q; P.q_stride = q_stride; P.allow = F.allow; P.allow_stride = F.stride; P.n = ix.n; P.k = k;
  P.labels = F.labels; P.preds = F.preds; P.kind = (uint32_t)F.kind;      // (a bitmap filter has no labels, a label filter no rows)
  P.out_ids = d_out_ids; P.out_dists = d_out_dists; P.out_counts = d_out_counts;
#define CALL_MS(DT, MT, L, N1)                                                                                              \
  do {                                                                                                                      \
    if (by_labels) hipLaunchKernelGGL((masked_scan_kernel<DT, MT, L, N1, true>), dim3((uint32_t)nq), dim3(PANN_WAVE), qb, st, P);  \
    else hipLaunchKernelGGL((masked_scan_kernel<DT, MT, L, N1, false>), dim3((uint32_t)nq), dim3(PANN_WAVE), qb, st, P);    \
  } while (0)
  PANN_TYPE_SWITCH(ix, CALL_MS);
#undef CALL_MS
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

int labels_to_allow_dev(const uint32_t* d_labels, uint64_t n, int kind, const pann_label_pred* d_preds, uint64_t npreds,
                        uint32_t* d_allow, uint64_t stride, hipStream_t st) {
  if (npreds == 0 || n == 0) return PANN_OK;
  const uint32_t gx = (uint32_t)((n + LA_BLOCK_LABELS - 1) / LA_BLOCK_LABELS);
  hipLaunchKernelGGL(labels_to_allow_kernel, dim3(gx, (uint32_t)std::min<uint64_t>(npreds, 65535)), dim3(MK_BLOCK), 0, st, d_labels, n,
                     (uint32_t)kind, d_preds, npreds, d_allow, stride);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

int label_count_dev(const uint32_t* d_labels, uint64_t n, int kind, const pann_label_pred* d_preds, uint64_t npreds,
                    uint32_t* d_counts, hipStream_t st) {
  if (npreds == 0) return PANN_OK;
  PANN_HIP(hipMemsetAsync(d_counts, 0, npreds * 4, st));
  if (n == 0) return PANN_OK;
  const uint32_t gx = (uint32_t)((n + LC_TILE - 1) / LC_TILE);
  const uint32_t gy = (uint32_t)std::min<uint64_t>((npreds + MK_BLOCK - 1) / MK_BLOCK, 65535);
  hipLaunchKernelGGL(label_count_kernel, dim3(gx, gy), dim3(MK_BLOCK), 0, st, d_labels, n, (uint32_t)kind, d_preds, npreds, d_counts);
  PANN_HIP(hipGetLastError());
  return PANN_OK;
}

}  // namespace pann
