// vamana_delete.hip -- one batch of deletions consolidated on gfx950 (DESIGN.md "Deleting points").
//
// The reference has no deletion (knn_index::delete_set, vamanaRange/index.h:51, is never used); the rule is the delete
// consolidation of FreshDiskANN (Singh et al. 2021, Algorithm 4) with this project's snapshot semantics:
//
//   mark    bitmap of n bits <- the ids given (duplicates mean nothing)
//   count   one wave per vertex p not in D: does N(p) meet D?  how long is p's candidate list?      -> scan -> owners A, CSR offsets
//   fill    one wave per owner: survivors of N(p) in row order, then per deleted v in N(p), in row order, the survivors of N(v)
//           other than p, in row order; duplicates kept (the prune's sort + unique removes them, and counts them)
//   prune   robustPrune in the id-only form, add_out_nbrs = 0 (vamana_build.hip: prune_csr_dev), rows to a side buffer
//   write   only now: the rows of A are replaced, the rows of D emptied; count, fill and prune saw the graph as it was
//
// count and fill are ONE kernel template, so the two walks cannot disagree about a list's length.
#include <algorithm>
#include <vector>

#include "pann_internal.h"
#include "rocprim_temp.h"

namespace pann {

namespace {

constexpr int WAVE = 64;
constexpr int EXPAND_WAVES = 4;      // waves per block of the count / fill walk (no wave talks to another)
enum { SC_BAD = 0, SC_NDEL = 1, SC_MAXLEN = 2, SC_SUM64 = 8 /* a uint64, 8-byte aligned */, SC_WORDS = 64 };

__device__ __forceinline__ bool marked(const uint32_t* bitmap, uint32_t id) { return (bitmap[id >> 5] >> (id & 31u)) & 1u; }
__device__ __forceinline__ uint32_t below(uint64_t m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// sc[SC_BAD] |= an id >= n was given; sc[SC_NDEL] = |D| (an id counts when its bit was clear)
__global__ void delete_mark_kernel(const uint32_t* __restrict__ del, uint64_t m, uint64_t n, uint32_t* bitmap, uint32_t* sc) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  bool bad = false, fresh = false;
  if (i < m) {
    const uint32_t id = del[i];
    if (id >= n) bad = true;
    else { const uint32_t b = 1u << (id & 31u); fresh = (atomicOr(&bitmap[id >> 5], b) & b) == 0u; }
  }
  const uint64_t fm = __ballot(fresh), bm = __ballot(bad);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    if (bm) atomicOr(&sc[SC_BAD], 1u);
    if (fm) atomicAdd(&sc[SC_NDEL], (uint32_t)__popcll(fm));
  }
}

struct ExpandArgs {
  const uint32_t* graph; uint32_t gstride;
  const uint32_t* bitmap;
  uint64_t first, count;       // this launch starts at wave `first`; waves with work: n (count) or |A| (fill)
  uint32_t* cnt; uint32_t* flag; uint32_t* sc;                            // count: [n] list length, [n] p is an affected owner
  const uint32_t* owners; const uint64_t* offs; uint32_t* cand;           // fill: [|A|], [|A|] first slot of the owner's list
};

// One wave per vertex (count) / per affected owner (fill).  Rows are walked in wave-sized passes (gstride may exceed 64); lane i of
// a pass holds neighbour i, a ballot says which are deleted, and survivors are compacted with ballot + popcount.
template <bool FILL>
__global__ void __launch_bounds__(WAVE * EXPAND_WAVES) delete_expand_kernel(ExpandArgs A) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint64_t wv = A.first + blockIdx.x * (uint64_t)EXPAND_WAVES + (threadIdx.x >> 6);
  if (wv >= A.count) return;
  const uint32_t p = FILL ? A.owners[wv] : (uint32_t)wv;
  uint32_t* out = FILL ? A.cand + A.offs[wv] : nullptr;
  if (!FILL && marked(A.bitmap, p)) {          // members of D own no list
    if (lane == 0) { A.cnt[p] = 0; A.flag[p] = 0; }
    return;
  }
  const uint32_t* row = A.graph + (size_t)p * A.gstride;
  uint32_t w = 0;
  bool affected = false;
  for (uint32_t i0 = 0; i0 < A.gstride; i0 += WAVE) {                     // the surviving neighbours of p, in row order
    const uint32_t i = i0 + lane;
    const uint32_t a = i < A.gstride ? row[i] : SENTINEL;
    const bool valid = a != SENTINEL;
    const bool dead = valid && marked(A.bitmap, a);
    const uint64_t lm = __ballot(valid && !dead);
    affected = affected || __ballot(dead) != 0ull;
    if (FILL && valid && !dead) out[w + below(lm, lane)] = a;
    w += (uint32_t)__popcll(lm);
  }
  if (!FILL && !affected) {
    if (lane == 0) { A.cnt[p] = 0; A.flag[p] = 0; }
    return;
  }
  for (uint32_t i0 = 0; i0 < A.gstride; i0 += WAVE) {                     // per deleted neighbour v, in row order ...
    const uint32_t i = i0 + lane;
    const uint32_t a = i < A.gstride ? row[i] : SENTINEL;
    uint64_t dm = __ballot(a != SENTINEL && marked(A.bitmap, a));
    while (dm) {
      const int L = __ffsll((unsigned long long)dm) - 1;
      dm &= dm - 1;
      const uint32_t v = (uint32_t)__shfl((int)a, L);
      const uint32_t* rv = A.graph + (size_t)v * A.gstride;
      for (uint32_t j0 = 0; j0 < A.gstride; j0 += WAVE) {                 // ... the surviving neighbours of v other than p
        const uint32_t j = j0 + lane;
        const uint32_t b = j < A.gstride ? rv[j] : SENTINEL;
        const bool ok = b != SENTINEL && b != p && !marked(A.bitmap, b);
        const uint64_t km = __ballot(ok);
        if (FILL && ok) out[w + below(km, lane)] = b;
        w += (uint32_t)__popcll(km);
      }
    }
  }
  if (!FILL && lane == 0) { A.cnt[p] = w; A.flag[p] = 1; atomicMax(&A.sc[SC_MAXLEN], w); }
}

// A.count waves, in launches of at most launch_slice_blocks blocks (pann_internal.h)
template <bool FILL>
int launch_expand(ExpandArgs A, hipStream_t st) {
  const uint64_t slice = (uint64_t)launch_slice_blocks(WAVE * EXPAND_WAVES) * EXPAND_WAVES;
  for (A.first = 0; A.first < A.count; A.first += slice) {
    const uint64_t waves = std::min(slice, A.count - A.first);
    hipLaunchKernelGGL(delete_expand_kernel<FILL>, dim3((uint32_t)((waves + EXPAND_WAVES - 1) / EXPAND_WAVES)), dim3(WAVE * EXPAND_WAVES), 0, st, A);
    PANN_HIP(hipGetLastError());
  }
  return PANN_OK;
}

// A in increasing id: pos is the exclusive scan of flag
__global__ void delete_compact_kernel(const uint32_t* flag, const uint32_t* pos, const uint32_t* cnt, uint64_t n,
                                      uint32_t* owners, uint32_t* ocnt) {
  const uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (p < n && flag[p]) { owners[pos[p]] = (uint32_t)p; ocnt[pos[p]] = cnt[p]; }
}

// first key slot of the owners of one range, relative to the range
__global__ void delete_seg_kernel(const uint64_t* offs, uint32_t m, uint32_t* seg) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) seg[i] = (uint32_t)(offs[i] - offs[0]);
}

__global__ void delete_sum_kernel(const uint32_t* v, uint32_t m, unsigned long long* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long s = i < m ? v[i] : 0ull;
  for (int o = WAVE / 2; o; o >>= 1) s += __shfl_down(s, o);
  if ((threadIdx.x & (WAVE - 1)) == 0 && s) atomicAdd(out, s);
}

// one wave per affected owner: its new row (rows: [|A| x R], SENTINEL padded), with the filter codes when they are maintained
__global__ void __launch_bounds__(WAVE) delete_write_rows_kernel(uint32_t* graph, uint32_t gstride, const uint32_t* owners,
                                                                 const uint32_t* rows, uint32_t R, uint16_t* gcode,
                                                                 const uint16_t* rank16) {
  const uint32_t oi = blockIdx.x;
  const uint32_t p = owners[oi];
  uint32_t* row = graph + (size_t)p * gstride;
  uint16_t* crow = gcode ? gcode + (size_t)p * gstride : nullptr;
  for (uint32_t j = threadIdx.x; j < gstride; j += WAVE) {
    const uint32_t a = j < R ? rows[(size_t)oi * R + j] : SENTINEL;
    row[j] = a;
    if (crow) crow[j] = a == SENTINEL ? (uint16_t)0xFFFF : rank16[a];
  }
}

// one wave per id given: the row of a deleted vertex is emptied (an id given twice is emptied twice)
__global__ void __launch_bounds__(WAVE) delete_empty_rows_kernel(uint32_t* graph, uint32_t gstride, const uint32_t* del, uint16_t* gcode) {
  const uint32_t v = del[blockIdx.x];
  for (uint32_t j = threadIdx.x; j < gstride; j += WAVE) {
    graph[(size_t)v * gstride + j] = SENTINEL;
    if (gcode) gcode[(size_t)v * gstride + j] = (uint16_t)0xFFFF;
  }
}

}  // namespace

int vamana_delete_batch_dev(const DeviceIndex& ix, Workspace& ws, Workspace& prune_ws, Workspace& rows_ws, hipStream_t st,
                            const uint32_t* d_del, uint64_t m, uint32_t R, double alpha, uint64_t range_keys,
                            pann_delete_stats* stats) {
  if (m == 0) return PANN_OK;
  const auto t0 = now();
  const uint64_t n = ix.n;
  const size_t words = (size_t)((n + 31) / 32);

  const size_t stmp = std::max(scan_temp_bytes<uint32_t>((size_t)n), scan_temp_bytes<uint64_t>((size_t)n));
  uint32_t *sc, *cnt, *flag, *pos, *owners, *ocnt, *seg, *rcnt, *dc; uint64_t* offs; void* d_tmp;
  if (int rc = carve_into(ws, 4096, [&](Carve& b) {       // everything but the bitmap, the candidate slab and the rows; |A| <= n
    sc = b.take<uint32_t>(SC_WORDS);
    cnt = b.take<uint32_t>(n); flag = b.take<uint32_t>(n); pos = b.take<uint32_t>(n);
    owners = b.take<uint32_t>(n); ocnt = b.take<uint32_t>(n); offs = b.take<uint64_t>(n + 1);
    seg = b.take<uint32_t>(n); rcnt = b.take<uint32_t>(n); dc = b.take<uint32_t>(n);
    d_tmp = b.take<uint8_t>(stmp, 16);
  })) return rc;

  // ---- 1. mark ----
  HBuf bm;
  if (int rc = bm.ensure(words * 4)) return rc;
  uint32_t* bitmap = bm.as<uint32_t>();
  PANN_HIP(hipMemsetAsync(bitmap, 0, words * 4, st));
  PANN_HIP(hipMemsetAsync(sc, 0, SC_WORDS * 4, st));
  hipLaunchKernelGGL(delete_mark_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, d_del, m, n, bitmap, sc);
  PANN_HIP(hipGetLastError());
  uint32_t h_sc[2] = {0, 0};
  PANN_HIP(hipMemcpyAsync(h_sc, sc, 8, hipMemcpyDeviceToHost, st));
  PANN_HIP(hipStreamSynchronize(st));
  if (h_sc[SC_BAD]) { set_error("vamana delete: id out of range (>= number of points); nothing was changed"); return PANN_ERR_BAD_ARG; }
  const uint32_t ndel = h_sc[SC_NDEL];

  // ---- 2. count, scan, compact ----
  ExpandArgs ea{};
  ea.graph = ix.graph; ea.gstride = ix.gstride; ea.bitmap = bitmap;
  ea.count = n; ea.cnt = cnt; ea.flag = flag; ea.sc = sc;
  if (int rc = launch_expand<false>(ea, st)) return rc;
  size_t tb = stmp;
  PANN_HIP(rocprim::exclusive_scan(d_tmp, tb, flag, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
  uint32_t h_last[3] = {0, 0, 0};
  PANN_HIP(hipMemcpyAsync(&h_last[0], pos + (n - 1), 4, hipMemcpyDeviceToHost, st));
  PANN_HIP(hipMemcpyAsync(&h_last[1], flag + (n - 1), 4, hipMemcpyDeviceToHost, st));
  PANN_HIP(hipMemcpyAsync(&h_last[2], sc + SC_MAXLEN, 4, hipMemcpyDeviceToHost, st));
  PANN_HIP(hipStreamSynchronize(st));
  const uint32_t na = h_last[0] + h_last[1], max_len = h_last[2];

  // ---- 3. fill ----
  uint64_t total = 0;
  HBuf cand;
  if (na) {
    hipLaunchKernelGGL(delete_compact_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, flag, pos, cnt, n, owners, ocnt);
    PANN_HIP(hipGetLastError());
    tb = stmp;
    PANN_HIP(rocprim::exclusive_scan(d_tmp, tb, ocnt, offs, (uint64_t)0, (size_t)na, rocprim::plus<uint64_t>(), st));
    uint64_t h_off = 0; uint32_t h_cnt = 0;
    PANN_HIP(hipMemcpyAsync(&h_off, offs + (na - 1), 8, hipMemcpyDeviceToHost, st));
    PANN_HIP(hipMemcpyAsync(&h_cnt, ocnt + (na - 1), 4, hipMemcpyDeviceToHost, st));
    PANN_HIP(hipStreamSynchronize(st));
    total = h_off + h_cnt;
    if (int rc = cand.ensure((total + 1) * 4)) return rc;
    ea.count = na; ea.owners = owners; ea.offs = offs; ea.cand = cand.as<uint32_t>();
    if (int rc = launch_expand<true>(ea, st)) return rc;
  }
  PANN_HIP(hipStreamSynchronize(st));
  const auto t1 = now();

  // ---- 4. prune, in ranges of owners whose keys fit the prune's 32-bit key index; all against the same snapshot ----
  uint16_t* const gcode = ix.codes_valid ? ix.gcode : nullptr;      // filter codes maintained with the rows (filter_codes.hip)
  if (na) {
    const uint64_t cap = std::min<uint64_t>(range_keys ? range_keys : ~0ull, 0xFFFFFFEFull);
    std::vector<uint32_t> bounds{0u};
    std::vector<uint64_t> h_offs;
    if (total > cap) {
      h_offs.resize((size_t)na + 1);
      PANN_HIP(hipMemcpy(h_offs.data(), offs, (size_t)na * 8, hipMemcpyDeviceToHost));
      h_offs[na] = total;
      uint32_t lo = 0;
      for (uint32_t i = 1; i <= na; i++)         // a range takes owners while its keys fit, and at least one
        if (h_offs[i] - h_offs[lo] > cap && i - 1 > lo) { bounds.push_back(i - 1); lo = i - 1; }
    }
    bounds.push_back(na);
    if (int rc = rows_ws.ensure((size_t)na * R * 4 + 256)) return rc;
    uint32_t* d_rows = (uint32_t*)rows_ws.buf;
    PANN_HIP(hipMemsetAsync(dc, 0, (size_t)na * 4, st));
    for (size_t r = 0; r + 1 < bounds.size(); r++) {
      const uint32_t lo = bounds[r], cntr = bounds[r + 1] - lo;
      const uint64_t keys = h_offs.empty() ? total : h_offs[lo + cntr] - h_offs[lo];
      if (keys >= 0xFFFFFFF0ull) { set_error("vamana delete: one candidate list exceeds the key index"); return PANN_ERR_OVERFLOW; }
      hipLaunchKernelGGL(delete_seg_kernel, dim3((cntr + 255) / 256), dim3(256), 0, st, offs + lo, cntr, seg + lo);
      PANN_HIP(hipGetLastError());
      if (int rc = prune_csr_dev(ix, prune_ws, st, owners + lo, cntr, cand.as<uint32_t>(), offs + lo, ocnt + lo, seg + lo,
                                 (uint32_t)keys, max_len, alpha, R, d_rows + (size_t)lo * R, rcnt + lo, dc + lo)) return rc;
      PANN_HIP(hipStreamSynchronize(st));        // the next range reuses the key scratch (and may regrow it)
    }
    // ---- 5. write: every prune is done ----
    for (uint32_t i0 = 0; i0 < na; i0 += launch_slice_blocks(WAVE)) {
      hipLaunchKernelGGL(delete_write_rows_kernel, dim3(std::min(na - i0, launch_slice_blocks(WAVE))), dim3(WAVE), 0, st, ix.graph, ix.gstride,
                         owners + i0, d_rows + (size_t)i0 * R, R, gcode, ix.rank16);
      PANN_HIP(hipGetLastError());
    }
  }
  for (uint64_t i0 = 0; i0 < m; i0 += launch_slice_blocks(WAVE)) {
    const uint32_t c = (uint32_t)std::min<uint64_t>(m - i0, launch_slice_blocks(WAVE));
    hipLaunchKernelGGL(delete_empty_rows_kernel, dim3(c), dim3(WAVE), 0, st, ix.graph, ix.gstride, d_del + i0, gcode);
    PANN_HIP(hipGetLastError());
  }
  unsigned long long h_sum = 0;
  if (stats && na) {
    hipLaunchKernelGGL(delete_sum_kernel, dim3((na + 255) / 256), dim3(256), 0, st, dc, na, reinterpret_cast<unsigned long long*>(sc + SC_SUM64));
    PANN_HIP(hipGetLastError());
    PANN_HIP(hipMemcpyAsync(&h_sum, sc + SC_SUM64, 8, hipMemcpyDeviceToHost, st));
  }
  PANN_HIP(hipStreamSynchronize(st));
  const auto t2 = now();
  if (stats) {
    if (stats->per_point_dist_cmps && na) {
      std::vector<uint32_t> ho(na), hd(na);
      PANN_HIP(hipMemcpy(ho.data(), owners, (size_t)na * 4, hipMemcpyDeviceToHost));
      PANN_HIP(hipMemcpy(hd.data(), dc, (size_t)na * 4, hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < na; i++) stats->per_point_dist_cmps[ho[i]] += hd[i];
    }
    stats->t_expand_s += secs(t0, t1); stats->t_prune_s += secs(t1, t2);
    stats->deleted += ndel; stats->affected += na; stats->candidates += total; stats->prune_dist_cmps += h_sum;
  }
  return PANN_OK;
}

}  // namespace pann
