// beam_search.hip -- batched greedy beam search on gfx950: ONE WAVEFRONT PER QUERY.
//
// Replaces the parallel_for over queries of searchAll/qsearchAll (beamSearch.h:374,556) and the
// per-insert searches of Vamana's batch_insert (vamana/index.h:247-259); each wave runs the exact
// state machine of filtered_beam_search (beamSearch.h:22-214, use_filtering == false):
//
//   frontier F[<=beam]  sorted (dist,id) keys in LDS, one "visited" flag per entry
//   filter   H[1<<bits] the reference's lossy direct-mapped table (LDS up to 16 KB, else HBM)
//   cands    C[...]     survivors of `dist < cutoff`, accumulated across skipped merges (:162-168)
//
// Per iteration: pick first unvisited frontier entry -> one aligned read of its adjacency row
// (lane i <- neighbour i) -> wave-parallel replay of the SEQUENTIAL filter update (:130-136) ->
// gather distances, LPC lanes x 16 B per candidate vector so every load instruction covers whole
// rows (coalesced 64..512 B segments) -> ballot-compaction of candidates -> rank-based merge.
//
// Equivalences used (proved in DESIGN.md "Kernel 1"):
//  * unvisited_frontier[offset] (:109) == first frontier entry whose flag is clear, because the
//    frontier does not change between merges and the skipped entries are exactly the flagged ones.
//  * set_difference(frontier, visited) (:203-208) == entries with flag clear, provided an entry
//    that re-enters the frontier after having been visited gets its flag back.  That can only
//    happen while the frontier is not full (cut-prune :190-195 dropped it); such entries are kept
//    in a small per-query "dropped" list and candidates are checked against it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pann_device.h"

namespace pann {

// Diagnostic build only (make STAMPS=1 -> lib/libpann_stamps.so): s_memtime at the phase boundaries
// of an iteration, summed per query into a buffer nothing else reads (guide section 7, In-kernel
// stamps).  In the shipped library PANN_STAMP() expands to nothing.
#ifndef PANN_GU
#define PANN_GU 4   /* candidate groups in flight per lane in the main gather */
#endif
#ifndef PANN_GU_B128
/* beam 65..128: a whole adjacency row per memory round trip (16 groups in flight) was measured SLOWER than 4
   (C3 build search phase 1.50 s vs 1.19 s); rows of several chunks per lane halve the group count inside
   gather_tile, so they ask for 8 here (= 4 groups x 3 chunks in flight) */
#define PANN_GU_B128(LPC, NCH1) 4   /* round 3, with the filter-code table: 4 / 8 / 16 for multi-chunk rows = 0.720 / 0.743 / 0.885 s (C3 2M search phase) */
#endif
#ifndef PANN_MINWAVES
#define PANN_MINWAVES 1
#endif
#ifndef PANN_B128_PAIR_CODES
/* beam 65..128: two vertices per memory round trip while merges are skipped.  Only the CODES variant has the path (the whole
   filter in 6 KB of LDS, no table traffic): C3 2M search phase 0.743 -> 0.712 s.  With the id table it was exact but slower
   (C3-shaped 2M build, search phase 0.864 s without vs 0.91..0.93 s with it: the kernel already moves 5.1 TB/s on the HBM side,
   81 % of the 6.3 TB/s random-row ceiling, so more bytes in flight buy nothing and the rows fetched for nothing when row 1 ends
   the skipping cost bandwidth), and that form has been removed. */
#define PANN_B128_PAIR_CODES 1
#endif
#ifndef PANN_B64_PREFETCH
#define PANN_B64_PREFETCH 1   /* speculative adjacency-row fetch in the beam-64 kernel (0: A/B library builds) */
#endif
#ifndef PANN_MINWAVES_B64
#define PANN_MINWAVES_B64 7   /* at least 7 waves per SIMD (<= 72 VGPRs); the kernel uses 61 -> 8 waves, LDS caps a CU at 30 queries */
#endif
#ifdef PANN_STAMPS
#define PANN_STAMP(slot)                                                                        \
  do {                                                                                          \
    unsigned long long t_;                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                          \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                   \
    __builtin_amdgcn_sched_barrier(0);                                                          \
    stamp_sum[slot] += t_ - stamp_prev;                                                         \
    stamp_prev = t_;                                                                            \
  } while (0)
/* once per query: before its first PANN_STAMP / after its last (the kernel's `lane` and `P` are in scope) */
#define PANN_STAMP_BEGIN()                                                                      \
  unsigned long long stamp_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, stamp_prev;                       \
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_prev)::"memory")
#define PANN_STAMP_FLUSH(qi)                                                                    \
  do {                                                                                          \
    if (lane == 0 && P.stamps) for (int i_ = 0; i_ < 8; i_++) P.stamps[(size_t)(qi) * 8 + i_] = stamp_sum[i_]; \
  } while (0)
#else
#define PANN_STAMP(slot) do { } while (0)
#define PANN_STAMP_BEGIN() ((void)0)
#define PANN_STAMP_FLUSH(qi) ((void)0)
#endif

// every kernel of this file runs ONE wavefront per workgroup
#ifdef PANN_FULL_BARRIERS
#define PANN_WSYNC() __syncthreads()
#else
#define PANN_WSYNC() wave_lds_sync()
#endif

struct BSParams {
  const uint8_t* points; uint32_t pstride; uint32_t dbytes; uint32_t nch; uint32_t exact;
  const uint32_t* graph; uint32_t gstride; uint32_t max_deg;
  const uint8_t* queries; uint64_t qstride; const uint32_t* query_ids;
  const uint32_t* starts; uint32_t nstarts; uint32_t starts_stride;   // starts_stride: 0 shared, nstarts per query
  uint32_t nq;
  uint32_t k, beam, limit, degree_limit; double cut;
  uint32_t skip_enabled;   // QP.limit >= 2*beam (:163)
  uint32_t cut_enabled;    // QP.k > 0 && is_metric() (:190)
  uint32_t bits;           // log2 of filter size (:52)
  uint32_t bcap, ccap;     // LDS capacities (multiples of 64)
  uint32_t* hash_global;   // [slots][1<<bits] when the filter does not fit LDS
  uint32_t prio_start;     // first block index that runs with raised issue priority (register-frontier beam-64 kernel)
  uint32_t hsplit;         // beam 65..128 in HBM mode: 0 whole table in HBM, 1 half, 2 three quarters of it in LDS
  uint32_t p24;            // ... whose LDS part holds planar 24-bit entries (n < 2^24 - 1)
  const uint32_t* order;   // launch slot -> query (or null: identity).  Results do not depend on it: every output is indexed by the query
  const uint16_t* gcode;   // filter-code table (filter_codes.hip): codes of the neighbours, slot-aligned with the graph rows
  const uint16_t* rank16;  // ... and of every id (start points)
  uint64_t* dropped; uint32_t dcap;  // [nq][dcap] visited entries that left a non-full frontier
  uint32_t* work_counter;  // persistent variant: next query to take
  uint32_t* status;        // [0] |= 1 on visited-list overflow, |= 2 on dropped-list overflow
  pann_search_out out;
  unsigned long long* stamps;   // diagnostic build: [nq][8] cycle sums
  // second level (FILTER variants of the generic kernel only): bit sketches, see sketch.hip
  const uint8_t* sketch; uint32_t sk_stride;      // [n] rows of sk_stride bytes (a multiple of 16, zero padded)
  union { uint32_t sk_kind; uint32_t fill; };     // PANN_SKETCH_* | STEER (no sketch there): the two-hop pass stops at `fill` entries of pruned (1..deg_eff)
  uint32_t sk_as_written, sk_nblk;                // Hamming loop as written; 64-bit blocks per sketch
  const uint8_t* sketch_queries; uint64_t sq_stride; uint32_t sk_row_bytes;   // external queries: nq host-layout rows
  union { uint32_t sk_lds_off; uint32_t br_off; };        // byte offset of the query sketch in LDS | STEER: of the bridge list
  union { uint32_t* pruned_cmps; uint32_t* steer_out; };  // [nq] optional: starts + neighbours that passed the hash filter | STEER: [nq][2]
                                                  // optional: bridge rows expanded, entries appended by the two-hop pass
  // masked search (MASKED variants only): allow bitmap, see DESIGN.md "Masked search"
  const uint32_t* allow; uint64_t allow_stride;   // point i is allowed iff bit i & 31 of word i >> 5; query q reads row q (stride in words, 0: shared)
  uint32_t* result_count; uint32_t* allowed_cmps; // [nq] optional: entries of the result list; full distances of allowed points
  uint32_t rl_off;                                // byte offset of the result list in LDS (64 keys), then the keys of one gather (64)
  // ... by label predicates (MASK_LABELS variants only), see DESIGN.md "Label predicates"
  const uint32_t* labels;                         // [n] one word per point
  const pann_label_pred* preds; uint32_t pred_stride, pred_kind;   // query q reads preds[q * pred_stride] (0: shared); PANN_PRED_*
  // The steered masked search (STEER variants, DESIGN.md "Steered masked search") keeps its three parameters in the storage of sketch
  // fields (the unions above): it has no sketch form, and the kernel argument block of every other instantiation stays byte for byte
  // what it was.
};

template <bool HASH_LDS>
__device__ __forceinline__ void hstore(uint32_t* H, uint32_t s, uint32_t v) {
  if constexpr (HASH_LDS) H[s] = v;
  else __hip_atomic_store(H + s, v, __ATOMIC_RELAXED, PANN_PRIVATE_SCOPE);
}
template <bool HASH_LDS>
__device__ __forceinline__ void hsync() {
  if constexpr (!HASH_LDS) __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0): global table ops retire in order
  PANN_WSYNC();
}

// first index in sorted A[0..n) with A[i] >= key
__device__ __forceinline__ uint32_t lower_bound_lds(const uint64_t* A, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (A[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Replay of `for a in row: has_been_seen(a)` (:54-59,:131-136) for up to 64 ids held one per lane.
// Sequential semantics: after lane j is processed table[s_j] == a_j whether or not it was a hit, so
// lane i is a hit iff the LAST earlier lane with the same slot holds the same id, or, when there is
// none, iff the table held a_i on entry.  Returns "seen" per lane and leaves the table as the
// sequential loop would.
// Lanes that share a slot are found by writing the lane number somewhere slot-indexed and reading it
// back: into the table itself when it lives in LDS; into a 1 KB LDS scratch T (index = slot mod 1024,
// false sharing only costs a loop trip) when the table lives in HBM, which then sees ONE dependent
// load (the entry values) and one fire-and-forget store per call instead of four round trips.
// Split mode (HBM branch, hb = 1 or 2): the slots whose low hb bits are all ones live in HBM (index s >> hb), the
// other half / three quarters in LDS right after T -- fewer single-word L2 requests per row for a smaller LDS
// footprint than the whole table.
// hb == 3: the WHOLE table in LDS as 24-bit planes (12 KB at beam 128) -- no table traffic to HBM at all
__device__ __forceinline__ uint32_t split_lds_index(uint32_t s, uint32_t hb) {
  return hb == 1 ? (s >> 1) : hb == 3 ? s : (s >> 2) * 3 + (s & 3);
}
// Planar 24-bit entries (p24 != 0: n < 2^24 - 1, the LDS part only): a low plane of uint16 followed by a high plane of uint8,
// 3 bytes per slot instead of 4 -- exact (an id IS 24 bits), and 2 KB less LDS per query at beam 65..128.
struct LdsPart { uint8_t* base; uint32_t nslots; uint32_t p24; };
__device__ __forceinline__ uint32_t lds_part_load(const LdsPart& L, uint32_t i) {
  if (L.p24) {
    const uint32_t lo = reinterpret_cast<const uint16_t*>(L.base)[i];
    const uint32_t hi = (L.base + 2 * L.nslots)[i];
    return lo | (hi << 16);                                              // empty slot = 0xFFFFFF, never equal to an id
  }
  return reinterpret_cast<const uint32_t*>(L.base)[i];
}
__device__ __forceinline__ void lds_part_store(const LdsPart& L, uint32_t i, uint32_t a) {
  if (L.p24) {
    reinterpret_cast<uint16_t*>(L.base)[i] = (uint16_t)a;
    (L.base + 2 * L.nslots)[i] = (uint8_t)(a >> 16);
  } else {
    reinterpret_cast<uint32_t*>(L.base)[i] = a;
  }
}
__device__ __forceinline__ void lds_part_clear(const LdsPart& L, int lane) {
  if (L.p24) {      // 3 * nslots bytes of 0xFF, nslots a multiple of 64
    uint32_t* w = reinterpret_cast<uint32_t*>(L.base);
    for (uint32_t i = lane; i < (3 * L.nslots) / 4; i += PANN_WAVE) w[i] = 0xFFFFFFFFu;
  } else {
    uint32_t* w = reinterpret_cast<uint32_t*>(L.base);
    for (uint32_t i = lane; i < L.nslots; i += PANN_WAVE) w[i] = SENTINEL;
  }
}

// victim (optional, table in LDS): per lane, the id this call evicted from the table -- the value the lane's slot held on entry,
// reported by the lane that writes the slot, when it was another id than the one written -- or SENTINEL.
template <bool HASH_LDS>
__device__ __forceinline__ bool filter_update(uint32_t* H, uint32_t hmask, bool active, uint32_t a, int lane,
                                              uint8_t* T = nullptr, uint32_t hb = 0, LdsPart Lp = LdsPart{nullptr, 0, 0},
                                              uint32_t* victim = nullptr) {
  const uint32_t s = (uint32_t)hash64_2((uint64_t)a) & hmask;
  uint32_t old, w;
  const uint32_t hm = (1u << hb) - 1u;
  const bool in_hbm = hb != 3 && (s & hm) == hm;                        // always true when hb == 0, never when hb == 3
  if constexpr (HASH_LDS) {
    old = active ? H[s] : 0u;
    PANN_WSYNC();
    if (active) H[s] = (uint32_t)lane;                   // some lane of each slot group wins
    PANN_WSYNC();
    w = active ? H[s] : (uint32_t)lane;
  } else {
    __builtin_amdgcn_s_waitcnt(0);                       // the previous call's table stores have been acknowledged
    old = 0u;
    if (active) old = in_hbm ? __hip_atomic_load(H + (s >> hb), __ATOMIC_RELAXED, PANN_PRIVATE_SCOPE) : lds_part_load(Lp, split_lds_index(s, hb));
    const uint32_t t = s & 1023u;
    if (active) T[t] = (uint8_t)lane;
    PANN_WSYNC();
    w = active ? (uint32_t)T[t] : (uint32_t)lane;
  }
  uint64_t losers = __ballot(active && w != (uint32_t)lane);
  int prev = -1;       // last earlier lane with my slot
  bool last = true;    // no later lane with my slot
  while (losers) {     // one trip per slot shared by >1 lane (about 2 per 64 ids at 1024 slots)
    const int L = __ffsll((unsigned long long)losers) - 1;
    const uint32_t sL = __builtin_amdgcn_readlane(s, L);
    const uint64_t grp = __ballot(active && s == sL);
    losers &= ~grp;
    if (active && s == sL) {
      const uint64_t below = grp & ((1ull << lane) - 1ull);
      prev = below ? 63 - __clzll((unsigned long long)below) : -1;
      last = (lane == 63) ? true : ((grp >> (lane + 1)) == 0ull);
    }
  }
  const uint32_t a_prev = __shfl(a, prev < 0 ? lane : prev);
  const bool seen = active && (prev >= 0 ? (a_prev == a) : (old == a));
  if constexpr (HASH_LDS) {
    if (victim) *victim = (active && last && old != SENTINEL && old != a) ? old : SENTINEL;
    PANN_WSYNC();
    if (active && last) H[s] = a;
    PANN_WSYNC();
  } else {
    if (active && last) {
      if (in_hbm) __hip_atomic_store(H + (s >> hb), a, __ATOMIC_RELAXED, PANN_PRIVATE_SCOPE);
      else lds_part_store(Lp, split_lds_index(s, hb), a);
    }
    PANN_WSYNC();                                     // T (and the LDS part) may be touched by the next call
  }
  return seen;
}

// The same replay on a table of 12-bit CLASS CODES (filter_codes.hip): slot s remembers the code of the id written last, and
// "table[s] == a" is "table[s] == code(a)" because (slot, code) <-> id is a bijection.  4 096 slots take 6 KB of LDS: an 8-bit
// plane P8[s] and a 4-bit plane, eight slots per dword of P4.  Two lanes of one instruction may own different nibbles of one
// dword, so the nibble is written with ds_mskor_b32 (D = (D & ~mask) | data, atomic per lane).  Empty slot = 0xFFF (no code is).
// Lanes that share a slot are found through the 1 KB byte scratch T as in the HBM-table form above.
// What one filter_update_codes call changed, per lane: enough to put the table back (a row that was scanned speculatively and
// turns out not to be the next vertex must leave no trace in the lossy table, whose state decides later hits and misses).
struct FilterUndo { uint32_t s, old; bool wrote; };
__device__ __forceinline__ void code_store(uint8_t* P8, uint32_t* P4, uint32_t s, uint32_t code) {
  const uint32_t sh = (s & 7u) * 4u;
  P8[s] = (uint8_t)code;
  const uint32_t addr = (uint32_t)(uintptr_t)(P4 + (s >> 3));            // LDS byte address (low 32 bits of the flat address)
  asm volatile("ds_mskor_b32 %0, %1, %2" ::"v"(addr), "v"(0xFu << sh), "v"((code >> 8) << sh) : "memory");
}
__device__ __forceinline__ void filter_undo_codes(uint8_t* P8, uint32_t* P4, const FilterUndo& u) {
  if (u.wrote) code_store(P8, P4, u.s, u.old);
  PANN_WSYNC();
}
__device__ __forceinline__ bool filter_update_codes(uint8_t* P8, uint32_t* P4, uint32_t hmask, bool active, uint32_t a, uint32_t code,
                                                    int lane, uint8_t* T, FilterUndo* undo = nullptr) {
  const uint32_t s = (uint32_t)hash64_2((uint64_t)a) & hmask;
  const uint32_t sh = (s & 7u) * 4u;
  uint32_t old = 0x1000u;
  if (active) old = (uint32_t)P8[s] | (((P4[s >> 3] >> sh) & 0xFu) << 8);
  const uint32_t t = s & 1023u;
  if (active) T[t] = (uint8_t)lane;
  PANN_WSYNC();
  const uint32_t w = active ? (uint32_t)T[t] : (uint32_t)lane;
  uint64_t losers = __ballot(active && w != (uint32_t)lane);
  int prev = -1;       // last earlier lane with my slot
  bool last = true;    // no later lane with my slot
  while (losers) {
    const int L = __ffsll((unsigned long long)losers) - 1;
    const uint32_t sL = __builtin_amdgcn_readlane(s, L);
    const uint64_t grp = __ballot(active && s == sL);
    losers &= ~grp;
    if (active && s == sL) {
      const uint64_t below = grp & ((1ull << lane) - 1ull);
      prev = below ? 63 - __clzll((unsigned long long)below) : -1;
      last = (lane == 63) ? true : ((grp >> (lane + 1)) == 0ull);
    }
  }
  const uint32_t a_prev = __shfl(a, prev < 0 ? lane : prev);
  const bool seen = active && (prev >= 0 ? (a_prev == a) : (old == code));
  if (undo) { undo->s = s; undo->old = old; undo->wrote = active && last; }   // `old` of a slot group: the code on entry
  if (active && last) code_store(P8, P4, s, code);
  PANN_WSYNC();                                          // T and the table may be touched by the next call
  return seen;
}

// Distances from the query to the m ids in Pl[0..m); survivors of `dist < cutoff` (:157) are
// appended to C in row order.
template <int DT, int METRIC, int LPC, bool NCH1, int U, bool BATCH_EMIT = true>
__device__ __forceinline__ uint32_t gather_distances(const BSParams& P, const QReg<DT>& qreg,
                                                     const uint4* qlds, const uint32_t* Pl, uint32_t m,
                                                     uint32_t cutoff_ord, uint64_t* C, uint32_t c, int lane) {
  const PointsView PV{P.points, P.pstride, P.nch, P.exact};
  if constexpr (BATCH_EMIT) {
    // one append per gather iteration (G*U candidates): +4 % on the beam-64 kernel at 10K queries
    gather_tile<DT, METRIC, LPC, NCH1, U>(PV, qreg, qlds, Pl, m, lane,
      [&](bool has, uint32_t, uint32_t id, float dist, uint64_t before) {
        const uint32_t ord = f2ord(dist);
        const bool pass = has && (ord < cutoff_ord);
        const uint64_t pm = __ballot(pass);
        if (pass) C[c + (uint32_t)__popcll(pm & before)] = ((uint64_t)ord << 32) | id;
        c += __popcll(pm);
      });
  } else {
    // one append per candidate group (the beam-128 kernel measured 2.5 % slower with the batched form)
    gather_tile<DT, METRIC, LPC, NCH1, U>(PV, qreg, qlds, Pl, m, lane,
      [&](bool has, uint32_t, uint32_t id, float dist) {
        const uint32_t ord = f2ord(dist);
        const bool pass = has && (ord < cutoff_ord);
        const uint64_t pm = __ballot(pass);
        if (pass) C[c + lanes_below(pm, lane)] = ((uint64_t)ord << 32) | id;
        c += __popcll(pm);
      });
  }
  return c;
}

// The same for the survivors of TWO rows listed one after the other in Pl (row 1: Pl[0..split), row 2: the rest):
// *c_split = size of C after the candidates of row 1 alone (the appends keep Pl order).
template <int DT, int METRIC, int LPC, bool NCH1, int U>
__device__ __forceinline__ uint32_t gather_distances_split(const BSParams& P, const QReg<DT>& qreg, const uint4* qlds,
                                                           const uint32_t* Pl, uint32_t m, uint32_t split, uint32_t cutoff_ord,
                                                           uint64_t* C, uint32_t c, int lane, uint32_t* c_split) {
  const PointsView PV{P.points, P.pstride, P.nch, P.exact};
  uint32_t c1 = c;
  gather_tile<DT, METRIC, LPC, NCH1, U>(PV, qreg, qlds, Pl, m, lane,
    [&](bool has, uint32_t ci, uint32_t id, float dist) {
      const uint32_t ord = f2ord(dist);
      const bool pass = has && (ord < cutoff_ord);
      const uint64_t pm = __ballot(pass);
      if (pass) C[c + lanes_below(pm, lane)] = ((uint64_t)ord << 32) | id;
      c += __popcll(pm);
      c1 += __popcll(__ballot(pass && ci < split));
    });
  *c_split = c1;
  return c;
}


// ---- masked search: the result list (DESIGN.md "Masked search") ----
// The min(out_k, count) smallest keys among the ALLOWED points whose full distance the search computed, kept beside the
// traversal, which never looks at it: one key per lane, ascending, KEY_INF beyond the fill.  `thr` (wave-uniform) is its
// out_k-th entry: a key at or above it cannot enter the result.  The list itself keeps up to 64 entries, so a point that is
// compared again (the hash filter is lossy) and would enter is always still there to be recognised.
// The keys live in LDS (L[lane], touched by their own lane only) and are in registers only while a key is being inserted: the
// beam-64 kernel has no VGPRs to spare while the rows of a gather are in flight.
// (The masked helpers below carry a trailing template flag S that changes nothing in them: the STEER kernels instantiate their own
// copies, S = true.  hipcc's code for a kernel depends on which other kernels share its inlined helpers -- with shared copies 41 MASKED
// instantiations of the generic kernel came out with one or two more VGPRs; DESIGN.md "Steered masked search".)
struct MaskedList { uint64_t* L; uint64_t thr; uint32_t cmps; };
template <bool S = false>
__device__ __forceinline__ void masked_offer(MaskedList& R, uint64_t key, bool allowed, uint32_t thr_lane, int lane) {
  R.cmps += __popcll(__ballot(allowed));
  uint64_t bm = __ballot(allowed && key < R.thr);
  if (bm == 0ull) return;                                 // the common case once the list is full
  uint64_t lk = R.L[lane];
  while (bm) {                                            // uniform: one trip per key that may enter
    const int l = __ffsll((unsigned long long)bm) - 1;
    bm &= bm - 1;
    const uint64_t kk = readlane64(key, l);
    if (kk >= R.thr) continue;                            // an earlier trip tightened the threshold
    if (__ballot((uint32_t)lk == (uint32_t)kk) != 0ull) continue;   // compared before: equal ids <=> equal keys
    const uint32_t r = __popcll(__ballot(lk < kk));       // rank of the new key
    const uint64_t up = __shfl_up(lk, 1);
    if (lane > (int)r) lk = up; else if (lane == (int)r) lk = kk;
    R.thr = readlane64(lk, (int)thr_lane);
  }
  R.L[lane] = lk;
}

// Where a MASKED kernel's verdict on a compared point comes from.  MASK_BITMAP: W is the query's bitmap row, the word of point a
// is W[a >> 5] and the verdict its bit a & 31.  MASK_LABELS: W is the label array, the word of point a is W[a] and the verdict the
// query's predicate on it; kind, pa and pb are wave-uniform and are forced into scalar registers once per query, so the label
// form holds no vector register the bitmap form does not.  Either way ONE 4-byte load per compared point, issued at the same place.
struct MaskSrc { const uint32_t* W; uint32_t kind, pa, pb; };
template <int MODE, bool S = false>
__device__ __forceinline__ MaskSrc mask_src(const BSParams& P, uint32_t qi) {
  if constexpr (MODE == MASK_LABELS) {
    const pann_label_pred* pp = P.preds + (size_t)qi * P.pred_stride;
    return MaskSrc{P.labels, P.pred_kind, (uint32_t)__builtin_amdgcn_readfirstlane((int)pp->a),
                   (uint32_t)__builtin_amdgcn_readfirstlane((int)pp->b)};
  } else {
    return MaskSrc{P.allow + (size_t)qi * P.allow_stride, 0u, 0u, 0u};
  }
}
template <int MODE, bool S = false>
__device__ __forceinline__ uint32_t mask_word(const MaskSrc& M, uint32_t a) {
  if constexpr (MODE == MASK_LABELS) return M.W[a];
  else return M.W[a >> 5];
}
template <int MODE, bool S = false>
__device__ __forceinline__ bool mask_verdict(const MaskSrc& M, uint32_t aword, uint32_t note) {
  if constexpr (MODE == MASK_LABELS) return label_pred(M.kind, M.pa, M.pb, aword);
  else return ((aword >> (note & 31u)) & 1u) != 0u;
}

// What the lane that owns a filter survivor keeps across the gather: position in Pl and bit number of its id (0: owns none).
template <bool S = false>
__device__ __forceinline__ uint32_t masked_note(bool mine, uint32_t mypos, uint32_t a) {
  return mine ? (0x80000000u | (mypos << 5) | (a & 31u)) : 0u;
}

// gather_distances (batched emit) for the MASKED kernels.  The callback does what gather_distances' does and also leaves every
// candidate's key -- at or beyond the cutoff too -- in LDS at its index in Pl (MK, 64 keys behind the result list).  After the
// gather the lane that owns candidate Pl[mypos] (`note`, masked_note) reads that key back and tests its own bit (MASK_LABELS: its
// label against the query's predicate): the word `aword` was requested before the row loads of the gather and is first used here,
// after all of them, so it adds no dependent round trip, and the callback holds nothing but a ballot and LDS stores.  One offer of
// up to 64 keys per call.
template <int DT, int METRIC, int LPC, bool NCH1, int U, int MODE, bool S = false>
__device__ __forceinline__ uint32_t gather_distances_masked(const BSParams& P, const QReg<DT>& qreg, const uint4* qlds,
                                                            const uint32_t* Pl, uint32_t m, uint32_t cutoff_ord, uint64_t* C,
                                                            uint32_t c, int lane, uint32_t note, uint32_t aword, const MaskSrc& M,
                                                            MaskedList& R, uint32_t thr_lane) {
  const PointsView PV{P.points, P.pstride, P.nch, P.exact};
  uint64_t* MK = R.L + PANN_WAVE;
  gather_tile<DT, METRIC, LPC, NCH1, U>(PV, qreg, qlds, Pl, m, lane,
    [&](bool has, uint32_t ci, uint32_t id, float dist, uint64_t before) {
      const uint32_t ord = f2ord(dist);
      const uint64_t key = ((uint64_t)ord << 32) | id;
      const bool pass = has && (ord < cutoff_ord);
      const uint64_t pm = __ballot(pass);
      if (pass) C[c + (uint32_t)__popcll(pm & before)] = key;
      c += __popcll(pm);
      if (has) MK[ci] = key;
    });
  PANN_WSYNC();
  const bool mine = (note >> 31) != 0u;
  const uint64_t key = mine ? MK[(note >> 5) & 63u] : KEY_INF;
  masked_offer<S>(R, key, mine && mask_verdict<MODE, S>(M, aword, note), thr_lane, lane);
  return c;
}

// The same for the STEER variants, whose gathers hold allowed points only: the m ids of Pl were chosen by their verdict, so every
// key is offered, by the lane of its index in Pl.  masked_offer does the duplicate handling as for any other offer.
template <int DT, int METRIC, int LPC, bool NCH1, int U>
__device__ __forceinline__ uint32_t gather_distances_steered(const BSParams& P, const QReg<DT>& qreg, const uint4* qlds,
                                                             const uint32_t* Pl, uint32_t m, uint32_t cutoff_ord, uint64_t* C,
                                                             uint32_t c, int lane, MaskedList& R, uint32_t thr_lane) {
  const PointsView PV{P.points, P.pstride, P.nch, P.exact};
  uint64_t* MK = R.L + PANN_WAVE;
  gather_tile<DT, METRIC, LPC, NCH1, U>(PV, qreg, qlds, Pl, m, lane,
    [&](bool has, uint32_t ci, uint32_t id, float dist, uint64_t before) {
      const uint32_t ord = f2ord(dist);
      const uint64_t key = ((uint64_t)ord << 32) | id;
      const bool pass = has && (ord < cutoff_ord);
      const uint64_t pm = __ballot(pass);
      if (pass) C[c + (uint32_t)__popcll(pm & before)] = key;
      c += __popcll(pm);
      if (has) MK[ci] = key;
    });
  PANN_WSYNC();
  const bool mine = (uint32_t)lane < m;
  masked_offer<true>(R, mine ? MK[lane] : KEY_INF, mine, thr_lane, lane);
  return c;
}

// Sketch distance of base point `a` to the query sketch SQ (LDS, wave-uniform), as the float the reference's distance()
// returns: Hamming distance (Euclidean_Bit_Point / Mips_Bit_Point; as_written: the reference's loop, which counts block 0
// num_blocks times, euclidian_point.h:360-361, mips_point.h:652-653) or sum of 2 pop(ne & nz) - pop(nz) over the blocks
// (Mips_2Bit_Point::distance_8, mips_point.h:530-543; |total| <= d <= 2048 fits its int16).  The lane reads its candidate's
// row as 16-byte chunks: one for d <= 128 (one-bit) / d <= 64 (2-bit); pad bytes are zero on both sides and add nothing.
__device__ __forceinline__ float sketch_distance(const BSParams& P, const uint4* SQ, uint32_t a) {
  const uint4* __restrict__ row = reinterpret_cast<const uint4*>(P.sketch + (uint64_t)a * P.sk_stride);
  const uint32_t nch = P.sk_stride >> 4;
  int tot = 0;
  if (P.sk_kind == PANN_SKETCH_MIPS_2BIT) {             // a chunk = one block: sign word (x, y), mask word (z, w)
    for (uint32_t j = 0; j < nch; j++) {
      const uint4 p = row[j], q = SQ[j];
      const uint64_t ne = (((uint64_t)(p.y ^ q.y)) << 32) | (p.x ^ q.x);
      const uint64_t nz = (((uint64_t)(p.w & q.w)) << 32) | (p.z & q.z);
      tot += 2 * __popcll(ne & nz) - __popcll(nz);
    }
  } else if (P.sk_as_written) {
    const uint4 p = row[0], q = SQ[0];
    const uint64_t x = (((uint64_t)(p.y ^ q.y)) << 32) | (p.x ^ q.x);
    tot = (int)P.sk_nblk * __popcll(x);
  } else {                                              // a chunk = two blocks
    for (uint32_t j = 0; j < nch; j++) {
      const uint4 p = row[j], q = SQ[j];
      const uint64_t x0 = (((uint64_t)(p.y ^ q.y)) << 32) | (p.x ^ q.x);
      const uint64_t x1 = (((uint64_t)(p.w ^ q.w)) << 32) | (p.z ^ q.z);
      tot += __popcll(x0) + __popcll(x1);
    }
  }
  return (float)tot;
}

// ---- per-query bookkeeping that does not depend on the frontier layout: shared by the three kernels ----
// The callers keep the `lane == 0` tests: with the test inside the helper hipcc schedules the register-frontier kernels
// differently ("Shared per-query helpers").

// Persistent blocks (filter table in HBM, one table per block): the next launch slot from the counter, wave-uniform.  Only
// lane 0's value is read back; `slot` is what the other lanes carry meanwhile.
__device__ __forceinline__ uint32_t next_slot(const BSParams& P, int lane, uint32_t slot = 0) {
  if (lane == 0) slot = atomicAdd(P.work_counter, 1u);
  return __builtin_amdgcn_readfirstlane(slot);
}

// visited.insert(current) (:112-114) as far as the caller sees it: entry nvis of the query's visited list (lane 0, and only when
// a list was asked for: visited_cap != 0).  A full list sets status bit 1.  The frontier's own flag is the kernel's business.
__device__ __forceinline__ void record_visit(const BSParams& P, uint32_t qi, uint32_t nvis, uint64_t cur_key) {
  if (nvis < P.out.visited_cap) {
    if (P.out.visited_ids) P.out.visited_ids[(size_t)qi * P.out.visited_cap + nvis] = key_id(cur_key);
    if (P.out.visited_dists) P.out.visited_dists[(size_t)qi * P.out.visited_cap + nvis] = key_dist(cur_key);
  } else {
    atomicOr(P.status, 1u);
  }
}

// The per-query counters (:211-213), each optional (lane 0).
__device__ __forceinline__ void write_counters(const BSParams& P, uint32_t qi, uint32_t f, uint32_t nvis, uint32_t dcmps, uint32_t degsum) {
  if (P.out.frontier_size) P.out.frontier_size[qi] = f;
  if (P.out.visited_count) P.out.visited_count[qi] = nvis;
  if (P.out.dist_cmps) P.out.dist_cmps[qi] = dcmps;
  if (P.out.degree_sum) P.out.degree_sum[qi] = degsum;
}

// Generic kernel: any beam (frontier in LDS), filter in LDS or in HBM scratch.
// FILTER: filtered_beam_search with use_filtering (beamSearch.h:98-100,117-123,139-146) -- while the frontier is full, a
// neighbour that passed the hash filter gets a full distance only if its sketch distance to the query is below the running
// mean of the sketch distance to the worst frontier entry.  After the hash-filter replay lane i still owns neighbour i: it
// reads its own candidate's sketch, and the ballot compaction that follows hands the gather a dense list in row order.
// MASKED (MASK_BITMAP / MASK_LABELS): the traversal of the plain search; out->ids/dists hold the result list over the allowed
// points (see MaskedList, MaskSrc).
// STEER (masked forms only; DESIGN.md "Steered masked search"): `pruned` of a visit holds allowed points only -- the allowed
// neighbours that passed the hash filter, then the allowed neighbours of the disallowed ones (the bridges, BR in LDS) until `fill`
// entries are there.  The verdict is taken BEFORE the gather, survivors wait in the whole of NF (128 ids) and are gathered 64 at a
// time or when the visit ends; bridge rows are loaded four row chunks at a time, their mask words requested together, and only then
// does the filter replay run, chunk by chunk in order, on the allowed lanes: a row loaded past the `fill` stop is dropped unseen.
template <int DT, int METRIC, int LPC, bool NCH1, bool HASH_LDS, bool FILTER = false, int MASKED = MASK_NONE, bool STEER = false>
__global__ void __launch_bounds__(PANN_WAVE, PANN_MINWAVES) beam_search_kernel(BSParams P) {
  static_assert(!(FILTER && MASKED), "the masked search has no sketch-filtered form");
  static_assert(!STEER || MASKED != MASK_NONE, "steering needs a verdict: masked forms only");
  const int lane = threadIdx.x;
  extern __shared__ __align__(16) uint8_t smem[];   // carved as generic_lds (search_plan.h) lays it out, by typed pointer steps
  // ---- LDS carve (all regions 16 B aligned): 6.4 KB at beam 64 / degree 64 -> 24 queries per CU ----
  uint64_t* F = reinterpret_cast<uint64_t*>(smem);       // [bcap] frontier keys
  uint64_t* NF = F + P.bcap;                             // [bcap] merge output (swapped with F); between
                                                         //        merges its first 256 B hold Pl
  uint64_t* C = NF + P.bcap;                             // [ccap] candidates (unsorted)
  uint8_t* Fv = reinterpret_cast<uint8_t*>(C + P.ccap);  // [bcap] 0 unvisited, 1 visited, 2 visited+listed
  uint8_t* NFv = Fv + P.bcap;                            // [bcap]
  uint16_t* CP = reinterpret_cast<uint16_t*>(NFv + P.bcap);  // [ccap] candidate's lower_bound in F
  uint4* qlds = reinterpret_cast<uint4*>(CP + P.ccap);   // [nch*LPC] query (generic variant)
  uint32_t* Hl = reinterpret_cast<uint32_t*>(qlds + (NCH1 ? 0 : P.nch * LPC));  // [1<<bits] if HASH_LDS, else 1 KB replay scratch
#define PANN_PL (reinterpret_cast<uint32_t*>(NF))        /* [64] filter survivors of one row chunk */

  const uint32_t hsize = 1u << P.bits, hmask = hsize - 1u;
  const uint32_t beam = P.beam;
  const uint32_t BIG_ORD = f2ord(2147483648.0f);  // (distanceType) numeric_limits<int>::max()  (:152)

  uint32_t slot = blockIdx.x;
  if constexpr (!HASH_LDS) slot = next_slot(P, lane);
  while (slot < P.nq) {
    const uint32_t qi = P.order ? P.order[slot] : slot;
    uint32_t* H = HASH_LDS ? Hl : P.hash_global + ((size_t)blockIdx.x << P.bits);
    // ---- filter init: hash_filter(1<<bits, -1) (:53) ----
    for (uint32_t i = lane; i < hsize; i += PANN_WAVE) hstore<HASH_LDS>(H, i, SENTINEL);

    // ---- query vector -> registers (one chunk) or LDS (generic) ----
    const int64_t self = P.query_ids ? (int64_t)P.query_ids[qi] : -1;
    const uint8_t* qrow = P.query_ids ? P.points + (uint64_t)self * P.pstride : P.queries + (uint64_t)qi * P.qstride;
    QReg<DT> qreg{};
    load_query<DT, LPC, NCH1>(qrow, P.dbytes, P.nch, qreg, qlds, lane);
    [[maybe_unused]] const uint4* SQ = reinterpret_cast<const uint4*>(smem + P.sk_lds_off);   // [sk_stride / 16] query sketch
    if constexpr (FILTER) {   // qq: the query's sketch -- its own row of the slab, or an external host-layout row (zero padded)
      uint32_t* sq = reinterpret_cast<uint32_t*>(smem + P.sk_lds_off);
      const uint32_t* srow = reinterpret_cast<const uint32_t*>(P.query_ids ? P.sketch + (uint64_t)self * P.sk_stride
                                                                           : P.sketch_queries + (uint64_t)qi * P.sq_stride);
      const uint32_t valid = (P.query_ids ? P.sk_stride : P.sk_row_bytes) >> 2;
      for (uint32_t w = lane; w < (P.sk_stride >> 2); w += PANN_WAVE) sq[w] = w < valid ? srow[w] : 0u;
    }
    hsync<HASH_LDS>();

    uint32_t f = 0;        // frontier size
    uint32_t c = 0;        // accumulated candidates
    uint32_t nvis = 0;     // num_visited
    uint32_t dcmps = P.nstarts;  // dist_cmps == full_dist_cmps (:83-84)
    uint32_t degsum = 0;
    uint32_t ndrop = 0;    // entries in the dropped list
    [[maybe_unused]] uint32_t pcmps = P.nstarts;   // FILTER: the reference's local dist_cmps (:83,137); dcmps is full_dist_cmps
    [[maybe_unused]] float fsum = 0.0f, fthr = 0.0f;   // FILTER: filter_threshold_sum / filter_threshold (:98-100)
    [[maybe_unused]] uint32_t fcount = 0;
    [[maybe_unused]] uint32_t sbr = 0, shop = 0;       // STEER: bridge rows expanded; entries the two-hop pass appended
    PANN_STAMP_BEGIN();
    uint64_t* DL = P.dropped + (size_t)qi * P.dcap;
    [[maybe_unused]] MaskedList R{reinterpret_cast<uint64_t*>(smem + P.rl_off), P.out.out_k ? KEY_INF : 0ull, 0u};
    [[maybe_unused]] const uint32_t thr_lane = P.out.out_k ? P.out.out_k - 1u : 0u;
    [[maybe_unused]] MaskSrc M{};
    if constexpr (MASKED) { M = mask_src<MASKED, STEER>(P, qi); R.L[lane] = KEY_INF; }

    // ---- start points (:66-70): distance for each, filter insert in order, then "merge" into
    // the empty frontier (which sorts them) ----
    for (uint32_t s0 = 0; s0 < P.nstarts; s0 += PANN_WAVE) {
      const uint32_t i = s0 + lane;
      const bool act = i < P.nstarts;
      const uint32_t a = act ? P.starts[(size_t)qi * P.starts_stride + i] : 0u;
      (void)filter_update<HASH_LDS>(H, hmask, act, a, lane, reinterpret_cast<uint8_t*>(Hl));
      [[maybe_unused]] uint32_t aword = 0u;
      if constexpr (MASKED) if (act) aword = mask_word<MASKED, STEER>(M, a);
      if (act) PANN_PL[lane] = a;
      PANN_WSYNC();
      const uint32_t m = min(P.nstarts - s0, (uint32_t)PANN_WAVE);
      // every start enters the frontier: cutoff above any finite distance
      if constexpr (MASKED)
        c = gather_distances_masked<DT, METRIC, LPC, NCH1, 4, MASKED, STEER>(P, qreg, qlds, PANN_PL, m, 0xFFFFFFFFu, C, c, lane,
                                                              masked_note<STEER>(act, (uint32_t)lane, a), aword, M, R, thr_lane);
      else
      c = gather_distances<DT, METRIC, LPC, NCH1, 4>(P, qreg, qlds, PANN_PL, m, 0xFFFFFFFFu, C, c, lane);
      PANN_WSYNC();
    }

    bool first = true;  // the start-point pseudo-merge: no cut-prune, no visit
    for (;;) {
      bool do_merge = first;
      if (!first) {
        // ---- next vertex: first unvisited frontier entry (:107-109) ----
        int cur_idx = -1;
        uint32_t unv_total = 0;
        for (uint32_t e0 = 0; e0 < f; e0 += PANN_WAVE) {
          const uint32_t e = e0 + lane;
          const uint64_t um = __ballot(e < f && Fv[e] == 0);
          if (cur_idx < 0 && um) cur_idx = (int)e0 + __ffsll((unsigned long long)um) - 1;
          unv_total += __popcll(um);
        }
        if (cur_idx < 0 || nvis >= P.limit) break;
        PANN_STAMP(0);   // head scan
        const uint64_t cur_key = F[cur_idx];
        const uint32_t cur = key_id(cur_key);
        // ---- visited.insert(current) (:112-114) ----
        if (lane == 0) {
          Fv[cur_idx] = 1;
          if (P.out.visited_cap) record_visit(P, qi, nvis, cur_key);
        }
        nvis++;
        const bool more_unvisited = unv_total > 1;         // offset + 1 < remain (:165)
        const bool full = (f == beam);                      // :115
        uint32_t cutoff_ord = BIG_ORD;                      // :150-152
        if (full) cutoff_ord = (uint32_t)(F[f - 1] >> 32);
        if constexpr (FILTER) {
          // ---- running mean of the sketch distance to the worst frontier entry (:119-123): small integers, so the f32 sum is
          // exact; ONE IEEE-rounded division, as the reference's float / int ----
          if (full) {
            fsum += sketch_distance(P, SQ, key_id(F[f - 1]));
            fcount++;
            fthr = __fdiv_rn(fsum, (float)fcount);
          }
        }

        // ---- adjacency row: lane i <- slot i; degree = number of non-sentinel slots ----
        const uint32_t* row = P.graph + (size_t)cur * P.gstride;
        if constexpr (STEER) {
          uint32_t* BR = reinterpret_cast<uint32_t*>(smem + P.br_off);   // [deg_eff] bridges of this visit, in row order
          uint32_t* PQ = PANN_PL;                  // [128] pruned entries waiting for their gather (NF is idle between merges)
          uint32_t npend = 0, npr = 0, nbr = 0;    // waiting in PQ; len(pruned) so far; bridges
          // gather 64 at a time while at least `least` entries wait; what stays moves to the head of PQ
          auto drain = [&](uint32_t least) {
            while (npend != 0u && npend >= least) {
              const uint32_t m = min(npend, (uint32_t)PANN_WAVE), rest = npend - m;      // rest < 64
              c = gather_distances_steered<DT, METRIC, LPC, NCH1, PANN_GU>(P, qreg, qlds, PQ, m, cutoff_ord, C, c, lane, R, thr_lane);
              PANN_WSYNC();
              uint32_t mv = 0u;
              if ((uint32_t)lane < rest) mv = PQ[PANN_WAVE + lane];
              PANN_WSYNC();
              if ((uint32_t)lane < rest) PQ[lane] = mv;
              PANN_WSYNC();
              npend = rest;
            }
          };
          // ---- direct pass: filter replay in row order; allowed survivors -> pruned, the others -> bridges ----
          for (uint32_t i0 = 0; i0 < P.gstride; i0 += PANN_WAVE) {
            const uint32_t i = i0 + lane;
            uint32_t a = SENTINEL;
            if (i < P.gstride) a = row[i];
            const bool act = (a != SENTINEL) && (i < P.degree_limit);   // min(size, degree_limit) (:130)
            const uint64_t am = __ballot(act);
            if (am == 0ull) break;
            degsum += __popcll(am);
            const bool seen = filter_update<HASH_LDS>(H, hmask, act, a, lane, reinterpret_cast<uint8_t*>(Hl));
            const bool keep = act && !seen && ((int64_t)a != self);     // :133
            uint32_t aword = 0u;
            if (keep) aword = mask_word<MASKED, true>(M, a);
            const bool ok = keep && mask_verdict<MASKED, true>(M, aword, a);
            const uint64_t okm = __ballot(ok), brm = __ballot(keep && !ok);
            if (ok) PQ[npend + lanes_below(okm, lane)] = a;
            if (keep && !ok) BR[nbr + lanes_below(brm, lane)] = a;     // nbr <= deg_eff: act holds for the first degree_limit slots only
            npend += __popcll(okm); npr += __popcll(okm); nbr += __popcll(brm);
            PANN_WSYNC();
            drain(PANN_WAVE);
          }
          // ---- two-hop pass: unit t = row chunk t % nchunk of bridge t / nchunk; four units per round trip ----
          const uint32_t nchunk = (P.gstride + PANN_WAVE - 1) / PANN_WAVE, nunits = nbr * nchunk;
          bool stop = false;
          for (uint32_t t0 = 0; t0 < nunits && !stop; t0 += 4) {
            if (t0 % nchunk == 0u && npr >= P.fill) break;             // nothing to speculate on
            uint32_t rc[4], rw[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
              const uint32_t t = t0 + u;
              rc[u] = SENTINEL;
              if (t < nunits) {
                const uint32_t b = BR[t / nchunk], i = (t % nchunk) * PANN_WAVE + lane;
                if (i < P.gstride && i < P.degree_limit) rc[u] = P.graph[(size_t)b * P.gstride + i];
              }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
              rw[u] = 0u;
              if (rc[u] != SENTINEL) rw[u] = mask_word<MASKED, true>(M, rc[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
              const uint32_t t = t0 + u;
              if (t >= nunits) break;
              if (t % nchunk == 0u) {                                  // before touching a bridge: taken whole or not at all
                if (npr >= P.fill) { stop = true; break; }
                sbr++;
              }
              const bool al = rc[u] != SENTINEL && mask_verdict<MASKED, true>(M, rw[u], rc[u]);   // disallowed: the filter is not touched
              if (__ballot(al) == 0ull) continue;
              const bool seen = filter_update<HASH_LDS>(H, hmask, al, rc[u], lane, reinterpret_cast<uint8_t*>(Hl));
              const bool keep = al && !seen && ((int64_t)rc[u] != self);
              const uint64_t km = __ballot(keep);
              if (keep) PQ[npend + lanes_below(km, lane)] = rc[u];
              const uint32_t m = __popcll(km);
              npend += m; npr += m; shop += m;
              PANN_WSYNC();
              drain(PANN_WAVE);
            }
          }
          drain(1u);
          dcmps += npr;                                                // :137,155
        } else
        for (uint32_t i0 = 0; i0 < P.gstride; i0 += PANN_WAVE) {
          const uint32_t i = i0 + lane;
          uint32_t a = SENTINEL;
          if (i < P.gstride) a = row[i];
          const bool act = (a != SENTINEL) && (i < P.degree_limit);   // min(size, degree_limit) (:130)
          const uint64_t am = __ballot(act);
          PANN_STAMP(1);   // adjacency row arrived
          if (am == 0ull) break;
          degsum += __popcll(am);
          const bool seen = filter_update<HASH_LDS>(H, hmask, act, a, lane, reinterpret_cast<uint8_t*>(Hl));
          bool keep = act && !seen && ((int64_t)a != self);           // :133
          if constexpr (FILTER) {
            pcmps += __popcll(__ballot(keep));                        // dist_cmps += pruned.size() (:137)
            if (full && keep) keep = !(sketch_distance(P, SQ, a) >= fthr);   // :140-145; not full: everything passes (:146)
          }
          const uint64_t km = __ballot(keep);
          const uint32_t m = __popcll(km);
          [[maybe_unused]] uint32_t aword = 0u;
          if constexpr (MASKED) if (keep) aword = mask_word<MASKED>(M, a);         // in flight with the rows of the gather
          const uint32_t mypos = lanes_below(km, lane);
          if (keep) PANN_PL[mypos] = a;
          dcmps += m;                                                 // :137,155
          PANN_WSYNC();
          PANN_STAMP(2);   // filter + compaction
          if constexpr (MASKED) {
            if (m) c = gather_distances_masked<DT, METRIC, LPC, NCH1, PANN_GU, MASKED>(P, qreg, qlds, PANN_PL, m, cutoff_ord, C, c, lane,
                                                                               masked_note(keep, mypos, a), aword, M, R, thr_lane);
          } else {
          if (m) c = gather_distances<DT, METRIC, LPC, NCH1, PANN_GU>(P, qreg, qlds, PANN_PL, m, cutoff_ord, C, c, lane);
          }
          PANN_WSYNC();
          PANN_STAMP(3);   // gather + distances
        }
        // ---- skip the merge while too few candidates (:162-168) ----
        PANN_WSYNC();
        const bool skip = (c == 0) || (P.skip_enabled && c < beam / 8 && more_unvisited);
        do_merge = !skip;
      }
      if (do_merge) {
        {
          // ================= merge: sort+unique(C), set_union with F, trim (:173-185) =========
          // A1: kill duplicates (same id <=> same key) and entries already in F; remember rank in F
          for (uint32_t j0 = 0; j0 < c; j0 += PANN_WAVE) {
            const uint32_t j = j0 + lane;
            uint64_t key = KEY_INF;
            uint32_t p = 0;
            if (j < c) {
              key = C[j];
              bool dead = false;
              for (uint32_t i = 0; i < j; i++) dead |= (C[i] == key);
              p = lower_bound_lds(F, f, key);
              dead |= (p < f && F[p] == key);
              if (dead) key = KEY_INF;
            }
            PANN_WSYNC();       // all reads of C[0..j) by this chunk are done
            if (j < c) { C[j] = key; CP[j] = (uint16_t)p; }
            // later chunks compare against earlier ORIGINAL keys; a killed earlier key was itself a
            // duplicate of a still earlier live one (or of F), so the verdict is unchanged.
            PANN_WSYNC();
          }
          // A2: rank among live candidates -> direct placement into NF
          uint32_t nvalid = 0;
          for (uint32_t j0 = 0; j0 < c; j0 += PANN_WAVE) {
            const uint32_t j = j0 + lane;
            const uint64_t key = j < c ? C[j] : KEY_INF;
            nvalid += __popcll(__ballot(key != KEY_INF));
            if (key != KEY_INF) {
              uint32_t r = 0;
              for (uint32_t i = 0; i < c; i++) r += (C[i] < key) ? 1u : 0u;   // dead entries are KEY_INF
              const uint32_t pos = r + CP[j];
              if (pos < beam) {
                uint32_t flag = 0u;   // re-entry of an already visited vertex? (only while not full)
                for (uint32_t t = 0; t < ndrop; t++)
                  flag |= (__hip_atomic_load(DL + t, __ATOMIC_RELAXED, PANN_PRIVATE_SCOPE) == key) ? 2u : 0u;
                NF[pos] = key; NFv[pos] = (uint8_t)flag;
              }
            }
          }
          // B: old frontier entries move right by the number of live candidates below them
          for (uint32_t e0 = 0; e0 < f; e0 += PANN_WAVE) {
            const uint32_t e = e0 + lane;
            if (e < f) {
              const uint64_t key = F[e];
              uint32_t below = 0;
              for (uint32_t i = 0; i < c; i++) below += (C[i] < key) ? 1u : 0u;
              const uint32_t pos = e + below;
              if (pos < beam) { NF[pos] = key; NFv[pos] = Fv[e]; }
            }
          }
          PANN_WSYNC();
          const uint32_t f_old = f;
          uint32_t f_new = min(f_old + nvalid, beam);   // :185
          // ---- cut-prune (:190-195) ----
          if (!first && P.cut_enabled && f_new > P.k) {
            const float dk = key_dist(NF[P.k]);
            const float thr = (float)(P.cut * (double)dk);
            const uint64_t thr_key = (uint64_t)f2ord(thr) << 32;   // pair{0, thr}: kept iff key <= thr_key
            uint32_t ub = 0;
            for (uint32_t e0 = 0; e0 < f_new; e0 += PANN_WAVE) {
              const uint32_t e = e0 + lane;
              ub += __popcll(__ballot(e < f_new && NF[e] <= thr_key));
            }
            f_new = max(ub, f_old);
          }
          // ---- visited entries that fall off a frontier that is still not full can come back:
          // remember them (see file header).  Once full, nothing dropped can ever re-enter. ----
          if (f_new == beam) {
            ndrop = 0;
          } else if (P.cut_enabled && !first) {
            for (uint32_t e0 = 0; e0 < f_old; e0 += PANN_WAVE) {
              const uint32_t e = e0 + lane;
              bool lost = false;
              uint64_t key = 0;
              if (e < f_old && Fv[e] == 1) {
                key = F[e];
                uint32_t below = 0;
                for (uint32_t i = 0; i < c; i++) below += (C[i] < key) ? 1u : 0u;
                lost = (e + below) >= f_new;
              }
              const uint64_t lm = __ballot(lost);
              if (lost) {
                const uint32_t at = ndrop + lanes_below(lm, lane);
                if (at < P.dcap) DL[at] = key; else atomicOr(P.status, 2u);
              }
              ndrop = min(ndrop + (uint32_t)__popcll(lm), P.dcap);
            }
            // entries already listed (flag 2) stay listed; nothing to do for them
            __builtin_amdgcn_s_waitcnt(0);   // dropped-list stores visible to this wave's later loads
          }
          // visited entries with flag 2 that stay in the frontier keep flag 2 (== visited)
          { uint64_t* t = F; F = NF; NF = t; uint8_t* tv = Fv; Fv = NFv; NFv = tv; }
          f = f_new;
          c = 0;                      // candidates.clear() (:182)
          PANN_WSYNC();
        }
      }
      PANN_STAMP(4);     // merge (or nothing when skipped)
      first = false;
    }

    // ---- outputs (:211-213; searchAll takes the first k ids :378-380) ----
    const size_t qo = (size_t)qi * P.out.out_k;
    if constexpr (MASKED) {                                        // out_k <= 64: the result list, not the head of the frontier
      const uint64_t rkey = R.L[lane];
      const uint64_t fill = __ballot(rkey != KEY_INF);
      if (lane < (int)P.out.out_k) {
        const bool ok = rkey != KEY_INF;
        if (P.out.ids) P.out.ids[qo + lane] = ok ? key_id(rkey) : SENTINEL;
        if (P.out.dists) P.out.dists[qo + lane] = ok ? key_dist(rkey) : __builtin_inff();
      }
      if (lane == 0) {
        if (P.result_count) P.result_count[qi] = min((uint32_t)__popcll(fill), P.out.out_k);
        if (P.allowed_cmps) P.allowed_cmps[qi] = R.cmps;
      }
    } else {
    for (uint32_t j = lane; j < P.out.out_k; j += PANN_WAVE) {
      const bool ok = j < f;
      uint64_t key = 0ull;
      if (ok) key = F[j];
      if (P.out.ids) P.out.ids[qo + j] = ok ? key_id(key) : SENTINEL;
      if (P.out.dists) P.out.dists[qo + j] = ok ? key_dist(key) : __builtin_inff();
    }
    }
    PANN_STAMP_FLUSH(qi);
    if (lane == 0) {
      write_counters(P, qi, f, nvis, dcmps, degsum);
      if constexpr (FILTER) if (P.pruned_cmps) P.pruned_cmps[qi] = pcmps;
      if constexpr (STEER) if (P.steer_out) { P.steer_out[(size_t)qi * 2] = sbr; P.steer_out[(size_t)qi * 2 + 1] = shop; }
    }
    PANN_WSYNC();
    if constexpr (HASH_LDS) break;
    else slot = next_slot(P, lane);
  }
}

// =============================================================================================
// beam <= 64 specialisation: the frontier lives in REGISTERS (lane e <-> entry e: key + visited
// flag).  Head scan = one ballot, cutoff = one readlane, every merge = loops of readlane/ballot
// steps over <= 64 candidates at a time (top-beam of a union is associative, so candidate chunks
// are merged one after the other; cut-prune runs once at the end).  LDS per query shrinks to the
// filter (4 KB) + a 64-entry scatter scratch + the candidate list: 5.2 KB -> 31 queries per CU.
// =============================================================================================
// MASKED: as in the generic kernel.
// MODE: MASK_NONE, a masked form, or B64_SEEN: the plain search with the second-sighting table V ("Second
// sightings"), whose size is the compile-time constant VN (0: no table, the kernel as it was before V).
enum { B64_SEEN = 3 };
template <int DT, int METRIC, int LPC, bool NCH1, int MODE = MASK_NONE>
__global__ void __launch_bounds__(PANN_WAVE, PANN_MINWAVES_B64) beam_search_b64_kernel(BSParams P) {
  constexpr int MASKED = (MODE == MASK_BITMAP || MODE == MASK_LABELS) ? MODE : MASK_NONE;
  constexpr int VN = MODE == B64_SEEN ? (int)B64_SEEN_N : 0;
  static_assert((B64_SEEN_N & (B64_SEEN_N - 1)) == 0 && B64_SEEN_N >= 128, "V: a power of two of whole words per lane");
  const int lane = threadIdx.x;
  extern __shared__ __align__(16) uint8_t smem[];   // carved as b64_lds (search_plan.h) lays it out, by typed pointer steps
  uint64_t* S = reinterpret_cast<uint64_t*>(smem);          // [64] merge scatter scratch; first 256 B double as Pl
  uint64_t* C = S + 64;                                     // [ccap] candidates (unsorted)
  uint8_t* Sv = reinterpret_cast<uint8_t*>(C + P.ccap);     // [64] flags of the scatter scratch
  uint4* qlds = reinterpret_cast<uint4*>(Sv + 64);          // [nch*LPC] query (generic variant)
  uint32_t* H = reinterpret_cast<uint32_t*>(qlds + (NCH1 ? 0 : P.nch * LPC));  // [1<<bits]
  uint32_t* Pl = reinterpret_cast<uint32_t*>(S);            // [64] filter survivors of one row chunk

  const uint32_t hsize = 1u << P.bits, hmask = hsize - 1u;
  const uint32_t beam = P.beam;
  const uint32_t BIG_ORD = f2ord(2147483648.0f);            // (:152)
  // V[VN]: entry id & (VN - 1) holds the tag id >> log2(VN) of an id that H has forgotten (0xFFFF: empty; make_plan keeps every
  // tag below it).  An id found here was compared by this query before; an id not found may have been, too.
  constexpr uint32_t VSHIFT = VN ? (uint32_t)__builtin_ctz((unsigned)(VN ? VN : 1)) : 0u;
  [[maybe_unused]] uint16_t* V = reinterpret_cast<uint16_t*>(H + hsize);
  [[maybe_unused]] bool v_ok = true;                        // no cut-prune has left the frontier at or below k entries
  if constexpr (VN != 0) for (uint32_t i = lane; i < VN / 2; i += PANN_WAVE) reinterpret_cast<uint32_t*>(V)[i] = 0xFFFFFFFFu;
  const uint32_t qi = P.order ? P.order[blockIdx.x] : blockIdx.x;
  // Blocks are dispatched in index order, so the highest indices start last and form the tail of the launch: they
  // get instruction-issue priority over the queries that are already under way (measured +1..3 % at 10K queries,
  // inside the box-to-box noise but never negative).
  if (blockIdx.x >= P.prio_start) __builtin_amdgcn_s_setprio(3);

  for (uint32_t i = lane; i < hsize; i += PANN_WAVE) H[i] = SENTINEL;       // :53
  const int64_t self = P.query_ids ? (int64_t)P.query_ids[qi] : -1;
  const uint8_t* qrow = P.query_ids ? P.points + (uint64_t)self * P.pstride : P.queries + (uint64_t)qi * P.qstride;
  QReg<DT> qreg{};
  load_query<DT, LPC, NCH1>(qrow, P.dbytes, P.nch, qreg, qlds, lane);
  PANN_WSYNC();

  uint32_t f = 0, c = 0, nvis = 0, dcmps = P.nstarts, degsum = 0, ndrop = 0;
  uint64_t fkey = KEY_INF;
  uint32_t fflag = 0;
  uint64_t* DL = P.dropped + (size_t)qi * P.dcap;
  [[maybe_unused]] MaskedList R{reinterpret_cast<uint64_t*>(smem + P.rl_off), P.out.out_k ? KEY_INF : 0ull, 0u};
  [[maybe_unused]] const uint32_t thr_lane = P.out.out_k ? P.out.out_k - 1u : 0u;
  [[maybe_unused]] MaskSrc M{};
  if constexpr (MASKED) { M = mask_src<MASKED>(P, qi); R.L[lane] = KEY_INF; }
  PANN_STAMP_BEGIN();

  // ---- start points (:66-70); nstarts <= 64 here ----
  {
    const bool act = lane < (int)P.nstarts;
    const uint32_t a = act ? P.starts[(size_t)qi * P.starts_stride + lane] : 0u;
    (void)filter_update<true>(H, hmask, act, a, lane);
    [[maybe_unused]] uint32_t aword = 0u;
    if constexpr (MASKED) if (act) aword = mask_word<MASKED>(M, a);
    if (act) Pl[lane] = a;
    PANN_WSYNC();
    if constexpr (MASKED)
      c = gather_distances_masked<DT, METRIC, LPC, NCH1, 4, MASKED>(P, qreg, qlds, Pl, P.nstarts, 0xFFFFFFFFu, C, c, lane,
                                                            masked_note(act, (uint32_t)lane, a), aword, M, R, thr_lane);
    else
    c = gather_distances<DT, METRIC, LPC, NCH1, 4>(P, qreg, qlds, Pl, P.nstarts, 0xFFFFFFFFu, C, c, lane);
    PANN_WSYNC();
  }

  uint32_t pref_id = SENTINEL, pref_row = SENTINEL;            // speculative row fetch (see the loop)
  bool first = true;
  for (;;) {
    bool do_merge = first;
    if (!first) {
      // ---- next vertex: first unvisited frontier entry (:107-109) ----
      const uint64_t um = __ballot(lane < (int)f && fflag == 0);
      if (um == 0ull || nvis >= P.limit) break;
      const int cur_idx = __ffsll((unsigned long long)um) - 1;
      const bool more_unvisited = (um & (um - 1)) != 0ull;       // offset + 1 < remain (:165)
      PANN_STAMP(0);
      const uint64_t cur_key = readlane64(fkey, cur_idx);
      const uint32_t cur = key_id(cur_key);
      if (lane == cur_idx) fflag = 1;                            // visited.insert(current) (:112-114)
      if (lane == 0 && P.out.visited_cap) record_visit(P, qi, nvis, cur_key);
      nvis++;
      uint32_t cutoff_ord = BIG_ORD;                             // :150-152
      if (f == beam) cutoff_ord = (uint32_t)(readlane64(fkey, (int)f - 1) >> 32);

      // Speculative adjacency-row fetch: the frontier's NEXT unvisited entry is the next vertex unless this iteration's
      // merge puts something in front of it (hit rate ~80 %), so its row is requested now, a whole iteration ahead -- one
      // dependent memory round trip less per iteration, which is what a query costs once the chip is no longer full (the
      // tail of a 10K-query launch).  The load is issued by hand (asm): hipcc drains vmcnt(0) at loop headers, which made a
      // compiler-visible prefetch wait at once (round 1: -2..-8 %).  An unknown older load only makes the compiler's
      // counted waits wait for more, never less; the register is drained (vmcnt(0), free by then) before it is reused.
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(pref_row));
      const bool pref_hit = PANN_B64_PREFETCH && (pref_id == cur);
      const uint32_t pref_val = pref_row;
      pref_id = SENTINEL;
      if (PANN_B64_PREFETCH) {
        const uint64_t rest = um & (um - 1);                       // the entry after the one visited now
        if (rest) {
          pref_id = key_id(readlane64(fkey, __ffsll((unsigned long long)rest) - 1));
          const uint32_t* np = P.graph + (size_t)pref_id * P.gstride + min((uint32_t)lane, P.gstride - 1);
          asm volatile("global_load_dword %0, %1, off" : "=v"(pref_row) : "v"(np));
        }
      }

      const uint32_t* row = P.graph + (size_t)cur * P.gstride;
      for (uint32_t i0 = 0; i0 < P.gstride; i0 += PANN_WAVE) {
        const uint32_t i = i0 + lane;
        uint32_t a = SENTINEL;
        if (i0 == 0 && pref_hit) { if (i < P.gstride) a = pref_val; }
        else if (i < P.gstride) a = row[i];
        const bool act = (a != SENTINEL) && (i < P.degree_limit);
        const uint64_t am = __ballot(act);
        PANN_STAMP(1);
        if (am == 0ull) break;
        degsum += __popcll(am);
        [[maybe_unused]] uint32_t victim = SENTINEL;
        bool seen;
        if constexpr (VN != 0) seen = filter_update<true>(H, hmask, act, a, lane, nullptr, 0, LdsPart{nullptr, 0, 0}, &victim);
        else seen = filter_update<true>(H, hmask, act, a, lane);
        bool keep = act && !seen && ((int64_t)a != self);         // :133
        if constexpr (VN != 0) {
          dcmps += __popcll(__ballot(keep));                      // :137,155 -- a comparison, whether or not its row is fetched
          // Second sightings.  The frontier is full and no cut-prune ever left it at or below k entries, so a vertex this query
          // compared before and that is neither in the frontier nor pending in C lies at or beyond the cutoff:
          // its row is not fetched.  One in the frontier or in C gets the key it has there -- the key the fetch would produce.
          // Pending candidates are looked at through one register per lane, hence c <= 64 (always, for rows of <= 64 slots).
          if (f == beam && v_ok && cutoff_ord <= BIG_ORD && c <= PANN_WAVE) {
            const bool hit = keep && V[a & (VN - 1)] == (uint16_t)(a >> VSHIFT);
            uint64_t hm = __ballot(hit);
            if (hm) {
              const uint64_t pkey = lane < (int)c ? C[lane] : KEY_INF;      // the id of KEY_INF (free lanes, too) is no vertex
              const uint32_t fid = (uint32_t)fkey, pid = (uint32_t)pkey;
              while (hm) {                                        // uniform: one trip per second sighting
                const int l = __ffsll((unsigned long long)hm) - 1;
                hm &= hm - 1;
                const uint32_t al = __builtin_amdgcn_readlane(a, l);
                const uint64_t inf = __ballot(fid == al), inc = __ballot(pid == al);
                uint64_t key = KEY_INF;
                if (inf) key = readlane64(fkey, __ffsll((unsigned long long)inf) - 1);
                else if (inc) key = readlane64(pkey, __ffsll((unsigned long long)inc) - 1);
                if ((uint32_t)(key >> 32) < cutoff_ord) {          // :157
                  if (lane == 0) C[c] = key;
                  c++;
                }
              }
              keep = keep && !hit;
            }
          }
          if (victim != SENTINEL) V[victim & (VN - 1)] = (uint16_t)(victim >> VSHIFT);
        }
        const uint64_t km = __ballot(keep);
        const uint32_t m = __popcll(km);
        [[maybe_unused]] uint32_t aword = 0u;
        if constexpr (MASKED) if (keep) aword = mask_word<MASKED>(M, a);         // in flight with the rows of the gather
        const uint32_t mypos = lanes_below(km, lane);
        if (keep) Pl[mypos] = a;
        if constexpr (VN == 0) dcmps += m;
        PANN_WSYNC();
        PANN_STAMP(2);
        if constexpr (MASKED) {
          if (m) c = gather_distances_masked<DT, METRIC, LPC, NCH1, PANN_GU, MASKED>(P, qreg, qlds, Pl, m, cutoff_ord, C, c, lane,
                                                                             masked_note(keep, mypos, a), aword, M, R, thr_lane);
        } else {
        if (m) c = gather_distances<DT, METRIC, LPC, NCH1, PANN_GU>(P, qreg, qlds, Pl, m, cutoff_ord, C, c, lane);
        }
        PANN_WSYNC();
        PANN_STAMP(3);
      }
      const bool skip = (c == 0) || (P.skip_enabled && c < beam / 8 && more_unvisited);   // :162-168
      do_merge = !skip;
    }
    if (do_merge) {
      const uint32_t f_old = f;
      const bool track = P.cut_enabled && !first;
      uint32_t lt = 0;                                           // tentative appends to the dropped list
      for (uint32_t c0 = 0; c0 < c; c0 += PANN_WAVE) {           // sort+unique(C) U frontier, trimmed (:173-185)
        const uint32_t cc = min(c - c0, (uint32_t)PANN_WAVE);
        const uint64_t ckey = (lane < (int)cc) ? C[c0 + lane] : KEY_INF;
        const bool fl = lane < (int)f;
        uint32_t myp = 0, rank_c = 0, below_f = 0;
        uint64_t live_mask = 0;
        // 64-bit compares issue at 2.5 x the cost of 32-bit ones on gfx950 (tools/valu_rate.hip), so the loop makes two of them
        // per candidate instead of five: equal keys <=> equal ids (a vertex's distance to this query is one deterministic
        // value, whichever row offered it), and "frontier entry below the candidate" is the complement of "candidate below the
        // entry" once no entry is equal (free lanes hold KEY_INF: above every candidate, masked out by vmask).
        const uint64_t vmask = __ballot(fl);
        const uint32_t cid = (uint32_t)ckey, fid = (uint32_t)fkey;
        for (uint32_t i = 0; i < cc; i++) {
          const uint64_t kk = readlane64(ckey, (int)i);
          const uint32_t kid = (uint32_t)kk;
          const bool g = kk < fkey;
          const uint64_t gtm = __ballot(g);
          const uint64_t eqm = __ballot(fid == kid);                     // already in the frontier (set_union)
          const uint64_t dupm = __ballot(cid == kid) & ((1ull << i) - 1ull);   // duplicate (std::unique)
          if (eqm == 0ull && dupm == 0ull) {
            live_mask |= 1ull << i;
            if (lane == (int)i) myp = f - (uint32_t)__popcll(gtm & vmask);
            rank_c += (kk < ckey) ? 1u : 0u;
            below_f += g ? 1u : 0u;
          }
        }
        const uint32_t nvalid = __popcll(live_mask);
        const bool clive = (lane < (int)cc) && ((live_mask >> lane) & 1ull);
        const uint32_t cpos = rank_c + myp, fpos = (uint32_t)lane + below_f;
        if (clive && cpos < beam) {
          uint32_t flag = 0u;   // re-entry of an already visited vertex (only while the frontier is not full)
          for (uint32_t t = 0; t < ndrop; t++)
            flag |= (__hip_atomic_load(DL + t, __ATOMIC_RELAXED, PANN_PRIVATE_SCOPE) == ckey) ? 2u : 0u;
          S[cpos] = ckey; Sv[cpos] = (uint8_t)flag;
        }
        if (fl && fpos < beam) { S[fpos] = fkey; Sv[fpos] = (uint8_t)fflag; }
        if (track) {            // visited entries pushed past the beam by this chunk
          const bool lost = fl && fflag == 1u && fpos >= beam;
          const uint64_t lm = __ballot(lost);
          if (lost) {
            const uint32_t at = ndrop + lt + lanes_below(lm, lane);
            if (at < P.dcap) DL[at] = fkey; else atomicOr(P.status, 2u);
          }
          lt += __popcll(lm);
        }
        PANN_WSYNC();
        f = min(f + nvalid, beam);
        fkey = (lane < (int)f) ? S[lane] : KEY_INF;
        fflag = (lane < (int)f) ? (uint32_t)Sv[lane] : 0u;
        PANN_WSYNC();
      }
      uint32_t f_new = f;
      if (!first && P.cut_enabled && f_new > P.k) {              // cut-prune (:190-195)
        const float dk = key_dist(readlane64(fkey, (int)P.k));
        const float thr = (float)(P.cut * (double)dk);
        const uint64_t thr_key = (uint64_t)f2ord(thr) << 32;     // pair{0, thr}: kept iff key <= thr_key
        const uint32_t ub = __popcll(__ballot(lane < (int)f_new && fkey <= thr_key));
        f_new = max(ub, f_old);
        if constexpr (VN != 0) if (f_new <= P.k) v_ok = false;    // entry k is gone: the next threshold may be a higher one
      }
      if (f_new == beam) {
        ndrop = 0;                                               // a full frontier never re-admits anything
      } else if (track) {
        const bool lost = lane >= (int)f_new && lane < (int)f && fflag == 1u;
        const uint64_t lm = __ballot(lost);
        if (lost) {
          const uint32_t at = ndrop + lt + lanes_below(lm, lane);
          if (at < P.dcap) DL[at] = fkey; else atomicOr(P.status, 2u);
        }
        lt += __popcll(lm);
        ndrop = min(ndrop + lt, P.dcap);
        if (lt) __builtin_amdgcn_s_waitcnt(0);
      }
      f = f_new;
      if (lane >= (int)f) { fkey = KEY_INF; fflag = 0u; }
      c = 0;                                                     // candidates.clear() (:182)
    }
    PANN_STAMP(4);
    first = false;
  }
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(pref_row));          // no speculative load may outlive its register

  const size_t qo = (size_t)qi * P.out.out_k;
  if constexpr (MASKED) {                                        // the result list, not the head of the frontier
    const uint64_t rkey = R.L[lane];
    const uint64_t fill = __ballot(rkey != KEY_INF);
    if (lane < (int)P.out.out_k) {
      const bool ok = rkey != KEY_INF;
      if (P.out.ids) P.out.ids[qo + lane] = ok ? key_id(rkey) : SENTINEL;
      if (P.out.dists) P.out.dists[qo + lane] = ok ? key_dist(rkey) : __builtin_inff();
    }
    if (lane == 0) {
      if (P.result_count) P.result_count[qi] = min((uint32_t)__popcll(fill), P.out.out_k);
      if (P.allowed_cmps) P.allowed_cmps[qi] = R.cmps;
    }
  } else
  if (lane < (int)P.out.out_k) {                                 // out_k <= beam <= 64
    const bool ok = lane < (int)f;
    if (P.out.ids) P.out.ids[qo + lane] = ok ? key_id(fkey) : SENTINEL;
    if (P.out.dists) P.out.dists[qo + lane] = ok ? key_dist(fkey) : __builtin_inff();
  }
  PANN_STAMP_FLUSH(qi);
  if (lane == 0) write_counters(P, qi, f, nvis, dcmps, degsum);
}

// =============================================================================================
// 64 < beam <= 128 (the builder's L = 128): the same register-resident frontier with TWO entries
// per lane (entry e lives in lane e % 64, slot e / 64).  LDS per query: the 16 KB filter + a 128-entry
// scatter scratch + candidates = 18.2 KB -> 9 queries per CU (the LDS-frontier kernel needs 19.9 KB).
// =============================================================================================
// CODES (with HASH_LDS): the whole filter in LDS as 12-bit class codes (filter_update_codes), the codes of a row's neighbours
// read with the row from P.gcode -- the builder's searches when the index keeps the codes (filter_codes.hip).
template <int DT, int METRIC, int LPC, bool NCH1, bool HASH_LDS, bool CODES = false>
__global__ void __launch_bounds__(PANN_WAVE) beam_search_b128_kernel(BSParams P) {
  static_assert(!CODES || HASH_LDS, "the code table lives in LDS");
  constexpr int RB = 2;
  const int lane = threadIdx.x;
  extern __shared__ __align__(16) uint8_t smem[];   // carved as b128_lds (search_plan.h) lays it out, by typed pointer steps
  uint64_t* S = reinterpret_cast<uint64_t*>(smem);          // [128] merge scatter scratch; first 256 B double as Pl
  uint64_t* C = S + 64 * RB;                                // [ccap] candidates (unsorted)
  uint8_t* Sv = reinterpret_cast<uint8_t*>(C + P.ccap);     // [128] flags of the scatter scratch
  uint4* qlds = reinterpret_cast<uint4*>(Sv + 64 * RB);     // [nch*LPC] query (generic variant)
  uint32_t* Hl = reinterpret_cast<uint32_t*>(qlds + (NCH1 ? 0 : P.nch * LPC));  // [1<<bits] if HASH_LDS, else the LDS part of a split table
  uint8_t* T = reinterpret_cast<uint8_t*>(S);               // 1 KB replay scratch of the HBM-table filter: S is idle outside the merge
  uint32_t* Pl = reinterpret_cast<uint32_t*>(S);

  const uint32_t hsize = 1u << P.bits, hmask = hsize - 1u;
  const uint32_t beam = P.beam;
  const uint32_t BIG_ORD = f2ord(2147483648.0f);
  const LdsPart Lp{reinterpret_cast<uint8_t*>(Hl), HASH_LDS ? 0u : (P.hsplit == 3 ? hsize : P.hsplit ? hsize - (hsize >> P.hsplit) : 0u), P.p24};
  // filter in LDS: one query per block.  Filter in HBM (16 KB of LDS would cap a CU at 8 queries): persistent
  // blocks, one table per block, queries pulled from a counter.
  uint32_t slot = blockIdx.x;
  if constexpr (!HASH_LDS) slot = next_slot(P, lane);
  while (slot < P.nq) {
  const uint32_t qi = P.order ? P.order[slot] : slot;
  uint32_t* H = HASH_LDS ? Hl : P.hash_global + ((size_t)blockIdx.x << P.bits);
  const uint32_t hb = HASH_LDS ? 0u : P.hsplit;
  uint8_t* const P8 = reinterpret_cast<uint8_t*>(Hl);                    // CODES: 8-bit plane [hsize], then
  uint32_t* const P4 = Hl + (hsize >> 2);                            // ... the 4-bit plane, 8 slots per dword [hsize / 8]
  if constexpr (CODES) {
    for (uint32_t i = lane; i < (hsize >> 2) + (hsize >> 3); i += PANN_WAVE) Hl[i] = 0xFFFFFFFFu;
  } else {
    if (hb != 3) for (uint32_t i = lane; i < (hsize >> hb); i += PANN_WAVE) hstore<HASH_LDS>(H, i, SENTINEL);
    if (hb) lds_part_clear(Lp, lane);
  }
  const int64_t self = P.query_ids ? (int64_t)P.query_ids[qi] : -1;
  const uint8_t* qrow = P.query_ids ? P.points + (uint64_t)self * P.pstride : P.queries + (uint64_t)qi * P.qstride;
  QReg<DT> qreg{};
  load_query<DT, LPC, NCH1>(qrow, P.dbytes, P.nch, qreg, qlds, lane);
  hsync<HASH_LDS>();

  uint32_t f = 0, c = 0, nvis = 0, dcmps = P.nstarts, degsum = 0, ndrop = 0;
  uint64_t fkey[RB] = {KEY_INF, KEY_INF};
  uint32_t fflag[RB] = {0, 0};
  uint64_t* DL = P.dropped + (size_t)qi * P.dcap;
  PANN_STAMP_BEGIN();
  auto entry_key = [&](uint32_t e) -> uint64_t {            // uniform e
    return (e < 64) ? readlane64(fkey[0], (int)e) : readlane64(fkey[1], (int)e - 64);
  };

  {   // start points (:66-70); nstarts <= 64 in this kernel
    const bool act = lane < (int)P.nstarts;
    const uint32_t a = act ? P.starts[(size_t)qi * P.starts_stride + lane] : 0u;
    if constexpr (CODES) (void)filter_update_codes(P8, P4, hmask, act, a, act ? (uint32_t)P.rank16[a] : 0u, lane, T);
    else (void)filter_update<HASH_LDS>(H, hmask, act, a, lane, T, hb, Lp);
    if (act) Pl[lane] = a;
    PANN_WSYNC();
    c = gather_distances<DT, METRIC, LPC, NCH1, 4, false>(P, qreg, qlds, Pl, P.nstarts, 0xFFFFFFFFu, C, c, lane);
    PANN_WSYNC();
  }

  // Speculative adjacency-row fetch: while the candidates of vertex v are gathered, the row of the frontier's NEXT
  // unvisited entry is already requested; it is the next vertex unless the merge puts something in front of it.
  uint32_t pref_id = SENTINEL, pref_row = SENTINEL, pref_code = 0;
  bool first = true;
  for (;;) {
    bool do_merge = first;
    if (!first) {
      const uint64_t um0 = __ballot(lane < (int)f && fflag[0] == 0);
      const uint64_t um1 = __ballot(lane + 64 < (int)f && fflag[1] == 0);
      if ((um0 | um1) == 0ull || nvis >= P.limit) break;
      const int cur_idx = um0 ? __ffsll((unsigned long long)um0) - 1 : 64 + __ffsll((unsigned long long)um1) - 1;
      const bool more_unvisited = (__popcll(um0) + __popcll(um1)) > 1;          // offset + 1 < remain (:165)
      PANN_STAMP(0);
      const uint64_t cur_key = entry_key((uint32_t)cur_idx);
      const uint32_t cur = key_id(cur_key);
      // ---- two vertices per memory round trip.  While merges are being skipped (:162-168: fewer than beam/8 candidates
      // and another unvisited entry) the frontier and the cutoff do not change, so the vertex after `cur` is already known:
      // the second unvisited entry.  83 % of the builder's iterations skip (66 % of beam-64 queries), so both adjacency
      // rows are fetched together, the filter is replayed row after row (row 2 sees row 1's updates, as in the
      // sequential loop) and ONE gather fetches the survivors of both -- twice the bytes in flight per wave in the phase
      // that is 52 % of this kernel's time.  If the candidates of row 1 alone end the skipping (or row 2 does not fit),
      // row 2 never happened: its candidates are cut off the list and its table writes are put back (FilterUndo).
      // Only with the filter of class codes (PANN_B128_PAIR_CODES): the id table, in LDS or HBM, measured slower with it.
      bool pair = false;
      if constexpr (CODES) pair = PANN_B128_PAIR_CODES && P.skip_enabled && more_unvisited && P.gstride <= PANN_WAVE && nvis + 1 < P.limit;
      if (pair) {
        uint64_t r0 = um0, r1 = um1;
        if (r0) r0 &= r0 - 1; else r1 &= r1 - 1;
        const int idx2 = r0 ? __ffsll((unsigned long long)r0) - 1 : 64 + __ffsll((unsigned long long)r1) - 1;
        if (r0) r0 &= r0 - 1; else r1 &= r1 - 1;
        const bool more_after2 = (r0 | r1) != 0ull;
        const uint64_t key2 = entry_key((uint32_t)idx2);
        const uint32_t cur2 = key_id(key2);
        uint32_t cutoff2 = BIG_ORD;
        if (f == beam) cutoff2 = (uint32_t)(entry_key(f - 1) >> 32);
        uint32_t a1 = SENTINEL, a2 = SENTINEL, code1 = 0, code2 = 0;
        if (lane < (int)P.gstride) {
          a1 = (pref_id == cur) ? pref_row : P.graph[(size_t)cur * P.gstride + lane];
          a2 = P.graph[(size_t)cur2 * P.gstride + lane];
          code1 = (pref_id == cur) ? pref_code : (uint32_t)P.gcode[(size_t)cur * P.gstride + lane];
          code2 = P.gcode[(size_t)cur2 * P.gstride + lane];
        }
        pref_id = SENTINEL;
        const bool act1 = (a1 != SENTINEL) && ((uint32_t)lane < P.degree_limit);
        const bool act2 = (a2 != SENTINEL) && ((uint32_t)lane < P.degree_limit);
        FilterUndo u2;
        const bool seen1 = filter_update_codes(P8, P4, hmask, act1, a1, code1, lane, T);
        const bool seen2 = filter_update_codes(P8, P4, hmask, act2, a2, code2, lane, T, &u2);
        const bool keep1 = act1 && !seen1 && ((int64_t)a1 != self);
        const bool keep2 = act2 && !seen2 && ((int64_t)a2 != self);
        const uint64_t km1 = __ballot(keep1), km2 = __ballot(keep2);
        const uint32_t m1 = __popcll(km1), m2 = __popcll(km2);
        const bool both = (c + m1 + m2 <= P.ccap);                     // the candidate list is sized for beam/8 - 1 + ONE row
        if (keep1) Pl[lanes_below(km1, lane)] = a1;
        if (both && keep2) Pl[m1 + lanes_below(km2, lane)] = a2;
        PANN_WSYNC();
        uint32_t c_after1 = c;
        if (both) {
          if (m1 + m2) c = gather_distances_split<DT, METRIC, LPC, NCH1, PANN_GU_B128(LPC, NCH1)>(P, qreg, qlds, Pl, m1 + m2, m1, cutoff2, C, c, lane, &c_after1);
        } else {
          if (m1) c = gather_distances<DT, METRIC, LPC, NCH1, PANN_GU_B128(LPC, NCH1), false>(P, qreg, qlds, Pl, m1, cutoff2, C, c, lane);
          c_after1 = c;
        }
        PANN_WSYNC();
        // the reference's decision after vertex 1 (another unvisited entry exists): skip iff its list is still short
        const bool two = both && (c_after1 == 0 || c_after1 < beam / 8);
        if (!two) { c = c_after1; filter_undo_codes(P8, P4, u2); }
        // commit: visited.insert(current) (:112-114), counters
        if (cur_idx < 64) { if (lane == cur_idx) fflag[0] = 1; } else { if (lane == cur_idx - 64) fflag[1] = 1; }
        if (two) { if (idx2 < 64) { if (lane == idx2) fflag[0] = 1; } else { if (lane == idx2 - 64) fflag[1] = 1; } }
        if (lane == 0 && P.out.visited_cap) {
          const uint32_t nv = two ? 2u : 1u;
          if (nvis + nv <= P.out.visited_cap) {
            const size_t at = (size_t)qi * P.out.visited_cap + nvis;
            if (P.out.visited_ids) { P.out.visited_ids[at] = cur; if (two) P.out.visited_ids[at + 1] = cur2; }
            if (P.out.visited_dists) { P.out.visited_dists[at] = key_dist(cur_key); if (two) P.out.visited_dists[at + 1] = key_dist(key2); }
          } else {
            atomicOr(P.status, 1u);
          }
        }
        nvis += two ? 2u : 1u;
        degsum += __popcll(__ballot(act1)) + (two ? __popcll(__ballot(act2)) : 0u);
        dcmps += m1 + (two ? m2 : 0u);
        const bool more_left = two ? more_after2 : true;
        const bool skip = (c == 0) || (c < beam / 8 && more_left);
        do_merge = !skip;
      } else {
      if (cur_idx < 64) { if (lane == cur_idx) fflag[0] = 1; } else { if (lane == cur_idx - 64) fflag[1] = 1; }
      if (lane == 0 && P.out.visited_cap) record_visit(P, qi, nvis, cur_key);
      nvis++;
      uint32_t cutoff_ord = BIG_ORD;
      if (f == beam) cutoff_ord = (uint32_t)(entry_key(f - 1) >> 32);

      const uint32_t* row = P.graph + (size_t)cur * P.gstride;
      const uint16_t* crow = CODES ? P.gcode + (size_t)cur * P.gstride : nullptr;
      const bool pref_hit = (pref_id == cur);
      const uint32_t pref_val = pref_row, pref_cval = pref_code;
      uint32_t next_id = SENTINEL;   // the entry after `cur` among the unvisited ones
      {
        uint64_t r0 = um0, r1 = um1;
        if (r0) r0 &= r0 - 1; else r1 &= r1 - 1;
        if (r0 | r1) {
          const int nx = r0 ? __ffsll((unsigned long long)r0) - 1 : 64 + __ffsll((unsigned long long)r1) - 1;
          next_id = key_id(entry_key((uint32_t)nx));
        }
      }
      pref_id = SENTINEL;
      for (uint32_t i0 = 0; i0 < P.gstride; i0 += PANN_WAVE) {
        const uint32_t i = i0 + lane;
        uint32_t a = SENTINEL, code = 0;
        if (i0 == 0 && pref_hit) { a = pref_val; code = pref_cval; }
        else if (i < P.gstride) { a = row[i]; if constexpr (CODES) code = crow[i]; }
        const bool act = (a != SENTINEL) && (i < P.degree_limit);
        const uint64_t am = __ballot(act);
        PANN_STAMP(1);
        if (am == 0ull) break;
        degsum += __popcll(am);
        bool seen;
        if constexpr (CODES) seen = filter_update_codes(P8, P4, hmask, act, a, code, lane, T);
        else seen = filter_update<HASH_LDS>(H, hmask, act, a, lane, T, hb, Lp);
        const bool keep = act && !seen && ((int64_t)a != self);
        const uint64_t km = __ballot(keep);
        const uint32_t m = __popcll(km);
        if (keep) Pl[lanes_below(km, lane)] = a;
        dcmps += m;
        PANN_WSYNC();
        PANN_STAMP(2);
        // requested after the filter's table loads, right before the gather's.  Only for base-point queries (the
        // builder's searches: f32 d=96 search phase -5.5 %); external beam-128 queries measured 2 % slower with it.
        if (i0 == 0 && next_id != SENTINEL && P.query_ids) {
          pref_id = next_id;
          pref_row = (lane < (int)P.gstride) ? P.graph[(size_t)next_id * P.gstride + lane] : SENTINEL;
          if constexpr (CODES) pref_code = (lane < (int)P.gstride) ? (uint32_t)P.gcode[(size_t)next_id * P.gstride + lane] : 0u;
        }
        if (m) c = gather_distances<DT, METRIC, LPC, NCH1, PANN_GU_B128(LPC, NCH1), false>(P, qreg, qlds, Pl, m, cutoff_ord, C, c, lane);
        PANN_WSYNC();
        PANN_STAMP(3);
      }
      const bool skip = (c == 0) || (P.skip_enabled && c < beam / 8 && more_unvisited);
      do_merge = !skip;
      }   // single-vertex path
    }
    if (do_merge) {
      const uint32_t f_old = f;
      const bool track = P.cut_enabled && !first;
      uint32_t lt = 0;
      for (uint32_t c0 = 0; c0 < c; c0 += PANN_WAVE) {
        const uint32_t cc = min(c - c0, (uint32_t)PANN_WAVE);
        const uint64_t ckey = (lane < (int)cc) ? C[c0 + lane] : KEY_INF;
        const bool fl[RB] = {lane < (int)f, lane + 64 < (int)f};
        uint32_t myp = 0, rank_c = 0, below_f[RB] = {0, 0};
        uint64_t live_mask = 0;
        // three 64-bit compares per candidate instead of eight (see the beam-64 kernel): ids decide equality, and the
        // entries below a candidate are those not above it
        const uint64_t vmask0 = __ballot(fl[0]), vmask1 = __ballot(fl[1]);
        const uint32_t cid = (uint32_t)ckey, fid0 = (uint32_t)fkey[0], fid1 = (uint32_t)fkey[1];
        for (uint32_t i = 0; i < cc; i++) {
          const uint64_t kk = readlane64(ckey, (int)i);
          const uint32_t kid = (uint32_t)kk;
          const bool g0 = kk < fkey[0], g1 = kk < fkey[1];
          const uint64_t gt0 = __ballot(g0), gt1 = __ballot(g1);
          const uint64_t eqm = __ballot(fid0 == kid || fid1 == kid);
          const uint64_t dupm = __ballot(cid == kid) & ((1ull << i) - 1ull);
          if (eqm == 0ull && dupm == 0ull) {
            live_mask |= 1ull << i;
            if (lane == (int)i) myp = f - (uint32_t)__popcll(gt0 & vmask0) - (uint32_t)__popcll(gt1 & vmask1);
            rank_c += (kk < ckey) ? 1u : 0u;
            below_f[0] += g0 ? 1u : 0u;
            below_f[1] += g1 ? 1u : 0u;
          }
        }
        const uint32_t nvalid = __popcll(live_mask);
        const bool clive = (lane < (int)cc) && ((live_mask >> lane) & 1ull);
        const uint32_t cpos = rank_c + myp;
        if (clive && cpos < beam) {
          uint32_t flag = 0u;
          for (uint32_t t = 0; t < ndrop; t++)
            flag |= (__hip_atomic_load(DL + t, __ATOMIC_RELAXED, PANN_PRIVATE_SCOPE) == ckey) ? 2u : 0u;
          S[cpos] = ckey; Sv[cpos] = (uint8_t)flag;
        }
#pragma unroll
        for (int r = 0; r < RB; r++) {
          const uint32_t fpos = (uint32_t)lane + 64 * r + below_f[r];
          if (fl[r] && fpos < beam) { S[fpos] = fkey[r]; Sv[fpos] = (uint8_t)fflag[r]; }
          if (track) {
            const bool lost = fl[r] && fflag[r] == 1u && fpos >= beam;
            const uint64_t lm = __ballot(lost);
            if (lost) {
              const uint32_t at = ndrop + lt + lanes_below(lm, lane);
              if (at < P.dcap) DL[at] = fkey[r]; else atomicOr(P.status, 2u);
            }
            lt += __popcll(lm);
          }
        }
        PANN_WSYNC();
        f = min(f + nvalid, beam);
#pragma unroll
        for (int r = 0; r < RB; r++) {
          const bool in = lane + 64 * r < (int)f;
          fkey[r] = in ? S[lane + 64 * r] : KEY_INF;
          fflag[r] = in ? (uint32_t)Sv[lane + 64 * r] : 0u;
        }
        PANN_WSYNC();
      }
      uint32_t f_new = f;
      if (!first && P.cut_enabled && f_new > P.k) {
        const float dk = key_dist(entry_key(P.k));
        const float thr = (float)(P.cut * (double)dk);
        const uint64_t thr_key = (uint64_t)f2ord(thr) << 32;
        const uint32_t ub = __popcll(__ballot(lane < (int)f_new && fkey[0] <= thr_key)) +
                            __popcll(__ballot(lane + 64 < (int)f_new && fkey[1] <= thr_key));
        f_new = max(ub, f_old);
      }
      if (f_new == beam) {
        ndrop = 0;
      } else if (track) {
#pragma unroll
        for (int r = 0; r < RB; r++) {
          const int e = lane + 64 * r;
          const bool lost = e >= (int)f_new && e < (int)f && fflag[r] == 1u;
          const uint64_t lm = __ballot(lost);
          if (lost) {
            const uint32_t at = ndrop + lt + lanes_below(lm, lane);
            if (at < P.dcap) DL[at] = fkey[r]; else atomicOr(P.status, 2u);
          }
          lt += __popcll(lm);
        }
        ndrop = min(ndrop + lt, P.dcap);
        if (lt) __builtin_amdgcn_s_waitcnt(0);
      }
      f = f_new;
#pragma unroll
      for (int r = 0; r < RB; r++) if (lane + 64 * r >= (int)f) { fkey[r] = KEY_INF; fflag[r] = 0u; }
      c = 0;
    }
    PANN_STAMP(4);
    first = false;
  }
  PANN_STAMP_FLUSH(qi);

  const size_t qo = (size_t)qi * P.out.out_k;
#pragma unroll
  for (int r = 0; r < RB; r++) {
    const uint32_t j = lane + 64 * r;
    if (j < P.out.out_k) {
      const bool ok = j < f;
      if (P.out.ids) P.out.ids[qo + j] = ok ? key_id(fkey[r]) : SENTINEL;
      if (P.out.dists) P.out.dists[qo + j] = ok ? key_dist(fkey[r]) : __builtin_inff();
    }
  }
  if (lane == 0) write_counters(P, qi, f, nvis, dcmps, degsum);
  if constexpr (HASH_LDS) {
    break;
  } else {
    PANN_WSYNC();
    slot = next_slot(P, lane, slot);
  }
  }   // while (slot < P.nq)
}

// ---- host side: the plan (search_plan.h) and the dispatch ----
// The plan's A/B switches, read here and nowhere else (`make alt` builds; in the shipped library ab_env answers null).  As before,
// the three b128 switches are read once per process, PANN_B64_SEEN and PANN_FORCE_LPC at every call.
static PlanSwitches plan_switches() {
  static const bool b128_lds = ab_env("PANN_B128_LDS") != nullptr, b128_no24 = ab_env("PANN_B128_NO24") != nullptr;
  static const char* split = ab_env("PANN_B128_SPLIT");
  PlanSwitches s{b128_lds, b128_no24};
  if (split) s.b128_split = (uint32_t)atoi(split);
  if (const char* v = ab_env("PANN_B64_SEEN")) s.b64_seen = atoi(v) != 0;      // PANN_B64_SEEN=0 is the kernel without V
  if (const char* v = ab_env("PANN_FORCE_LPC")) s.force_lpc = (uint32_t)atoi(v);
  return s;
}
void choose_point_layout(uint32_t dbytes, uint32_t* lpc, uint32_t* nch) { choose_point_layout(dbytes, plan_switches().force_lpc, lpc, nch); }
static SearchPlan plan_of(const DeviceIndex& ix, const SearchArgs& a) {
  const PlanIndex pi{ix.dtype, ix.metric, ix.lpc, ix.nch, ix.max_deg, ix.gstride, ix.n, ix.sk_stride, ix.b64_seen,
                     ix.codes_valid && ix.gcode && ix.rank16};
  const PlanCall pc{a.nq, a.nstarts, a.k, a.beam, a.degree_limit, a.cut, a.dcap, a.filter != 0, a.masked, a.steer != 0};
  return make_plan(pi, pc, plan_switches());
}
size_t search_workspace_bytes(const DeviceIndex& ix, const SearchArgs& a) { return (size_t)plan_of(ix, a).ws_bytes; }

// The kernel of a plan's (kernel, table, mode) for one point layout.  make_plan plans no other combination: no masked or sketch
// b128, no sketch b64, no masked b64 of a layout that masked_b64_fits rules out.  The second form picks the handle's element type,
// metric and point layout; a handle with none of the known ones (a corrupt one) gets no kernel, as before.
using SearchKernel = void (*)(BSParams);
template <int DT, int METRIC, int LPC, bool NCH1>
static SearchKernel plan_kernel(const SearchPlan& p) {
  const bool lds = p.table == TABLE_LDS;
  switch (p.kernel * 8 + p.mode) {
    case KERNEL_GENERIC * 8 + MODE_SKETCH:  // frontier in LDS
      return lds ? beam_search_kernel<DT, METRIC, LPC, NCH1, true, true> : beam_search_kernel<DT, METRIC, LPC, NCH1, false, true>;
    case KERNEL_B64 * 8 + MODE_LABELS:      // frontier in registers
      if constexpr (masked_b64_fits(DT, LPC, NCH1)) return beam_search_b64_kernel<DT, METRIC, LPC, NCH1, MASK_LABELS>;
      break;
    case KERNEL_GENERIC * 8 + MODE_LABELS:
      if (p.steer) return lds ? beam_search_kernel<DT, METRIC, LPC, NCH1, true, false, MASK_LABELS, true> : beam_search_kernel<DT, METRIC, LPC, NCH1, false, false, MASK_LABELS, true>;
      return lds ? beam_search_kernel<DT, METRIC, LPC, NCH1, true, false, MASK_LABELS> : beam_search_kernel<DT, METRIC, LPC, NCH1, false, false, MASK_LABELS>;
    case KERNEL_B64 * 8 + MODE_BITMAP:
      if constexpr (masked_b64_fits(DT, LPC, NCH1)) return beam_search_b64_kernel<DT, METRIC, LPC, NCH1, MASK_BITMAP>;
      break;
    case KERNEL_GENERIC * 8 + MODE_BITMAP:
      if (p.steer) return lds ? beam_search_kernel<DT, METRIC, LPC, NCH1, true, false, MASK_BITMAP, true> : beam_search_kernel<DT, METRIC, LPC, NCH1, false, false, MASK_BITMAP, true>;
      return lds ? beam_search_kernel<DT, METRIC, LPC, NCH1, true, false, MASK_BITMAP> : beam_search_kernel<DT, METRIC, LPC, NCH1, false, false, MASK_BITMAP>;
    case KERNEL_B64 * 8 + MODE_PLAIN_V: return beam_search_b64_kernel<DT, METRIC, LPC, NCH1, B64_SEEN>;
    case KERNEL_B64 * 8 + MODE_PLAIN: return beam_search_b64_kernel<DT, METRIC, LPC, NCH1>;
    case KERNEL_B128 * 8 + MODE_PLAIN:      // two frontier entries per lane
      if (p.table == TABLE_CODES) return beam_search_b128_kernel<DT, METRIC, LPC, NCH1, true, true>;
      return !lds ? beam_search_b128_kernel<DT, METRIC, LPC, NCH1, false> : beam_search_b128_kernel<DT, METRIC, LPC, NCH1, true>;
    case KERNEL_GENERIC * 8 + MODE_PLAIN:
      return lds ? beam_search_kernel<DT, METRIC, LPC, NCH1, true> : beam_search_kernel<DT, METRIC, LPC, NCH1, false>;
  }
  return nullptr;      // not a plan of make_plan: the launch fails with hipErrorInvalidValue
}
static SearchKernel plan_kernel(const DeviceIndex& ix, const SearchPlan& p) {
  const bool type_ok = ix.dtype == PANN_U4 ? ix.metric == PANN_L2 : ix.dtype == PANN_I4 ? ix.metric == PANN_MIPS      // a four-bit handle's only pairings
                       : esize_of(ix.dtype) != 0 && (ix.metric == PANN_L2 || ix.metric == PANN_MIPS);
  const bool lpc_ok = ix.lpc == 8 || ix.lpc == 16 || (layout_query_in_registers(ix) ? ix.lpc == 32 : ix.lpc == 4);
  SearchKernel kern = nullptr;
#define CALL_BS(DT, MT, LPC, NCH1) kern = plan_kernel<DT, MT, LPC, NCH1>(p)
  if (!type_ok || !lpc_ok) return nullptr;
  if (!is_4bit_dtype(ix.dtype)) PANN_TYPE_SWITCH(ix, CALL_BS);
  else if (ix.dtype == PANN_U4) PANN_LAYOUT_SWITCH(ix, PANN_U4, PANN_L2, CALL_BS);
  else PANN_LAYOUT_SWITCH(ix, PANN_I4, PANN_MIPS, CALL_BS);
#undef CALL_BS
  return kern;
}

int launch_beam_search(const DeviceIndex& ix, const SearchArgs& a, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (a.nq == 0) return PANN_OK;
  if (a.nq > 0xFFFFFFF0ull) { set_error("pann_batch_search: nq too large"); return PANN_ERR_BAD_ARG; }
  if (a.beam <= 0 || a.beam > 65536) { set_error("pann_batch_search: beam out of range [1,65536]"); return PANN_ERR_BAD_ARG; }
  if (a.nstarts == 0) { set_error("beam search expects at least one start point"); return PANN_ERR_BAD_ARG; }  // beamSearch.h:38-41
  if ((int64_t)a.nstarts > a.beam) { set_error("pann_batch_search: more start points than beam"); return PANN_ERR_BAD_ARG; }
  if (a.out.out_k > (uint64_t)a.beam) {  // beamSearch.h:368-372
    set_error("Error: beam search parameter Q same size or smaller than k"); return PANN_ERR_BAD_ARG;
  }
  if ((a.queries == nullptr) == (a.query_ids == nullptr)) { set_error("pann_batch_search: exactly one of queries / query_ids must be given"); return PANN_ERR_BAD_ARG; }
  if (a.filter) {
    if (!ix.sketch || !sketch_kind_ok(ix.sk_kind)) { set_error("pann_batch_search_filtered: no sketch attached to the index"); return PANN_ERR_BAD_ARG; }
    if ((a.queries != nullptr) != (a.sketch_queries != nullptr)) {
      set_error("pann_batch_search_filtered: sketch_queries go with queries, and only with them"); return PANN_ERR_BAD_ARG;
    }
    if (a.sketch_queries && (a.sq_stride < sketch_row_bytes(ix.sk_kind, ix.d) || a.sq_stride % 8 != 0 || (uintptr_t)a.sketch_queries % 8 != 0)) {
      set_error("pann_batch_search_filtered: sketch query stride smaller than a sketch row, or rows not 8-byte aligned"); return PANN_ERR_BAD_ARG;
    }
  }
  // the bitmap, its stride and out_k <= 64 are checked by the entry points (api.hip: masked_limits in search_refusals); no entry point combines a mask
  // with the sketch filter, and there is no kernel for it
  if (a.masked && a.filter) { set_error("pann_batch_search_masked: the sketch filter has no masked form"); return PANN_ERR_UNSUPPORTED; }
  // label mode: the entry points have checked the handle's labels, the kind and npreds (api.hip: filter_checks)
  if (a.masked == MASK_LABELS && (!a.labels || !a.preds || a.pred_stride > 1 || !pred_kind_known(a.pred_kind))) {
    set_error("pann_batch_search_labeled: labels, predicates of a known kind and a predicate stride of 0 or 1 are needed"); return PANN_ERR_BAD_ARG;
  }
  if (a.steer && (!a.masked || a.filter)) { set_error("pann_batch_search_steered: steering goes with a bitmap or label predicates, and not with the sketch filter"); return PANN_ERR_UNSUPPORTED; }
  const SearchPlan p = plan_of(ix, a);
  if (p.lds_bytes > 160 * 1024) { set_error("pann_batch_search: beam/degree too large for LDS state"); return PANN_ERR_UNSUPPORTED; }
  if (p.ws_bytes > ws_bytes) { set_error("pann_batch_search: workspace too small"); return PANN_ERR_BAD_ARG; }
  BSParams P;
  P.points = ix.points; P.pstride = ix.pstride; P.dbytes = ix.dbytes; P.nch = ix.nch; P.exact = ix.exact;
  P.graph = ix.graph; P.gstride = ix.gstride; P.max_deg = ix.max_deg;
  P.queries = a.queries; P.qstride = a.qstride; P.query_ids = a.query_ids;
  P.starts = a.starts; P.nstarts = a.nstarts; P.starts_stride = a.starts_per_query ? a.nstarts : 0u; P.nq = (uint32_t)a.nq;
  P.k = (uint32_t)std::max<int64_t>(a.k, 0); P.beam = (uint32_t)a.beam;
  P.limit = (uint32_t)std::min<int64_t>(std::max<int64_t>(a.limit, 0), 0xFFFFFFFFll);
  P.degree_limit = p.deg_eff; P.cut = a.cut;
  P.skip_enabled = (a.limit >= 2 * a.beam) ? 1u : 0u; P.cut_enabled = (a.k > 0 && ix.metric == PANN_L2) ? 1u : 0u;
  P.bits = p.bits; P.bcap = p.bcap; P.ccap = p.ccap; P.hsplit = p.hsplit; P.p24 = p.p24; P.sk_lds_off = p.sk_lds_off; P.rl_off = p.rl_off;   // the plan's
  uint8_t* w = (uint8_t*)ws;      // 256 bytes (counter, status) | dropped lists | filter tables of a persistent launch
  P.work_counter = (uint32_t*)w; P.status = (uint32_t*)(w + 64);
  P.dropped = (uint64_t*)(w + 256); P.dcap = p.dcap;
  static const char* pf = ab_env("PANN_PRIO_FROM");              // A/B switch: tenths of the grid without priority (default 8; 10 = off)
  const uint32_t tenths = pf ? (uint32_t)atoi(pf) : 8u;
  P.prio_start = tenths >= 10 ? 0xFFFFFFFFu : (uint32_t)((uint64_t)a.nq * tenths / 10);
  P.gcode = ix.gcode; P.rank16 = ix.rank16; P.order = a.order;
  P.hash_global = p.persistent() ? (uint32_t*)(w + 256 + p.dropped_bytes(a.nq)) : nullptr;
  P.out = a.out; P.stamps = nullptr;
  P.sketch = a.filter ? ix.sketch : nullptr; P.sk_stride = a.filter ? ix.sk_stride : 0u;
  P.sk_kind = (uint32_t)ix.sk_kind; P.sk_as_written = ix.sk_as_written; P.sk_nblk = (ix.d + 63) / 64;
  P.sketch_queries = a.sketch_queries; P.sq_stride = a.sq_stride;
  P.sk_row_bytes = a.filter ? sketch_row_bytes(ix.sk_kind, ix.d) : 0u;
  P.pruned_cmps = a.filter ? a.pruned_cmps : nullptr;
  P.allow = a.masked == MASK_BITMAP ? a.allow : nullptr; P.allow_stride = a.masked == MASK_BITMAP ? a.allow_stride : 0;
  const bool lab = a.masked == MASK_LABELS;
  P.labels = lab ? a.labels : nullptr; P.preds = lab ? a.preds : nullptr;
  P.pred_stride = lab ? a.pred_stride : 0u; P.pred_kind = lab ? (uint32_t)a.pred_kind : 0u;
  P.result_count = a.masked ? a.result_count : nullptr; P.allowed_cmps = a.masked ? a.allowed_cmps : nullptr;
  if (p.steer) {      // in the storage of sk_kind, sk_lds_off and pruned_cmps: a steered launch has no sketch
    P.fill = a.fill == 0 || a.fill > p.deg_eff ? p.deg_eff : a.fill;      // 0: deg_eff; clamped
    P.br_off = p.br_off; P.steer_out = a.steer_out;
  }
#ifdef PANN_STAMPS
  static unsigned long long* d_stamps = nullptr; static size_t stamps_cap = 0;
  if (stamps_cap < a.nq) { if (d_stamps) (void)hipFree(d_stamps); (void)hipMalloc((void**)&d_stamps, a.nq * 64); stamps_cap = a.nq; }
  P.stamps = d_stamps;
#endif
  PANN_HIP(hipMemsetAsync(w, 0, 256, stream));

  // One launch: LDS above the 48 KB default is asked for by attribute; one block per query, or -- persistent kernels, whose blocks
  // pull queries from the counter -- one block per filter table of the workspace.
  hipError_t e = hipErrorInvalidValue;
  if (const SearchKernel kern = plan_kernel(ix, p)) {
    if (p.lds_bytes > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    const uint32_t grid = p.persistent() ? (uint32_t)std::min<uint64_t>(P.nq, p.slots) : P.nq;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(PANN_WAVE), p.lds_bytes, stream, P);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return hip_fail(e, "beam_search_kernel launch");
  // the status word follows the results on the launch stream (pann_search_out::status, device pointer here)
  if (a.out.status) PANN_HIP(hipMemcpyAsync(a.out.status, P.status, 4, hipMemcpyDeviceToDevice, stream));
#ifdef PANN_STAMPS
  if (ab_env("PANN_STAMPS_PRINT") && a.nq >= 1000) {
    (void)hipStreamSynchronize(stream);
    std::vector<unsigned long long> h(a.nq * 8);
    (void)hipMemcpy(h.data(), P.stamps, a.nq * 64, hipMemcpyDeviceToHost);
    double sum[8] = {0}; for (size_t q = 0; q < a.nq; q++) for (int i = 0; i < 8; i++) sum[i] += (double)h[q * 8 + i];
    double tot = 0; for (int i = 0; i < 5; i++) tot += sum[i];
    fprintf(stderr, "[stamps] per-query cycles: head %.0f row %.0f filter %.0f gather %.0f merge %.0f total %.0f  (shares %.1f%% %.1f%% %.1f%% %.1f%% %.1f%%)\n",
            sum[0] / a.nq, sum[1] / a.nq, sum[2] / a.nq, sum[3] / a.nq, sum[4] / a.nq, tot / a.nq, 100 * sum[0] / tot, 100 * sum[1] / tot,
            100 * sum[2] / tot, 100 * sum[3] / tot, 100 * sum[4] / tot);
  }
#endif
  return PANN_OK;
}

}  // namespace pann
