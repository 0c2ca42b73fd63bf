// grouped_plan.h -- the host arithmetic of the segmented dense launches: the tiles of a list of segments, and the plan of the
// grouped exact kNN (DESIGN.md "Exact kNN by predicate group"): which table entries are used, how they are cut into chunks, and
// the bytes that go up to the device.  No HIP and nothing of pann_internal.h in here: a plain host compiler builds it
// (tests/test_grouped_plan_cpu.py does, under sanitizers).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <iterator>
#include <vector>

#include "scratch_carve.h"

namespace pann {

// One tile of 64 A rows per (segment, a0): segment s holds the rows [off[s], off[s + 1]), an empty one has no tile.  The tiles are
// written through the two iterators: pointers into a buffer with room for them, or back_inserters of two vectors.
template <class Out> inline void append_tiles(const uint64_t* off, size_t nseg, Out tile_seg, Out tile_a0) {
  for (size_t s = 0; s < nseg; s++)
    for (uint64_t a = off[s]; a < off[s + 1]; a += 64) { *tile_seg++ = (uint32_t)s; *tile_a0++ = (uint32_t)a; }
}

// most ids the lists of one chunk hold (they are indexed in 31 bits; max_list_ids == 0, include/pann.h: 64 MB of ids, as much again of
// bitmap rows), and most entries of one chunk: in the label form the entries' bitmap rows of `words` words are expanded per chunk and fit the budget too
inline uint64_t grouped_budget(uint64_t max_list_ids) { return std::min<uint64_t>(max_list_ids ? max_list_ids : 16ull << 20, 0x7FFFFFFFull); }
inline uint64_t grouped_row_cap(uint64_t budget, uint64_t words, bool label_form) {
  return label_form ? std::max<uint64_t>(1, budget / std::max<uint64_t>(words, 1)) : UINT64_MAX;
}

// One chunk of the plan: the used table entries [u0, u1) as the segments of one dense launch; o_*: where its arrays lie in the plan
struct GroupedChunk { size_t u0, u1; uint64_t a_base, na, ids, max_ids; uint32_t ntiles; size_t o_aoff, o_boff, o_tseg, o_ta0; };

// hist[g]: queries of table entry g, allowed[g]: points it allows (g < G).  The plan's bytes: used (U words) | per chunk: a_off and
// b_off (S + 1 uint64 each: the exclusive scans of the segments' queries and ids), tile_seg and tile_a0 (ntiles words each);
// every array 8-byte aligned.
struct GroupedPlan {
  std::vector<uint32_t> used;       // the entries with at least one query, ascending
  std::vector<uint64_t> first;      // first slot of every used entry among the sorted queries (the scan of hist), and nq behind them
  std::vector<GroupedChunk> chunks;
  size_t plan_bytes = 0;
  size_t max_rows = 0, max_na = 0; uint64_t max_ids = 0;      // the largest chunk: entries, queries, ids (the device buffers' sizes)
  static size_t al8(size_t x) { return (x + 7) & ~(size_t)7; }

  // chunks of consecutive used entries whose lists fit the budget; an entry larger than it is a chunk alone
  GroupedPlan(const uint32_t* hist, const uint32_t* allowed, uint64_t G, uint64_t budget, uint64_t row_cap) {
    uint64_t run = 0;
    for (uint64_t g = 0; g < G; g++) if (hist[g]) { used.push_back((uint32_t)g); first.push_back(run); run += hist[g]; }
    first.push_back(run);
    const size_t U = used.size();
    plan_bytes = al8(U * 4);
    for (size_t u = 0; u < U;) {
      GroupedChunk c{u, u, first[u], 0, 0, 0, 0, 0, 0, 0, 0};
      while (c.u1 < U && (c.u1 == c.u0 || (c.ids + allowed[used[c.u1]] <= budget && c.u1 - c.u0 < row_cap))) {
        const uint64_t cg = allowed[used[c.u1]];
        c.ids += cg; c.max_ids = std::max(c.max_ids, cg);
        c.ntiles += (uint32_t)((hist[used[c.u1]] + 63) / 64);
        c.u1++;
      }
      c.na = first[c.u1] - c.a_base;
      const size_t S = c.u1 - c.u0;
      c.o_aoff = plan_bytes; c.o_boff = c.o_aoff + (S + 1) * 8; c.o_tseg = c.o_boff + (S + 1) * 8; c.o_ta0 = c.o_tseg + al8((size_t)c.ntiles * 4);
      plan_bytes = c.o_ta0 + al8((size_t)c.ntiles * 4);
      max_rows = std::max(max_rows, S); max_na = std::max<size_t>(max_na, c.na); max_ids = std::max(max_ids, c.ids);
      chunks.push_back(c);
      u = c.u1;
    }
  }

  // the plan into `buf` (plan_bytes bytes, 8-byte aligned); the padding between the arrays is left as it is
  void write(const uint32_t* allowed, uint8_t* buf) const {
    if (!used.empty()) memcpy(buf, used.data(), used.size() * 4);
    for (const GroupedChunk& c : chunks) {
      uint64_t* a_off = (uint64_t*)(buf + c.o_aoff), *b_off = (uint64_t*)(buf + c.o_boff);
      const size_t S = c.u1 - c.u0;
      uint64_t b = 0;
      for (size_t s = 0; s < S; s++) { a_off[s] = first[c.u0 + s] - c.a_base; b_off[s] = b; b += allowed[used[c.u0 + s]]; }
      a_off[S] = c.na; b_off[S] = b;
      append_tiles(a_off, S, (uint32_t*)(buf + c.o_tseg), (uint32_t*)(buf + c.o_ta0));
    }
  }
};

// ---- the medoid form of the grouped route (DESIGN.md "Entry points"): the lists of a chunk are cut into pieces of
// CENTROID_PIECE_IDS consecutive ids, one workgroup sums one piece, and the sums wait in scratch for the finish pass.  The kernels
// (entry_points.hip) count a list's pieces with the same function, so host and device agree on every offset.
constexpr uint32_t CENTROID_PIECE_IDS = 512;      // pann_index_get_option("centroid_piece_ids")
constexpr uint64_t centroid_pieces_of(uint64_t ids) { return (ids + CENTROID_PIECE_IDS - 1) / CENTROID_PIECE_IDS; }
// the pieces of chunk c's lists
inline uint64_t centroid_chunk_pieces(const GroupedPlan& p, const GroupedChunk& c, const uint32_t* allowed) {
  uint64_t pieces = 0;
  for (size_t u = c.u0; u < c.u1; u++) pieces += centroid_pieces_of(allowed[p.used[u]]);
  return pieces;
}
// sums one piece leaves: the coordinates of the 16-byte chunks of a row that hold data (esize: bytes per element, 1, 2 or 4)
constexpr uint32_t centroid_row_sums(uint32_t dbytes, uint32_t esize) { return (dbytes + 15) / 16 * (16 / esize); }
// The scratch of a chunk of S lists: piece_off (S + 1 words: the pieces before every list, and their total) | 64-bit sums,
// row_sums per piece, 256-byte aligned.
struct CentroidScratch {
  size_t o_partial, bytes;
  CentroidScratch(uint64_t S, uint64_t pieces, uint32_t row_sums)
      : o_partial(Carve::align(((size_t)S + 1) * 4)), bytes(o_partial + (size_t)pieces * row_sums * 8) {}
};

}  // namespace pann
