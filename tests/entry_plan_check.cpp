// entry_plan_check.cpp -- the medoid form's host arithmetic in parlayann_amd/csrc/grouped_plan.h on its own, built by a plain host
// compiler under sanitizers and run by tests/test_entry_plan_cpu.py: the pieces of a list, the pieces of a chunk, the sums a piece
// leaves, and the scratch layout (piece offsets | 64-bit sums).  The piece offsets are restated here as the device's scan computes
// them (an exclusive scan of the lists' piece counts), written into a buffer of exactly the planned size, and every piece's sums
// are touched, so AddressSanitizer sees a byte too few.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../parlayann_amd/csrc/grouped_plan.h"

using pann::CentroidScratch;
using pann::GroupedChunk;
using pann::GroupedPlan;
typedef std::vector<uint32_t> V32;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static const uint64_t P = pann::CENTROID_PIECE_IDS;

static void named_cases() {
  CHECK(P == 512);
  CHECK(pann::centroid_pieces_of(0) == 0 && pann::centroid_pieces_of(1) == 1 && pann::centroid_pieces_of(P - 1) == 1);
  CHECK(pann::centroid_pieces_of(P) == 1 && pann::centroid_pieces_of(P + 1) == 2 && pann::centroid_pieces_of(3 * P + 7) == 4);
  CHECK(pann::centroid_pieces_of(0x7FFFFFFFull) == (1ull << 22));
  // sums per piece: 16 / esize coordinates for every 16-byte chunk that holds data
  CHECK(pann::centroid_row_sums(256, 2) == 128 && pann::centroid_row_sums(200, 2) == 104 && pann::centroid_row_sums(200, 1) == 208);
  CHECK(pann::centroid_row_sums(512, 4) == 128 && pann::centroid_row_sums(1, 1) == 16 && pann::centroid_row_sums(16, 4) == 4);
  {   // one list of P + 1 ids, d = 128 f16: 8 bytes of offsets rounded up to 256, then 2 pieces x 128 sums x 8 bytes
    const CentroidScratch s(1, 2, 128);
    CHECK(s.o_partial == 256 && s.bytes == 256 + 2 * 128 * 8);
  }
  {   // 63 lists: 64 words of offsets are exactly 256 bytes; 64 lists need a second block
    CHECK(CentroidScratch(63, 0, 16).o_partial == 256 && CentroidScratch(63, 0, 16).bytes == 256);
    CHECK(CentroidScratch(64, 5, 16).o_partial == 512 && CentroidScratch(64, 5, 16).bytes == 512 + 5 * 16 * 8);
  }
  {   // the medoid form of the plan: one query per entry, the lists 0, 1, P, P + 1, 3 P + 7
    const V32 hist = {1, 1, 1, 1, 1}, allowed = {0, 1, (uint32_t)P, (uint32_t)P + 1, 3 * (uint32_t)P + 7};
    const GroupedPlan p(hist.data(), allowed.data(), 5, 1u << 20, UINT64_MAX);
    CHECK(p.chunks.size() == 1 && pann::centroid_chunk_pieces(p, p.chunks[0], allowed.data()) == 0 + 1 + 1 + 2 + 4);
    const GroupedPlan q(hist.data(), allowed.data(), 5, P + 1, UINT64_MAX);      // budget P + 1: {0, 1, P} | {P + 1} | {3 P + 7}
    CHECK(q.chunks.size() == 3);
    CHECK(pann::centroid_chunk_pieces(q, q.chunks[0], allowed.data()) == 2 && pann::centroid_chunk_pieces(q, q.chunks[1], allowed.data()) == 2 &&
          pann::centroid_chunk_pieces(q, q.chunks[2], allowed.data()) == 4);
  }
}

static void sweep() {
  std::mt19937_64 rng(20252);
  auto draw = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  for (int it = 0; it < 300; it++) {
    const uint64_t G = draw(1, 40);
    V32 hist(G, 1), allowed(G);
    uint64_t total = 0;
    for (uint64_t g = 0; g < G; g++) {
      const uint64_t kind = draw(0, 5);
      allowed[g] = (uint32_t)(kind == 0 ? 0 : kind == 1 ? draw(1, 3) * P + draw(0, 2) - 1 : draw(0, 5000));
      total += allowed[g];
    }
    const uint64_t budget = it % 3 == 0 ? draw(1, 2000) : it % 3 == 1 ? draw(1, total + 10) : total + draw(1, 100);
    const uint32_t esize = (uint32_t[]){1, 2, 4}[draw(0, 2)], dbytes = (uint32_t)draw(1, 700) * esize;
    const uint32_t row_sums = pann::centroid_row_sums(dbytes, esize);
    CHECK((uint64_t)row_sums * esize >= dbytes && (uint64_t)row_sums * esize < dbytes + 16 && (uint64_t)row_sums * esize % 16 == 0);
    const GroupedPlan p(hist.data(), allowed.data(), G, budget, it % 4 == 0 ? draw(1, 5) : UINT64_MAX);
    uint64_t all_pieces = 0;
    for (const GroupedChunk& c : p.chunks) {
      const size_t S = c.u1 - c.u0;
      const uint64_t pieces = pann::centroid_chunk_pieces(p, c, allowed.data());
      CHECK(pieces >= c.ids / P && pieces <= c.ids / P + S);
      const CentroidScratch sc(S, pieces, row_sums);
      CHECK(sc.o_partial % 256 == 0 && sc.o_partial >= (S + 1) * 4 && sc.bytes == sc.o_partial + pieces * row_sums * 8);
      uint8_t* buf = (uint8_t*)malloc(sc.bytes ? sc.bytes : 1);
      // the device's scan, restated: piece_off[s] = the pieces of the lists before s, piece_off[S] = all of them
      uint32_t* piece_off = (uint32_t*)buf;
      uint32_t run = 0;
      for (size_t s = 0; s < S; s++) { piece_off[s] = run; run += (uint32_t)pann::centroid_pieces_of(allowed[p.used[c.u0 + s]]); }
      piece_off[S] = run;
      CHECK(run == pieces);                                       // host count == device scan's total: the launch covers every piece
      uint64_t* partial = (uint64_t*)(buf + sc.o_partial);
      for (size_t s = 0; s < S; s++) {
        const uint64_t len = allowed[p.used[c.u0 + s]];
        for (uint32_t pc = piece_off[s]; pc < piece_off[s + 1]; pc++) {
          const uint64_t first = (uint64_t)(pc - piece_off[s]) * P, cnt = std::min(len, first + P) - first;
          CHECK(first < len && cnt >= 1 && cnt <= P);           // every piece holds 1 .. P ids of its own list
          memset(partial + (uint64_t)pc * row_sums, 0x5A, (size_t)row_sums * 8);      // the piece's sums lie inside the scratch
        }
        CHECK((uint64_t)(piece_off[s + 1] - piece_off[s]) * P >= len && (len == 0 || (uint64_t)(piece_off[s + 1] - piece_off[s] - 1) * P < len));
      }
      free(buf);
      all_pieces += pieces;
    }
    uint64_t want = 0;
    for (uint64_t g = 0; g < G; g++) want += (allowed[g] + P - 1) / P;
    CHECK(all_pieces == want);
  }
}

int main() {
  named_cases();
  sweep();
  printf("entry_plan: ok\n");
  return 0;
}
