// grouped_plan_check.cpp -- parlayann_amd/csrc/grouped_plan.h on its own, built by a plain host compiler under sanitizers and run
// by tests/test_grouped_plan_cpu.py: the chunks, offsets, tiles and byte layout of the grouped exact kNN's plan.  The expected
// values of the named cases were worked by hand from the chunk loop.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../parlayann_amd/csrc/grouped_plan.h"

using pann::GroupedChunk;
using pann::GroupedPlan;
typedef std::vector<uint32_t> V32;
typedef std::vector<uint64_t> V64;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

// the plan written into a buffer of exactly plan_bytes (ASan sees a byte too many), and chunk c's four arrays read back from it
struct Written {
  uint8_t* buf; const GroupedPlan& p;
  Written(const GroupedPlan& plan, const V32& allowed) : buf((uint8_t*)malloc(plan.plan_bytes ? plan.plan_bytes : 1)), p(plan) {
    p.write(allowed.data(), buf);
  }
  ~Written() { free(buf); }
  V32 used() const { return V32((const uint32_t*)buf, (const uint32_t*)buf + p.used.size()); }
  V64 a_off(size_t c) const { const uint64_t* a = (const uint64_t*)(buf + p.chunks[c].o_aoff); return V64(a, a + (p.chunks[c].u1 - p.chunks[c].u0) + 1); }
  V64 b_off(size_t c) const { const uint64_t* a = (const uint64_t*)(buf + p.chunks[c].o_boff); return V64(a, a + (p.chunks[c].u1 - p.chunks[c].u0) + 1); }
  V32 tile_seg(size_t c) const { const uint32_t* a = (const uint32_t*)(buf + p.chunks[c].o_tseg); return V32(a, a + p.chunks[c].ntiles); }
  V32 tile_a0(size_t c) const { const uint32_t* a = (const uint32_t*)(buf + p.chunks[c].o_ta0); return V32(a, a + p.chunks[c].ntiles); }
};

static const V32 kHist = {65, 0, 64, 1, 3}, kAllowed = {10, 999, 0, 7, 5};

static void named_cases() {
  {   // A: everything fits one chunk
    const GroupedPlan p(kHist.data(), kAllowed.data(), 5, 1000, UINT64_MAX);
    CHECK((p.used == V32{0, 2, 3, 4}) && (p.first == V64{0, 65, 129, 130, 133}));
    CHECK(p.chunks.size() == 1);
    const GroupedChunk& c = p.chunks[0];
    CHECK(c.u0 == 0 && c.u1 == 4 && c.a_base == 0 && c.ids == 22 && c.max_ids == 10 && c.na == 133 && c.ntiles == 5);
    CHECK(c.o_aoff == 16 && c.o_boff == 56 && c.o_tseg == 96 && c.o_ta0 == 120 && p.plan_bytes == 144);
    CHECK(p.max_rows == 4 && p.max_na == 133 && p.max_ids == 22);
    const Written w(p, kAllowed);
    CHECK(w.used() == p.used);
    CHECK((w.a_off(0) == V64{0, 65, 129, 130, 133}) && (w.b_off(0) == V64{0, 10, 10, 17, 22}));
    CHECK((w.tile_seg(0) == V32{0, 0, 1, 2, 3}) && (w.tile_a0(0) == V32{0, 64, 65, 129, 130}));
  }
  {   // B: budget 12 -- the entry that allows nothing rides along, and a sum exactly at the budget is accepted
    const GroupedPlan p(kHist.data(), kAllowed.data(), 5, 12, UINT64_MAX);
    CHECK(p.chunks.size() == 2);
    const GroupedChunk& c1 = p.chunks[0], &c2 = p.chunks[1];
    CHECK(c1.u0 == 0 && c1.u1 == 2 && c1.ids == 10 && c1.na == 129 && c1.ntiles == 3 && c1.a_base == 0);
    CHECK(c2.u0 == 2 && c2.u1 == 4 && c2.a_base == 129 && c2.na == 4 && c2.ids == 12 && c2.ntiles == 2 && c2.max_ids == 7);
    CHECK(p.max_rows == 2 && p.max_na == 129 && p.max_ids == 12);
    const Written w(p, kAllowed);
    CHECK((w.a_off(0) == V64{0, 65, 129}) && (w.b_off(0) == V64{0, 10, 10}) && (w.tile_seg(0) == V32{0, 0, 1}) && (w.tile_a0(0) == V32{0, 64, 65}));
    CHECK((w.a_off(1) == V64{0, 1, 4}) && (w.b_off(1) == V64{0, 7, 12}) && (w.tile_seg(1) == V32{0, 1}) && (w.tile_a0(1) == V32{0, 1}));
  }
  {   // C: an entry larger than the budget is a chunk alone, and the one behind it starts a new chunk
    const V32 allowed = {10, 999, 0, 50, 5};
    const GroupedPlan p(kHist.data(), allowed.data(), 5, 12, UINT64_MAX);
    CHECK(p.chunks.size() == 3);
    CHECK(p.chunks[0].u0 == 0 && p.chunks[0].u1 == 2 && p.chunks[0].ids == 10);
    CHECK(p.chunks[1].u0 == 2 && p.chunks[1].u1 == 3 && p.chunks[1].ids == 50 && p.chunks[1].a_base == 129 && p.chunks[1].na == 1);
    CHECK(p.chunks[2].u0 == 3 && p.chunks[2].u1 == 4 && p.chunks[2].ids == 5 && p.chunks[2].a_base == 130 && p.chunks[2].na == 3);
    CHECK(p.max_ids == 50);
  }
  {   // D: a row cap of one entry
    const GroupedPlan p(kHist.data(), kAllowed.data(), 5, 1000, 1);
    CHECK(p.chunks.size() == 4 && p.max_rows == 1);
    for (size_t i = 0; i < 4; i++) CHECK(p.chunks[i].u0 == i && p.chunks[i].u1 == i + 1 && p.chunks[i].a_base == p.first[i]);
  }
  {   // E: the budget and the row cap of the label form
    CHECK(pann::grouped_budget(0) == (16ull << 20) && pann::grouped_budget(5) == 5);
    CHECK(pann::grouped_budget(0x7FFFFFFFull) == 0x7FFFFFFFull && pann::grouped_budget(0x80000000ull) == 0x7FFFFFFFull);
    CHECK(pann::grouped_budget(UINT64_MAX) == 0x7FFFFFFFull);
    CHECK(pann::grouped_row_cap(1000, 3, false) == UINT64_MAX);
    CHECK(pann::grouped_row_cap(1000, 3, true) == 333 && pann::grouped_row_cap(2, 3, true) == 1 && pann::grouped_row_cap(1000, 0, true) == 1000);
  }
  {   // F: one query whose entry allows nothing
    const V32 hist = {1}, allowed = {0};
    const GroupedPlan p(hist.data(), allowed.data(), 1, 1000, UINT64_MAX);
    CHECK(p.chunks.size() == 1 && p.chunks[0].ids == 0 && p.chunks[0].ntiles == 1 && p.chunks[0].na == 1);
    const Written w(p, allowed);
    CHECK((w.b_off(0) == V64{0, 0}) && (w.a_off(0) == V64{0, 1}) && (w.tile_seg(0) == V32{0}) && (w.tile_a0(0) == V32{0}));
  }
}

static void leaf_form() {      // the tile helper on absolute offsets (leaves of a tree): an empty segment yields no tile
  const V64 off = {0, 0, 64, 129};
  V32 seg = {9}, a0 = {9};
  pann::append_tiles(off.data(), 3, std::back_inserter(seg), std::back_inserter(a0));
  CHECK((seg == V32{9, 1, 2, 2}) && (a0 == V32{9, 0, 64, 128}));
  pann::append_tiles(off.data(), 1, std::back_inserter(seg), std::back_inserter(a0));
  CHECK(seg.size() == 4 && a0.size() == 4);
}

static void sweep() {
  std::mt19937_64 rng(20251);
  auto draw = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  for (int it = 0; it < 300; it++) {
    const uint64_t G = draw(1, 40);
    V32 hist(G), allowed(G);
    uint64_t total = 0;
    for (uint64_t g = 0; g < G; g++) {
      hist[g] = (uint32_t)(draw(0, 3) == 0 ? 0 : draw(0, 200)); allowed[g] = (uint32_t)(draw(0, 4) == 0 ? 0 : draw(0, 5000));
      total += allowed[g];
    }
    const uint64_t budget = it % 3 == 0 ? draw(1, 50) : it % 3 == 1 ? draw(1, total + 10) : total + draw(1, 100);
    const uint64_t row_cap = it % 4 == 0 ? draw(1, 5) : UINT64_MAX;
    const GroupedPlan p(hist.data(), allowed.data(), G, budget, row_cap);
    const size_t U = p.used.size();
    {   // used / first
      size_t u = 0; uint64_t run = 0;
      for (uint64_t g = 0; g < G; g++) if (hist[g]) { CHECK(u < U && p.used[u] == g && p.first[u] == run); run += hist[g]; u++; }
      CHECK(u == U && p.first.size() == U + 1 && p.first[U] == run);
    }
    const Written w(p, allowed);
    CHECK(w.used() == p.used);
    std::vector<std::pair<size_t, size_t>> spans = {{0, U * 4}};
    size_t next_u = 0, max_rows = 0, max_na = 0; uint64_t max_ids = 0;
    for (size_t ci = 0; ci < p.chunks.size(); ci++) {
      const GroupedChunk& c = p.chunks[ci];
      CHECK(c.u0 == next_u && c.u1 > c.u0 && c.u1 <= U);      // the chunks partition the used entries in order
      next_u = c.u1;
      const size_t S = c.u1 - c.u0;
      uint64_t ids = 0, big = 0; uint32_t ntiles = 0;
      for (size_t u = c.u0; u < c.u1; u++) { ids += allowed[p.used[u]]; big = std::max<uint64_t>(big, allowed[p.used[u]]); ntiles += (hist[p.used[u]] + 63) / 64; }
      CHECK(c.ids == ids && c.max_ids == big && c.ntiles == ntiles && c.a_base == p.first[c.u0] && c.na == p.first[c.u1] - c.a_base);
      if (S > 1) CHECK(ids <= budget && S <= row_cap);
      if (c.u1 < U) CHECK(ids + allowed[p.used[c.u1]] > budget || S >= row_cap);      // the next entry would not have fitted
      const V64 a = w.a_off(ci), b = w.b_off(ci);
      uint64_t ra = 0, rb = 0;
      for (size_t s = 0; s < S; s++) { CHECK(a[s] == ra && b[s] == rb); ra += hist[p.used[c.u0 + s]]; rb += allowed[p.used[c.u0 + s]]; }
      CHECK(a[S] == c.na && ra == c.na && b[S] == c.ids);
      const V32 seg = w.tile_seg(ci), a0 = w.tile_a0(ci);
      size_t t = 0;
      for (size_t s = 0; s < S; s++)
        for (uint64_t x = a[s]; x < a[s + 1]; x += 64, t++) CHECK(t < ntiles && seg[t] == s && a0[t] == x);
      CHECK(t == ntiles);
      for (size_t i = 1; i < seg.size(); i++) CHECK(seg[i - 1] <= seg[i]);
      spans.push_back({c.o_aoff, (S + 1) * 8}); spans.push_back({c.o_boff, (S + 1) * 8});
      spans.push_back({c.o_tseg, (size_t)ntiles * 4}); spans.push_back({c.o_ta0, (size_t)ntiles * 4});
      max_rows = std::max(max_rows, S); max_na = std::max<size_t>(max_na, c.na); max_ids = std::max(max_ids, ids);
    }
    CHECK(next_u == U && p.max_rows == max_rows && p.max_na == max_na && p.max_ids == max_ids);
    size_t end = 0;
    for (const auto& sp : spans) { CHECK(sp.first % 8 == 0 && sp.first >= end); end = sp.first + sp.second; }      // aligned, disjoint, in order
    CHECK(end <= p.plan_bytes);
  }
}

int main() {
  named_cases();
  leaf_form();
  sweep();
  printf("grouped_plan: ok\n");
  return 0;
}
