// host_staging_check.cpp -- parlayann_amd/csrc/host_staging.h on its own, built by a plain host compiler under sanitizers and run
// by tests/test_host_staging_cpu.py: the offsets of a packed region and the dropped-list growth policy against a fake launch.
#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <vector>

#include "../parlayann_amd/csrc/host_staging.h"

using pann::PackedLayout;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

struct Call { uint64_t q0, cnt; uint32_t dcap; };
static bool operator==(const Call& a, const Call& b) { return a.q0 == b.q0 && a.cnt == b.cnt && a.dcap == b.dcap; }

struct Run { int rc; uint32_t status; bool whole; uint32_t kept; std::string err; std::vector<Call> calls; };

// the policy with a launch that records its calls; word(call) = the status word that launch reports, rc(call) = its return code
static Run run(uint32_t kept, uint64_t n, uint64_t nq, int64_t limit, const std::function<uint32_t(const Call&)>& word,
               const std::function<int(const Call&)>& rc = [](const Call&) { return 0; }) {
  Run r{};
  r.kept = kept;
  r.rc = pann::run_with_dropped_growth(r.kept, n, nq, limit, "fake_entry", &r.status, &r.whole, &r.err,
                                       [&](uint64_t q0, uint64_t cnt, uint32_t dcap, uint32_t* st_word) -> int {
                                         const Call c{q0, cnt, dcap};
                                         r.calls.push_back(c);
                                         *st_word = word(c);
                                         return rc(c);
                                       });
  return r;
}

static void layout_checks() {
  uint8_t host[600], region[2048], back[600];
  for (int i = 0; i < 600; i++) host[i] = (uint8_t)(i * 7 + 1);
  {
    PackedLayout l;
    const int a = l.add(host, 1), b = l.add(host + 1, 256), c = l.add(host + 257, 257), d = l.add(host + 514, 0), e = l.add(nullptr, 64);
    CHECK(l.pc[a].off == 0 && l.pc[b].off == 256 && l.pc[c].off == 512 && l.pc[d].off == 1024 && l.pc[e].off == 1024);
    CHECK(l.total == 1024 && l.count == 5);
    CHECK(l.at(region, e) == nullptr && l.at(region, d) == nullptr);
    CHECK(l.at(region, a) == region && l.at(region, b) == region + 256 && l.at(region, c) == region + 512);
    memset(region, 0, sizeof region);
    l.copy(region, true);
    CHECK(region[0] == host[0] && region[1] == 0 && memcmp(region + 256, host + 1, 256) == 0 && memcmp(region + 512, host + 257, 257) == 0);
    // the way back: the same layout over another set of host arrays
    PackedLayout o;
    o.add(back, 1); o.add(back + 1, 256); o.add(back + 257, 257); o.add(back + 514, 0); o.add(nullptr, 64);
    memset(back, 0, sizeof back);
    o.copy(region, false);
    CHECK(memcmp(back, host, 514) == 0 && back[514] == 0);
  }
  {
    PackedLayout l;
    l.add(host, 100, 16);
    CHECK(l.pc[l.add(host, 4)].off == 256);
  }
  {
    PackedLayout l;
    l.add(host, 250, 16);
    CHECK(l.pc[l.add(host, 4)].off == 512 && l.total == 768);
  }
  {   // rows of a wider host table are packed densely: 3 rows of 8 bytes that lie 20 bytes apart
    PackedLayout l;
    l.add(host, 5);
    const int m = l.add_rows(host + 10, 3, 8, 20);
    CHECK(l.pc[m].off == 256 && l.pc[m].bytes == 24 && l.total == 512);
    l.copy(region, true);
    for (int r = 0; r < 3; r++) CHECK(memcmp(region + 256 + r * 8, host + 10 + r * 20, 8) == 0);
    CHECK(l.add_rows(nullptr, 3, 8, 20) == 2 && l.at(region, 2) == nullptr && l.total == 512);
  }
  {   // input, scratch and output pieces mixed: the scratch has room and an address, and no copy touches it or the gaps
    PackedLayout l;
    const int a = l.add(host, 10), s1 = l.add_scratch(300), e = l.add(nullptr, 64), b = l.add(host + 10, 257), s2 = l.add_scratch(1);
    CHECK(l.pc[a].off == 0 && l.pc[s1].off == 256 && l.pc[e].off == 768 && l.pc[b].off == 768 && l.pc[s2].off == 1280);
    for (int i = 0; i < l.count; i++) CHECK(l.pc[i].off % 256 == 0);
    CHECK(l.total == 1536 && l.host_end == 1280);      // the scratch counts; what a transfer must cover ends with the last host piece
    CHECK(l.end_of(1) == 256 && l.end_of(2) == 768 && l.end_of(l.count) == l.total);
    CHECK(l.at(region, s1) == region + 256 && l.at(region, s2) == region + 1280 && l.at(region, e) == nullptr);
    memset(region, 0xA5, sizeof region);
    l.copy(region, true);
    CHECK(memcmp(region, host, 10) == 0 && memcmp(region + 768, host + 10, 257) == 0);
    for (int i = 0; i < 2048; i++)
      if (!(i < 10 || (i >= 768 && i < 768 + 257))) CHECK(region[i] == 0xA5);
    // the way back, over host arrays of the same sizes: only the two host pieces arrive, the region is only read
    uint8_t was[2048];
    memcpy(was, region, sizeof was);
    PackedLayout o;
    o.add(back, 10); o.add_scratch(300); o.add(nullptr, 64); o.add(back + 10, 257); o.add_scratch(1);
    memset(back, 0x5A, sizeof back);
    o.copy(region, false);
    CHECK(memcmp(back, host, 267) == 0 && memcmp(region, was, sizeof was) == 0);
    for (int i = 267; i < 600; i++) CHECK(back[i] == 0x5A);
    // a range of pieces: the head alone, then the rest
    memset(back, 0x5A, sizeof back);
    o.copy(region, false, 0, 1);
    CHECK(memcmp(back, host, 10) == 0 && back[10] == 0x5A);
    o.copy(region, false, 1);
    CHECK(memcmp(back, host, 267) == 0);
    // an optional counter: a piece where the caller has an array, scratch where not -- room and an address either way
    PackedLayout c;
    CHECK(c.add_or_scratch(back, 40) == 0 && c.add_or_scratch(nullptr, 40) == 1);
    CHECK(c.total == 512 && c.host_end == 256 && c.at(region, 0) == region && c.at(region, 1) == region + 256);
  }
  {   // query rows as every upload takes them: host_stride > row_bytes, in an allocation that ends with the last row
    const size_t nq = 5, row = 24, stride = 64, extent = (nq - 1) * stride + row;
    uint8_t* q = (uint8_t*)malloc(extent);
    for (size_t i = 0; i < extent; i++) q[i] = (uint8_t)(i * 13 + 5);
    PackedLayout l;
    const int whole = l.add(q, extent, 16), rows = l.add_rows(q, nq, row, stride);
    CHECK(l.pc[whole].off == 0 && l.pc[rows].off == 512 && l.pc[rows].bytes == nq * row && l.total == 768);
    memset(region, 0xA5, sizeof region);
    l.copy(region, true);
    CHECK(memcmp(region, q, extent) == 0 && region[extent] == 0xA5);
    for (size_t r = 0; r < nq; r++) CHECK(memcmp(region + 512 + r * row, q + r * stride, row) == 0);
    CHECK(region[512 + nq * row] == 0xA5);
    free(q);
  }
  {   // direct pieces: a place in the region, no copy, no pinned room when they come last; rows of a table are never direct
    PackedLayout l;
    l.direct_from = 256;
    const int a = l.add(host, 100), rows = l.add_rows(host, 3, 100, 200), big = l.add(host + 300, 256, 16), e = l.add(nullptr, 4096);
    CHECK(!l.pc[a].direct && !l.pc[rows].direct && l.pc[big].direct && !l.pc[e].direct);
    CHECK(l.pc[big].off == 768 && l.total == 1280 && l.host_end == 768 && l.at(region, big) == region + 768);
    memset(region, 0xA5, sizeof region);
    l.copy(region, true);
    CHECK(memcmp(region, host, 100) == 0 && memcmp(region + 256, host, 100) == 0 && memcmp(region + 456, host + 400, 100) == 0);
    for (int i = 768; i < 2048; i++) CHECK(region[i] == 0xA5);
    uint8_t keep[600];
    memcpy(keep, host, sizeof keep);
    l.copy(region, false);                                   // the direct piece's host array is not written either
    CHECK(memcmp(keep + 300, host + 300, 256) == 0);
    // behind a direct piece a small one-row piece is direct too: the packed pieces stay a prefix that ends at host_end
    const int small = l.add(host, 8), tab = l.add_rows(host, 2, 8, 16), sc = l.add_scratch(8);
    CHECK(l.pc[small].direct && !l.pc[tab].direct && !l.pc[sc].direct && l.pc[small].off == 1280);
    PackedLayout f;                                          // small pieces first, as the callers add them: nothing pinned behind host_end
    f.direct_from = 256;
    f.add(host, 8); f.add(host, 300); f.add(host, 8);
    CHECK(f.host_end == 256 && f.total == 1024 && !f.pc[0].direct && f.pc[1].direct && f.pc[2].direct);
    PackedLayout packed;                                     // the default packs whatever the size
    CHECK(!packed.pc[packed.add(host, 600)].direct && packed.host_end == 768);
  }
  {   // a trip with nothing in it
    PackedLayout l;
    CHECK(l.total == 0 && l.host_end == 0 && l.end_of(0) == 0);
    l.add(nullptr, 100); l.add_rows(nullptr, 3, 8, 20); l.add(host, 0);
    CHECK(l.total == 0 && l.host_end == 0);
    memset(region, 0xA5, sizeof region);
    l.copy(region, true); l.copy(region, false);
    for (int i = 0; i < 2048; i++) CHECK(region[i] == 0xA5);
  }
}

static void growth_checks() {
  const uint32_t OVF = PANN_STATUS_DROPPED_OVERFLOW;
  const auto below700 = [&](const Call& c) { return c.dcap < 700 ? OVF : 0u; };
  {   // 1: grown once, one launch per pass
    const Run r = run(256, 1500, 3, 1500, below700);
    CHECK(r.rc == PANN_OK && r.err.empty());
    CHECK((r.calls == std::vector<Call>{{0, 3, 256}, {0, 3, 1536}}));
    CHECK(r.whole && r.status == 0 && r.kept == 1536);
  }
  {   // 2: the grown list of 100 000 queries is past the budget: two ranges
    const Run r = run(256, 1500, 100000, 1500, below700);
    CHECK(r.rc == PANN_OK);
    CHECK((r.calls == std::vector<Call>{{0, 100000, 256}, {0, 87381, 1536}, {87381, 100000 - 87381, 1536}}));
    CHECK(!r.whole && r.status == 0 && r.kept == 1536);
  }
  {   // 3: a list that overflows at its largest size
    const Run r = run(256, 1500, 3, 1500, [&](const Call&) { return OVF; });
    CHECK(r.rc == PANN_ERR_OVERFLOW && r.err == "fake_entry: internal dropped-list overflow");
    CHECK((r.calls == std::vector<Call>{{0, 3, 256}, {0, 3, 1536}}));
    CHECK(r.kept == 256);
  }
  {   // 4: an overflow in the first range ends that pass; the handle keeps at most 2048 entries
    const Run r = run(256, 1000000, 200000, 1000000, [&](const Call& c) { return c.dcap < 16384 ? OVF : 0u; });
    CHECK(r.rc == PANN_OK && !r.whole && r.status == 0 && r.kept == 2048);
    size_t at2048 = 0, at16384 = 0;
    for (const Call& c : r.calls) { at2048 += c.dcap == 2048; at16384 += c.dcap == 16384; }
    CHECK(r.calls[0] == (Call{0, 200000, 256}) && r.calls[1] == (Call{0, 65536, 2048}));
    CHECK(at2048 == 1 && r.calls[2] == (Call{0, 8192, 16384}));
    CHECK(at16384 == (200000 + 8191) / 8192 && r.calls.size() == 2 + at16384);
    uint64_t next = 0;                                     // the last pass covers every query once, in order
    for (size_t i = 2; i < r.calls.size(); i++) { CHECK(r.calls[i].q0 == next); next += r.calls[i].cnt; }
    CHECK(next == 200000);
  }
  {   // 5: a capacity below 64 is budgeted as 64 entries per query
    const Run r = run(8, 1500, 3000000, 1500, [](const Call&) { return 0u; });
    CHECK(r.rc == PANN_OK && !r.whole && r.kept == 8);
    CHECK((r.calls == std::vector<Call>{{0, 2097152, 8}, {2097152, 3000000 - 2097152, 8}}));
  }
  {   // 6: a launch's own error code ends the run
    const Run r = run(256, 1500, 3, 1500, below700, [](const Call& c) { return c.dcap > 256 ? PANN_ERR_HIP : 0; });
    CHECK(r.rc == PANN_ERR_HIP && r.err.empty() && r.kept == 256);
    CHECK((r.calls == std::vector<Call>{{0, 3, 256}, {0, 3, 1536}}));
  }
  {   // limit below n bounds the list; limit < 1 counts as 1
    const Run r = run(64, 1500, 3, 100, [&](const Call&) { return OVF; });
    CHECK(r.rc == PANN_ERR_OVERFLOW && r.calls.size() == 2 && r.calls[1].dcap == 128);
    const Run z = run(64, 1500, 3, 0, [&](const Call&) { return OVF; });
    CHECK(z.rc == PANN_ERR_OVERFLOW && z.calls.size() == 1);
  }
}

int main() {
  layout_checks();
  growth_checks();
  puts("host_staging: ok");
  return 0;
}
