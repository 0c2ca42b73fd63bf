// search_plan_check.cpp -- parlayann_amd/csrc/search_plan.h on its own, built by a plain host compiler under sanitizers and run by
// tests/test_search_plan_cpu.py with the path of tests/golden/search_plans_v1.txt: for every recorded row make_plan decides what
// beam_search.hip decided before the plan moved into the header, and the LDS layouts of the three kernel families keep their
// regions apart, aligned and inside the bytes the launch asks for.  The region sizes below are what the kernels index
// (beam_search.hip), written here a second time on purpose: the header is held against them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../parlayann_amd/csrc/search_plan.h"

using namespace pann;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (table line %d)\n", __FILE__, __LINE__, #cond, g_line); exit(1); } } while (0)
static int g_line = 0;

struct Region { const char* name; uint32_t off, bytes, align; };

// pairwise disjoint, aligned, inside `total`, and `total` ends with the last region
static void check_regions(const std::vector<Region>& R, uint32_t total) {
  uint32_t end = 0;
  for (size_t i = 0; i < R.size(); i++) {
    CHECK(R[i].off % R[i].align == 0);
    CHECK((uint64_t)R[i].off + R[i].bytes <= total);
    end = std::max(end, R[i].off + R[i].bytes);
    for (size_t j = 0; j < i; j++)
      CHECK(R[i].bytes == 0 || R[j].bytes == 0 || R[i].off + R[i].bytes <= R[j].off || R[j].off + R[j].bytes <= R[i].off);
  }
  CHECK(end == total);
}
// an alias named by the layout lies inside the region it borrows
static void check_alias(uint32_t off, uint32_t bytes, uint32_t align, uint32_t host_off, uint32_t host_bytes) {
  CHECK(off % align == 0 && off >= host_off && off + bytes <= host_off + host_bytes);
}

static void check_generic(uint32_t bcap, uint32_t ccap, uint32_t qb, uint32_t bits, bool lds, bool masked, uint32_t sk) {
  const GenericLds L = generic_lds(bcap, ccap, qb, bits, lds, masked, sk);
  check_regions({{"F", L.F, bcap * 8, 8}, {"NF", L.NF, bcap * 8, 8}, {"C", L.C, ccap * 8, 8}, {"Fv", L.Fv, bcap, 1}, {"NFv", L.NFv, bcap, 1},
                 {"CP", L.CP, ccap * 2, 2}, {"query", L.q, qb, 16}, {"H or T", L.H, lds ? 4u << bits : 1024u, 4},
                 {"result list or sketch", L.tail, masked ? 1024u : sk, 16}}, L.total);
  check_alias(L.Pl, 256, 4, L.NF, bcap * 8);      // Pl, 64 ids, at the head of NF
  check_alias(L.F + (L.Pl - L.NF), 256, 4, L.F, bcap * 8);      // ... or of F, when the two have swapped
}
static void check_b64(uint32_t ccap, uint32_t qb, uint32_t bits, uint32_t seen_n, bool masked) {
  const RegLds L = b64_lds(ccap, qb, bits, seen_n, masked);
  check_regions({{"S", L.S, 512, 8}, {"C", L.C, ccap * 8, 8}, {"Sv", L.Sv, 64, 1}, {"query", L.q, qb, 16}, {"H", L.H, 4u << bits, 4},
                 {"V", L.V, seen_n * 2, 4}, {"result list", L.rl, masked ? 1024u : 0u, 16}}, L.total);
  check_alias(L.Pl, 256, 4, L.S, 512);
}
static void check_b128(uint32_t ccap, uint32_t qb, uint32_t bits, int table, uint32_t hsplit, uint32_t p24) {
  const RegLds L = b128_lds(ccap, qb, bits, table, hsplit, p24);
  const uint32_t hsize = 1u << bits, slots = hsplit == 3 ? hsize : hsplit ? hsize - hsize / (1u << hsplit) : 0;
  const uint32_t hbytes = table == TABLE_LDS ? hsize * 4 : table == TABLE_CODES ? hsize + hsize / 2 : table == TABLE_HBM_SPLIT ? slots * (p24 ? 3 : 4) : 0;
  check_regions({{"S", L.S, 1024, 8}, {"C", L.C, ccap * 8, 8}, {"Sv", L.Sv, 128, 1}, {"query", L.q, qb, 16}, {"H", L.H, hbytes, 4}}, L.total);
  check_alias(L.Pl, 256, 4, L.S, 1024);
  check_alias(L.T, 1024, 1, L.S, 1024);      // the 1 KB replay scratch
  CHECK(table_lds_bytes(table, bits, hsplit, p24) == hbytes && hbytes % 4 == 0);      // lds_part_clear and the code table clear whole dwords
}

// the ten kernels a plan can ask for, as the recorder numbers them
static int choice_of(const SearchPlan& p) {
  if (p.mode == MODE_SKETCH) return 0;
  if (p.masked()) return p.kernel == KERNEL_B64 ? 1 : 2;
  if (p.kernel == KERNEL_B64) return p.mode == MODE_PLAIN_V ? 3 : 4;
  if (p.kernel == KERNEL_B128) return p.table == TABLE_CODES ? 5 : p.persistent() ? 6 : 7;
  return p.table == TABLE_LDS ? 8 : 9;
}

static void named_cases() {
  // the benchmark's shape (beam 64, degree 64, 128-byte rows in registers): 72 candidates, 5 248 B, with V 6 272 B
  CHECK(b64_lds(72, 0, 10, 0, false).total == 512 + 576 + 64 + 4096 && b64_lds(72, 0, 10, 512, false).total == 6272);
  CHECK(b64_lds(72, 0, 10, 0, true).rl == 5248 && b64_lds(72, 0, 10, 0, true).total == 6272);
  // beam 128, degree 64: 80 candidates; the 16 KB table, 6 KB of codes, half of the table as 24-bit planes
  CHECK(b128_lds(80, 0, 12, TABLE_LDS, 0, 0).total == 1024 + 640 + 128 + 16384);
  CHECK(b128_lds(80, 0, 12, TABLE_CODES, 0, 0).total == 1792 + 6144 && b128_lds(80, 0, 12, TABLE_HBM_SPLIT, 1, 1).total == 1792 + 6144);
  CHECK(b128_lds(80, 0, 12, TABLE_HBM, 0, 0).total == 1792 && b128_lds(80, 0, 12, TABLE_HBM_SPLIT, 2, 0).total == 1792 + 3072 * 4);
  // generic, beam 100 from 70 starts, 64-byte rows in LDS
  const GenericLds g = generic_lds(128, 128, 64, 12, true, true, 0);
  CHECK(g.NF == 1024 && g.C == 2048 && g.Fv == 3072 && g.NFv == 3200 && g.CP == 3328 && g.q == 3584 && g.H == 3648 && g.tail == 20032 && g.total == 21056);
  uint32_t lpc, nch;
  choose_point_layout(384, 0, &lpc, &nch); CHECK(lpc == 8 && nch == 3);
  choose_point_layout(100, 0, &lpc, &nch); CHECK(lpc == 8 && nch == 1 && layout_query_in_registers(lpc, nch) && query_lds_bytes(lpc, nch) == 0);
  choose_point_layout(64, 0, &lpc, &nch); CHECK(lpc == 4 && nch == 1 && query_lds_bytes(lpc, nch) == 64);
  choose_point_layout(512, 4, &lpc, &nch); CHECK(lpc == 4 && nch == 8);
  CHECK(filter_bits(64) == 10 && filter_bits(90) == 11 && filter_bits(91) == 12 && filter_bits(128) == 12 && filter_bits(129) == 13);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: search_plan_check TABLE\n"); return 2; }
  named_cases();
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  char head[1024];
  CHECK(fgets(head, sizeof head, f) && std::string(head).rfind("# dtype metric dbytes max_deg n codes b64_seen sk_stride nq nstarts k beam degree_limit "
        "cut_sign dcap filter masked sw_b128_lds sw_b128_split sw_b128_no24 sw_b64_seen sw_force_lpc choice bits bcap ccap deg_eff dcap_out "
        "lds_bytes hash_lds slots hsplit p24 sk_lds_off rl_off seen_n ws_bytes lpc nch", 0) == 0);
  int rows = 0, seen_choice[10] = {0};
  long long v[39];
  for (g_line = 2;; g_line++) {
    int got = 0;
    while (got < 39 && fscanf(f, "%lld", &v[got]) == 1) got++;
    if (got == 0) break;
    CHECK(got == 39);
    PlanSwitches sw;
    sw.b128_lds = v[17] != 0; sw.b128_split = (uint32_t)v[18]; sw.b128_no24 = v[19] != 0; sw.b64_seen = (int)v[20]; sw.force_lpc = (uint32_t)v[21];
    PlanIndex ix{};
    ix.dtype = (int)v[0]; ix.metric = (int)v[1]; ix.max_deg = (uint32_t)v[3]; ix.gstride = (ix.max_deg + 15) / 16 * 16; ix.n = (uint64_t)v[4];
    ix.codes = v[5] != 0; ix.b64_seen = (uint32_t)v[6]; ix.sk_stride = (uint32_t)v[7];
    choose_point_layout((uint32_t)v[2], sw.force_lpc, &ix.lpc, &ix.nch);
    const PlanCall a{(uint64_t)v[8], (uint32_t)v[9], v[10], v[11], v[12], 1.35 * (double)v[13], (uint32_t)v[14], v[15] != 0, (int)v[16]};
    const SearchPlan p = make_plan(ix, a, sw);
    const long long* o = v + 22;
    CHECK(choice_of(p) == o[0] && p.bits == o[1] && p.bcap == o[2] && p.ccap == o[3] && p.deg_eff == o[4] && p.dcap == o[5]);
    CHECK(p.lds_bytes == o[6] && p.table_in_lds() == (o[7] != 0) && p.slots == o[8] && p.hsplit == o[9] && p.p24 == o[10]);
    CHECK(p.sk_lds_off == o[11] && p.rl_off == o[12] && p.seen_n == o[13] && p.ws_bytes == (uint64_t)o[14] && ix.lpc == o[15] && ix.nch == o[16]);
    CHECK(p.persistent() == !p.table_in_lds() && (p.table != TABLE_HBM_SPLIT || p.hsplit) && (p.mode == MODE_PLAIN_V) == (p.seen_n != 0));
    seen_choice[o[0]]++; rows++;
    // the layouts: the planned family as planned, and every family over the variants this row's sizes allow
    const uint32_t qb = query_lds_bytes(ix.lpc, ix.nch), tb = std::min<uint32_t>(p.bits, 12);      // a table in LDS has at most 4 096 slots
    for (int masked = 0; masked < 2; masked++) {
      for (int lds = 0; lds < 2; lds++)
        for (uint32_t sk : {0u, 16u, ix.sk_stride}) if (!(masked && sk)) check_generic(p.bcap, p.ccap, qb, lds ? tb : p.bits, lds != 0, masked != 0, sk);
      for (uint32_t seen_n : {0u, B64_SEEN_N}) if (!(masked && seen_n)) check_b64(p.ccap, qb, tb, seen_n, masked != 0);
    }
    for (int table : {TABLE_LDS, TABLE_HBM, TABLE_CODES}) check_b128(p.ccap, qb, tb, table, 0, 0);
    for (uint32_t hs = 1; hs <= 3; hs++) for (uint32_t p24 = 0; p24 < 2; p24++) check_b128(p.ccap, qb, tb, TABLE_HBM_SPLIT, hs, p24);
    if (p.kernel == KERNEL_GENERIC) {
      const GenericLds L = generic_lds(p.bcap, p.ccap, qb, p.bits, p.table_in_lds(), p.masked(), a.filter ? ix.sk_stride : 0);
      CHECK(L.total == p.lds_bytes && (!p.masked() || L.tail == p.rl_off) && (!a.filter || L.tail == p.sk_lds_off));
    } else if (p.kernel == KERNEL_B64) {
      const RegLds L = b64_lds(p.ccap, qb, p.bits, p.seen_n, p.masked());
      CHECK(L.total == p.lds_bytes && (!p.masked() || L.rl == p.rl_off) && p.bits <= 12);
    } else {
      CHECK(b128_lds(p.ccap, qb, p.bits, p.table, p.hsplit, p.p24).total == p.lds_bytes && p.bits <= 12);
    }
  }
  fclose(f);
  for (int c = 0; c < 10; c++) CHECK(seen_choice[c] > 0);
  printf("search_plan: ok, %d rows\n", rows);
  return 0;
}
