// steer_plan_check.cpp -- the steered plans of parlayann_amd/csrc/search_plan.h on their own, built by a plain host compiler under
// sanitizers and run by tests/test_steer_plan_cpu.py.  Over a grid of (beam, max_deg, degree_limit, nstarts, row layout) a steered
// plan takes the generic kernel, its LDS regions -- the masked layout's and the bridge list behind it -- lie apart, aligned and
// inside the bytes the launch asks for, the total stays within 64 KB or the filter table has moved to HBM, and the candidate
// buffer covers the bound of DESIGN.md "Steered masked search": (beam/8 - 1) + (2 deg_eff - 1) entries at merge time, the start
// points before the first merge.  The region sizes are what the kernel indexes (beam_search.hip), written here a second time.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../parlayann_amd/csrc/search_plan.h"

using namespace pann;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (beam %d max_deg %u degree_limit %d nstarts %u dbytes %u masked %d)\n", \
  __FILE__, __LINE__, #cond, g_beam, g_deg, g_dl, g_ns, g_db, g_mode); exit(1); } } while (0)
static int g_beam, g_dl, g_mode;
static uint32_t g_deg, g_ns, g_db;

struct Region { const char* name; uint32_t off, bytes, align; };

static void check_regions(const std::vector<Region>& R, uint32_t total) {
  uint32_t end = 0;
  for (size_t i = 0; i < R.size(); i++) {
    CHECK(R[i].off % R[i].align == 0);
    CHECK((uint64_t)R[i].off + R[i].bytes <= total);
    end = std::max(end, R[i].off + R[i].bytes);
    for (size_t j = 0; j < i; j++)
      CHECK(R[i].bytes == 0 || R[j].bytes == 0 || R[i].off + R[i].bytes <= R[j].off || R[j].off + R[j].bytes <= R[i].off);
  }
  CHECK(end <= total && total - end < 16);      // the bridge list is padded to 16 bytes
}

// `steer_plan_check hbm_beam DBYTES MAX_DEG DEGREE_LIMIT NSTARTS`: the smallest beam whose steered plan keeps the filter table in HBM
// (tests/test_steered_gpu.py takes the beam of its HBM-table case from here)
static int hbm_beam(char** v) {
  PlanIndex ix{};
  ix.dtype = PANN_U8; ix.metric = PANN_L2; ix.max_deg = (uint32_t)atoi(v[1]); ix.gstride = (ix.max_deg + 15) / 16 * 16; ix.n = 3000;
  choose_point_layout((uint32_t)atoi(v[0]), 0, &ix.lpc, &ix.nch);
  for (int beam = std::max(1, atoi(v[3])); beam <= 4096; beam++) {
    PlanCall a{64, (uint32_t)atoi(v[3]), std::min(10, beam), beam, atoi(v[2]), 1.35, 256, false, MASK_BITMAP};
    a.steer = true;
    if (make_plan(ix, a).table == TABLE_HBM) { printf("%d\n", beam); return 0; }
  }
  return 1;
}

int main(int argc, char** argv) {
  if (argc == 6 && std::string(argv[1]) == "hbm_beam") return hbm_beam(argv + 2);
  if (argc != 1) { fprintf(stderr, "usage: steer_plan_check [hbm_beam DBYTES MAX_DEG DEGREE_LIMIT NSTARTS]\n"); return 2; }
  long plans = 0, in_hbm = 0, in_lds = 0;
  const uint32_t dbytes_of[] = {32, 64, 100, 128, 192, 256, 384, 400, 512, 800, 1024};      // every row layout: lpc 4 / 8 / 16 / 32, one and several chunks
  const int beams[] = {1, 2, 7, 8, 9, 31, 32, 63, 64, 65, 90, 91, 100, 127, 128, 129, 181, 182, 200, 255, 256, 257, 300};
  for (int beam : beams) for (uint32_t max_deg : {8u, 16u, 30u, 32u, 64u, 80u, 96u, 128u})
    for (int dl : {1, 5, (int)max_deg / 2, (int)max_deg, (int)max_deg + 40}) for (uint32_t nstarts : {1u, 3u, 64u, 70u})
      for (uint32_t dbytes : dbytes_of) for (int masked : {MASK_BITMAP, MASK_LABELS}) {
        if ((int)nstarts > beam) continue;
        g_beam = beam; g_deg = max_deg; g_dl = dl; g_ns = nstarts; g_db = dbytes; g_mode = masked;
        PlanIndex ix{};
        ix.dtype = PANN_U8; ix.metric = PANN_L2; ix.max_deg = max_deg; ix.gstride = (max_deg + 15) / 16 * 16; ix.n = 1000000;
        choose_point_layout(dbytes, 0, &ix.lpc, &ix.nch);
        PlanCall a{10000, nstarts, std::min(10, beam), beam, dl, 1.35, 256, false, masked};
        const SearchPlan m = make_plan(ix, a);      // the masked twin: untouched by the steer request
        a.steer = true;
        const SearchPlan p = make_plan(ix, a);
        plans++;
        CHECK(!m.steer && m.br_off == 0 && p.steer && p.kernel == KERNEL_GENERIC && p.masked() && (p.table == TABLE_LDS || p.table == TABLE_HBM));
        CHECK(p.bits == m.bits && p.bcap == m.bcap && p.deg_eff == m.deg_eff && p.deg_eff == (uint32_t)std::min<int>(dl, (int)max_deg));
        CHECK(p.bcap % 64 == 0 && p.bcap >= 64 && p.bcap >= (uint32_t)beam && p.bcap >= nstarts);
        // 3. the candidate buffer
        CHECK(p.ccap % 64 == 0 && p.ccap >= (uint32_t)beam / 8 + 2 * p.deg_eff && p.ccap >= nstarts);
        CHECK(p.ccap < std::max<uint32_t>((uint32_t)beam / 8 + 2 * p.deg_eff, nstarts) + 64);      // rounded to 64, no further
        // 1. the regions
        const uint32_t qb = query_lds_bytes(ix.lpc, ix.nch);
        const bool lds = p.table == TABLE_LDS;
        const SteerLds L = steered_lds(p.bcap, p.ccap, qb, p.bits, lds, p.deg_eff);
        CHECK(L.total == p.lds_bytes && L.g.tail == p.rl_off && L.br == p.br_off && p.rl_off + RESULT_LIST_BYTES == p.br_off);
        check_regions({{"F", L.g.F, p.bcap * 8, 8}, {"NF", L.g.NF, p.bcap * 8, 8}, {"C", L.g.C, p.ccap * 8, 8}, {"Fv", L.g.Fv, p.bcap, 1},
                       {"NFv", L.g.NFv, p.bcap, 1}, {"CP", L.g.CP, p.ccap * 2, 2}, {"query", L.g.q, qb, 16},
                       {"H or T", L.g.H, lds ? 4u << p.bits : 1024u, 4}, {"result list and gather keys", L.g.tail, 1024u, 16},
                       {"bridges", L.br, p.deg_eff * 4, 16}}, L.total);
        CHECK(L.g.Pl == L.g.NF && p.bcap * 8 >= 128 * 4);      // the pending survivors: 128 ids in NF (or F, when the two have swapped)
        // 2. within 64 KB, or the table is in HBM -- and in LDS whenever that fits
        const uint32_t with_table = steered_lds(p.bcap, p.ccap, qb, p.bits, true, p.deg_eff).total;
        CHECK(lds == (p.bits <= 12 && with_table <= 64 * 1024));
        CHECK(p.lds_bytes <= 64 * 1024 && p.persistent() == !lds);
        CHECK(p.ws_bytes == 256 + 10000ull * p.dcap * 8 + (lds ? 0 : (std::min<uint64_t>(10000, p.slots) << p.bits) * 4));
        (lds ? in_lds : in_hbm)++;
      }
  CHECK(in_lds > 0 && in_hbm > 0);
  // named: beam 64, degree 64, 128-byte rows in registers -- 8 + 128 candidates -> 192; bridges behind the 1 KB list
  {
    PlanIndex ix{}; ix.dtype = PANN_F16; ix.max_deg = 64; ix.gstride = 64; ix.n = 1000000; choose_point_layout(256, 0, &ix.lpc, &ix.nch);
    PlanCall a{10000, 1, 10, 64, 64, 1.35, 256, false, MASK_BITMAP}; a.steer = true;
    const SearchPlan p = make_plan(ix, a);
    CHECK(p.ccap == 192 && p.bcap == 64 && p.table == TABLE_LDS && p.lds_bytes == 512 + 512 + 1536 + 128 + 384 + 4096 + 1024 + 256);
  }
  printf("steer_plan: ok, %ld plans (%ld with the table in LDS, %ld in HBM)\n", plans, in_lds, in_hbm);
  return 0;
}
