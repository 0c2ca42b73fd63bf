// search_plan.h -- the host arithmetic of the beam search (beam_search.hip): the point layout, the LDS layout of the three kernel
// families, and the plan of one launch.  The host sizes every launch with the layout functions; the kernels carve the same regions in
// the same order by typed pointer steps (any other form costs them their machine code: DESIGN.md section 4).  No HIP and nothing of
// pann_internal.h in here: tests/test_search_plan_cpu.py builds it with a plain host compiler, under sanitizers.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include "../../include/pann.h"

namespace pann {
constexpr uint32_t B64_SEEN_N = 512;        // entries of the beam-64 search's second-sighting table ("Second sightings")
constexpr uint32_t FILTER_CODE_BITS = 12;   // the table size the filter codes are made for: beam 91..128 (beamSearch.h:52)
// how a masked search decides whether a compared point is allowed (SearchArgs::masked; template parameter of the kernels)
enum { MASK_NONE = 0, MASK_BITMAP = 1, MASK_LABELS = 2 };

// Lanes-per-candidate and chunks-per-lane for a row of dbytes.  One chunk (query in registers) whenever the row is 128/256/512 B
// after padding to 16*LPC; otherwise LPC=4 (64-B granules, the reference's own row alignment, point_range.h:94) or LPC=16 for
// long rows.  force_lpc (PlanSwitches): lanes per candidate 4 / 8 / 16 where the row allows it.
inline void choose_point_layout(uint32_t dbytes, uint32_t force_lpc, uint32_t* lpc, uint32_t* nch) {
  const uint32_t r64 = (dbytes + 63) / 64 * 64, l = force_lpc;
  if ((l == 4 || l == 8 || l == 16) && r64 % (l * 16) == 0 && r64 / (l * 16) > 1) { *lpc = l; *nch = r64 / (l * 16); return; }
  if (r64 == 128) { *lpc = 8; *nch = 1; return; }
  if (r64 == 256) { *lpc = 16; *nch = 1; return; }
  if (r64 == 512) { *lpc = 32; *nch = 1; return; }
  if (r64 % 256 == 0) { *lpc = 16; *nch = r64 / 256; return; }
  if (r64 % 128 == 0) { *lpc = 8; *nch = r64 / 128; return; }      // e.g. f32 d=96: 384 B = 3 chunks of 8 lanes x 16 B
  *lpc = 4; *nch = r64 / 64;
}
// The kernels come in two families (PANN_LAYOUT_SWITCH): rows that are ONE 16-byte chunk per lane with 8 / 16 / 32 lanes per
// candidate keep the query in registers; every other layout -- including 64-byte rows, lpc 4 / nch 1 -- runs the generic
// variants, which keep the query in LDS.  All LDS sizes on the host must use THIS predicate.
constexpr bool layout_query_in_registers(uint32_t lpc, uint32_t nch) { return nch == 1 && lpc != 4; }
constexpr uint32_t query_lds_bytes(uint32_t lpc, uint32_t nch) { return layout_query_in_registers(lpc, nch) ? 0u : nch * lpc * 16u; }

// ---- LDS layouts: byte offsets of every region from the start of the dynamic LDS, and the bytes to launch with ----
enum { TABLE_LDS, TABLE_HBM, TABLE_HBM_SPLIT, TABLE_CODES };      // where the filter table H lives; HBM_SPLIT: HBM with an LDS share
constexpr uint32_t REPLAY_BYTES = 1024;         // T, the byte scratch of filter_update's replay when the table is not in LDS
constexpr uint32_t RESULT_LIST_BYTES = 1024;    // masked: the result list (64 keys), then the keys of one gather (64)
constexpr uint32_t align16(uint32_t x) { return (x + 15u) & ~15u; }
// bytes of H in LDS.  Code table: an 8-bit plane of 1 << bits bytes, then the 4-bit plane, eight slots per dword.  Split table (hsplit
// 1 / 2: half / three quarters of the slots in LDS, 3: all of them): entries of 3 (p24) or 4 bytes.  (A b64 table is always TABLE_LDS.)
constexpr uint32_t table_lds_bytes(int table, uint32_t bits, uint32_t hsplit, uint32_t p24) {
  const uint32_t hsize = 1u << bits, split_slots = hsplit == 3 ? hsize : hsplit ? hsize - (hsize >> hsplit) : 0u;
  return table == TABLE_LDS ? 4u * hsize : table == TABLE_CODES ? hsize + hsize / 2 : table == TABLE_HBM_SPLIT ? split_slots * (p24 ? 3u : 4u) : 0u;
}
// generic kernel: F[bcap] NF[bcap] C[ccap] keys | Fv[bcap] NFv[bcap] flags | CP[ccap] uint16 | query | H: the table, or T when the
// table is in HBM | tail: the result list (masked) or the query sketch (sk_stride bytes).  Pl, the 64 filter survivors of one row
// chunk, aliases the head of the merge output, which is NF (as named here) and F by turns.
struct GenericLds { uint32_t F, NF, C, Fv, NFv, CP, q, H, tail, total, Pl; };
constexpr GenericLds generic_lds(uint32_t bcap, uint32_t ccap, uint32_t qbytes, uint32_t bits, bool table_in_lds, bool masked, uint32_t sk_stride) {
  GenericLds L{};
  L.NF = L.F + bcap * 8; L.C = L.NF + bcap * 8; L.Fv = L.C + ccap * 8; L.NFv = L.Fv + bcap; L.CP = L.NFv + bcap; L.q = L.CP + ccap * 2; L.H = L.q + qbytes;
  const uint32_t end = L.H + (table_in_lds ? 4u << bits : REPLAY_BYTES), tail_bytes = masked ? RESULT_LIST_BYTES : sk_stride;
  L.tail = align16(end); L.total = tail_bytes ? L.tail + tail_bytes : end; L.Pl = L.NF;
  return L;
}
// register-frontier kernels, nf = 64 (beam <= 64) or 128 entries: S[nf] merge scatter scratch | C[ccap] | Sv[nf] flags of S | query |
// H: table_bytes of table | V[seen_n] uint16 | rl: the result list (masked).  Pl and T alias S, which is idle outside the merge.
struct RegLds { uint32_t S, C, Sv, q, H, V, rl, total, Pl, T; };
constexpr RegLds reg_lds(uint32_t nf, uint32_t ccap, uint32_t qbytes, uint32_t table_bytes, uint32_t seen_n, bool masked) {
  RegLds L{};
  L.C = L.S + nf * 8; L.Sv = L.C + ccap * 8; L.q = L.Sv + nf; L.H = L.q + qbytes; L.V = L.H + table_bytes;
  const uint32_t end = L.V + seen_n * 2;
  L.rl = align16(end); L.total = masked ? L.rl + RESULT_LIST_BYTES : end; L.Pl = L.T = L.S;
  return L;
}
// steered generic kernel (masked modes only; DESIGN.md "Steered masked search"): the masked layout, then BR, the bridge list of one
// visit: deg_eff ids behind the result list.  Between merges the whole of NF (>= 512 B) holds the pending survivors, 128 ids.
struct SteerLds { GenericLds g; uint32_t br, total; };
constexpr SteerLds steered_lds(uint32_t bcap, uint32_t ccap, uint32_t qbytes, uint32_t bits, bool table_in_lds, uint32_t deg_eff) {
  SteerLds L{generic_lds(bcap, ccap, qbytes, bits, table_in_lds, true, 0), 0, 0};
  L.br = L.g.total; L.total = L.br + align16(deg_eff * 4);
  return L;
}
constexpr RegLds b64_lds(uint32_t ccap, uint32_t qbytes, uint32_t bits, uint32_t seen_n, bool masked) { return reg_lds(64, ccap, qbytes, 4u << bits, seen_n, masked); }
constexpr RegLds b128_lds(uint32_t ccap, uint32_t qbytes, uint32_t bits, int table, uint32_t hsplit, uint32_t p24) {
  static_assert(REPLAY_BYTES <= 128 * 8, "T fits S");
  return reg_lds(128, ccap, qbytes, table_lds_bytes(table, bits, hsplit, p24), 0, false);
}

// ---- the plan of one launch: three exclusive choices (the dispatch is a switch over them), sizes, the layout's bytes ----
enum { KERNEL_GENERIC, KERNEL_B64, KERNEL_B128 };      // frontier in LDS (any beam) | in registers | two entries per lane
enum { MODE_PLAIN, MODE_PLAIN_V, MODE_SKETCH, MODE_BITMAP, MODE_LABELS };      // PLAIN_V: with the second-sighting table V
struct SearchPlan {
  int kernel, table, mode;
  uint32_t bits, bcap, ccap, deg_eff;      // log2 of the filter size (:52); LDS capacities of frontier and candidates; min(degree_limit, max_deg)
  uint32_t dcap, slots, hsplit, p24, seen_n;      // dropped-list entries per query; blocks of a persistent launch; HBM_SPLIT: LDS share, 24-bit planes; entries of V
  uint32_t lds_bytes, sk_lds_off, rl_off;      // of the kernel's layout: total, and the tail of the sketch / masked modes
  uint32_t br_off = 0; bool steer = false;     // steered masked search: the bridge list's offset (always KERNEL_GENERIC)
  uint64_t ws_bytes;             // 256 (counter, status) | dropped_bytes | the tables of a persistent launch
  bool table_in_lds() const { return table == TABLE_LDS || table == TABLE_CODES; }
  bool persistent() const { return !table_in_lds(); }      // every kernel whose table is in HBM is persistent, and no other
  bool masked() const { return mode == MODE_BITMAP || mode == MODE_LABELS; }
  uint64_t dropped_bytes(uint64_t nq) const { return nq * dcap * 8; }
};
struct PlanIndex { int dtype, metric; uint32_t lpc, nch, max_deg, gstride; uint64_t n; uint32_t sk_stride, b64_seen; bool codes; };
struct PlanCall { uint64_t nq; uint32_t nstarts; int64_t k, beam, degree_limit; double cut; uint32_t dcap; bool filter; int masked;
                  bool steer = false; };      // steer: the steered form of a masked call (no sketch filter)
// Diagnostic A/B switches of `make alt` builds (beam_search.hip reads them from the environment); the shipped library runs on these defaults
struct PlanSwitches {
  bool b128_lds = false, b128_no24 = false;      // PANN_B128_LDS: never the HBM table; PANN_B128_NO24: no 24-bit planes
  uint32_t b128_split = 1, force_lpc = 0;        // PANN_B128_SPLIT: hsplit of the HBM table (above 3: 0); PANN_FORCE_LPC
  int b64_seen = -1;                             // PANN_B64_SEEN: 0 the kernel without V, 1 with it; -1: as the index says
};
inline uint32_t filter_bits(int64_t beam) {  // :52
  const int b = (int)(std::ceil(std::log2((double)beam * (double)beam)) - 2.0);
  return (uint32_t)(b < 10 ? 10 : b);
}
// Which layouts have a MASKED instantiation of the b64 kernel: 128-byte rows (8 lanes per candidate) and bf16 rows of several chunks
// per lane would spill under its 72-VGPR bound (DESIGN.md "Masked search") and take the generic kernel.  The label form needs no
// vector register beyond the bitmap form (MaskSrc), so one predicate serves both.
constexpr bool masked_b64_fits(int dtype, uint32_t lpc, bool nch1) { return !(lpc == 8 && nch1) && !(dtype == PANN_BF16 && !nch1); }
inline SearchPlan make_plan(const PlanIndex& ix, const PlanCall& a, const PlanSwitches& sw = PlanSwitches()) {
  SearchPlan p{};
  const uint32_t beam = (uint32_t)a.beam, qb = query_lds_bytes(ix.lpc, ix.nch);
  p.bits = filter_bits(a.beam);
  p.bcap = (std::max<uint32_t>(beam, a.nstarts) + 63) / 64 * 64;
  p.deg_eff = (uint32_t)std::min<int64_t>(std::max<int64_t>(a.degree_limit, 0), (int64_t)ix.max_deg);
  // at merge time |C| <= (beam/8 - 1) + deg_eff (accumulation stops at beam/8); starts first
  const uint32_t cmax = std::max<uint32_t>(beam / 8 + p.deg_eff, a.nstarts);
  p.ccap = (cmax + 63) / 64 * 64;
  p.dcap = std::max<uint32_t>(a.dcap, 64); p.slots = 256 * 8;
  p.mode = a.filter ? MODE_SKETCH : a.masked == MASK_BITMAP ? MODE_BITMAP : a.masked == MASK_LABELS ? MODE_LABELS : MODE_PLAIN;
  if (a.steer) {
    // steered: |pruned| <= fill - 1 + deg_eff <= 2 deg_eff - 1 per visit, so |C| <= (beam/8 - 1) + 2 deg_eff - 1 at merge time; the
    // table's place is decided with the steered layout's bytes
    p.steer = true; p.kernel = KERNEL_GENERIC;
    p.ccap = (std::max<uint32_t>(beam / 8 + 2 * p.deg_eff, a.nstarts) + 63) / 64 * 64;
    const bool sfits = p.bits <= 12 && steered_lds(p.bcap, p.ccap, qb, p.bits, true, p.deg_eff).total <= 64 * 1024;
    p.table = sfits ? TABLE_LDS : TABLE_HBM;
    const SteerLds L = steered_lds(p.bcap, p.ccap, qb, p.bits, sfits, p.deg_eff);
    p.lds_bytes = L.total; p.rl_off = L.g.tail; p.br_off = L.br;
    p.ws_bytes = 256 + p.dropped_bytes(a.nq) + (p.persistent() ? (std::min<uint64_t>(a.nq, p.slots) << p.bits) * 4 : 0);
    return p;
  }
  // the table goes to LDS up to 16 KB, if the generic kernel's state with it stays within 64 KB
  const bool fits = p.bits <= 12 && generic_lds(p.bcap, p.ccap, qb, p.bits, true, false, 0).total <= 64 * 1024;
  // the register-frontier kernels: no sketch form; masked forms of b64 only, and not for every layout
  const bool regs = fits && (p.mode == MODE_PLAIN || (p.masked() && masked_b64_fits(ix.dtype, ix.lpc, layout_query_in_registers(ix.lpc, ix.nch))));
  p.kernel = regs && p.bcap == 64 ? KERNEL_B64 : regs && p.bcap == 128 && a.nstarts <= 64 && !p.masked() ? KERNEL_B128 : KERNEL_GENERIC;
  p.table = fits ? TABLE_LDS : TABLE_HBM;
  if (p.kernel != KERNEL_GENERIC) p.ccap = (cmax + 7) / 8 * 8;      // exact, 8-entry granules
  if (p.kernel == KERNEL_GENERIC) {
    const GenericLds L = generic_lds(p.bcap, p.ccap, qb, p.bits, fits, p.masked(), a.filter ? ix.sk_stride : 0);
    p.lds_bytes = L.total; p.rl_off = p.masked() ? L.tail : 0; p.sk_lds_off = a.filter ? L.tail : 0;
  } else if (p.kernel == KERNEL_B64) {
    // Second-sighting table (plain search): its 16-bit tags id >> log2(B64_SEEN_N) stay below the empty value 0xFFFF up
    // to n = 0xFFFF * B64_SEEN_N points, and it needs a cut-prune threshold that is monotone in the distance (no negative or NaN `cut`)
    const bool seen = sw.b64_seen >= 0 ? sw.b64_seen != 0 : ix.b64_seen != 0, cut_monotone = !(a.k > 0 && ix.metric == PANN_L2) || a.cut >= 0.0;
    if (p.mode == MODE_PLAIN && seen && cut_monotone && ix.n <= (uint64_t)0xFFFF * B64_SEEN_N) { p.mode = MODE_PLAIN_V; p.seen_n = B64_SEEN_N; }
    const RegLds L = b64_lds(p.ccap, qb, p.bits, p.seen_n, p.masked());
    p.lds_bytes = L.total; p.rl_off = p.masked() ? L.rl : 0;
  } else {
    // 16 KB of filter per query leaves 8 queries per CU (2 048 on the chip): with the index's class codes the table is 6 KB, else
    // larger batches put it in HBM, by default with half of it in LDS ("The plan of a launch", has the measurements)
    if (p.bits == FILTER_CODE_BITS && ix.codes && ix.gstride <= 64) {
      p.table = TABLE_CODES;
    } else if (p.bits > 11 && a.nq > 2048 && !sw.b128_lds) {      // a table above 8 KB; one table per block, >= the resident waves
      p.slots = 256 * 32;
      const bool n24 = ix.n < 0xFFFFFFull && !sw.b128_no24;       // an id is 24 bits and 0xFFFFFF is free for "empty"
      p.hsplit = sw.b128_split > 3 ? 0u : sw.b128_split;
      if (p.hsplit == 3 && !n24) p.hsplit = 1;                    // the all-LDS mode exists for 24-bit planes only
      p.p24 = p.hsplit && n24 ? 1u : 0u;
      p.table = p.hsplit ? TABLE_HBM_SPLIT : TABLE_HBM;
    }
    p.lds_bytes = b128_lds(p.ccap, qb, p.bits, p.table, p.hsplit, p.p24).total;
  }
  p.ws_bytes = 256 + p.dropped_bytes(a.nq) + (p.persistent() ? (std::min<uint64_t>(a.nq, p.slots) << p.bits) * 4 : 0);
  return p;
}

}  // namespace pann
