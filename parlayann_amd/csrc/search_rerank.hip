// search_rerank.hip -- beam_search_rerank (beamSearch.h:390-454) without leaving the device: float queries in, k exact
// (id, distance) pairs out.  Three launches on one stream:
//
//   prepare_queries_kernel   one pass over the float query rows: the one-byte (or packed four-bit) rows the quantised index is
//                            searched with (translate_point, as quantize.hip), with normalize_first the Point::normalize'd float rows the
//                            rerank scores against (graph_index.cpp:172), and for a filtered search the sketch rows (one
//                            ballot per 64 coordinates, as sketch.hip)
//   launch_beam_search       the search kernels of beam_search.hip, unchanged, on the one-byte index; the frontier ids and
//                            sizes stay in scratch
//   rerank_frontier_kernel   num_check = min(k * rerank_factor, frontier size) (:428) read on the device, exact distances on
//                            the f32 index through the same gather_tile as rerank_kernel (dense.hip) -- bit-identical
//                            distances, exact-float-order mode included --, sorted by (dist, id), first k written (:437-444)
//
// The rerank comes in two forms.  Up to 64 candidates (every search with beam <= 64, and any with k * rerank_factor <= 64)
// lane j keeps candidate j's key in registers: the keys move to their lanes by a lane permute as the gather emits them, a
// bitonic network of lane exchanges sorts them, lane r writes result r.  Nothing but the candidate ids (and a query that
// does not fit registers) is in LDS, so four queries share a 256-thread workgroup.  More candidates (up to the 4 096 of
// pann_rerank) keep their keys in LDS and are ranked by counting, one wave per query, as rerank_kernel does.
//
// Masked form (pann_batch_search_masked_rerank*, DESIGN.md "Masked search on the fused path"): step 2 is the masked search with
// a result list of pool = min(k * rerank_factor, beam, 64) ids, step 3 is rerank_list_kernel, which reads result_count entries of
// that list instead of the head of the frontier.  At most 64 candidates, so it has the register form only.
#include <algorithm>

#include "pann_device.h"
#include "quant_device.h"

namespace pann {
namespace {

constexpr uint32_t RR_WAVES = 4;           // queries per workgroup of the register form (fewer when four long queries do not fit LDS)
constexpr uint32_t PREP_MAX_BLOCKS = 4096; // 256 CUs x 16 one-wave blocks

// ---- step 1: the queries ------------------------------------------------------------------------------------------------
// One wave per row.  Without normalize the row is read straight from memory, 64 coordinates (256 B) at a time.  With it the
// row is staged in LDS, lane 0 sums the squares in index order -- float product, double sum: the order is part of the
// result (mips_point.h:117-118, normalize_rows_kernel) -- and every lane scales its coordinates by the one inverse norm.
// sk_kind < 0: no sketch.  sk_words: 64-bit words written per sketch row (the row's words, then zeros).
__global__ __launch_bounds__(64) void prepare_queries_kernel(const uint8_t* __restrict__ src, uint64_t sstride, uint64_t nq,
                                                             uint32_t d, int normalize, QParams q, uint8_t* __restrict__ qout,
                                                             uint64_t qstride, uint8_t* __restrict__ nout, uint64_t nstride,
                                                             int sk_kind, float thr, uint8_t* __restrict__ sout, uint64_t sk_stride,
                                                             uint32_t sk_words) {
#pragma clang fp contract(off)
  extern __shared__ float staged[];               // d floats, only with normalize
  const uint32_t lane = threadIdx.x;
  const uint32_t nblk = (d + 63) / 64;
  for (uint64_t r = blockIdx.x; r < nq; r += gridDim.x) {
    const float* __restrict__ row = reinterpret_cast<const float*>(src + r * sstride);
    float inv = 1.0f;
    if (normalize) {
      for (uint32_t c = lane; c < d; c += 64) staged[c] = row[c];
      wave_lds_sync();
      if (lane == 0) {
        double norm = 0.0;
        for (uint32_t j = 0; j < d; j++) { const float p = staged[j] * staged[j]; norm += (double)p; }
        norm = __dsqrt_rn(norm);
        if (norm == 0) norm = 1.0;
        inv = (float)__ddiv_rn(1.0, norm);                        // float inv_norm = 1.0 / norm
      }
      inv = __shfl(inv, 0);
    }
    uint8_t* __restrict__ qrow = qout + r * qstride;
    float* __restrict__ nrow = normalize ? reinterpret_cast<float*>(nout + r * nstride) : nullptr;
    unsigned long long w_sign = 0, w_mask = 0;
    for (uint32_t b = 0; b < nblk; b++) {
      const uint32_t j = b * 64 + lane;
      const bool in = j < d;
      float x = 0.0f;
      if (in) {
        if (normalize) { x = staged[j] * inv; nrow[j] = x; }
        else x = row[j];
        if (!q.bits4) qrow[j] = (uint8_t)quantize_one(x, q);
      }
      if (q.bits4) {      // the even lane of a pair writes the byte: its own nibble low, its neighbour's high (0 past the row's end)
        const uint32_t v = in ? quantize_one(x, q) : 0u;
        const uint32_t hi = (uint32_t)__shfl_down((int)v, 1);
        if (in && !(lane & 1)) qrow[j >> 1] = (uint8_t)(v | (hi << 4));
      }
      if (sk_kind >= 0) {                                          // sketch_translate_kernel's tests, on the same values
        bool s, m = false;
        if (sk_kind == PANN_SKETCH_MIPS_2BIT) {
          const bool neg = x < -thr, pos = !neg && x > thr;
          m = in && (neg || pos);
          s = in && pos;
        } else {
          s = in && x > thr;
        }
        const unsigned long long sw = __ballot(s), mw = __ballot(m);
        if (lane == b) { w_sign = sw; w_mask = mw; }
      }
    }
    if (sk_kind >= 0) {
      unsigned long long* o = reinterpret_cast<unsigned long long*>(sout + r * sk_stride);
      if (sk_kind == PANN_SKETCH_MIPS_2BIT) {
        if (2 * lane < sk_words) { o[2 * lane] = w_sign; o[2 * lane + 1] = w_mask; }
      } else {
        if (lane < sk_words) o[lane] = w_sign;
      }
    }
    wave_lds_sync();                                               // the next row overwrites the staged one
  }
}

// ---- step 3: rerank from the frontier -----------------------------------------------------------------------------------
struct RerankArgs {
  PointsView pv; uint32_t dbytes;                 // the f32 index
  const uint8_t* q; uint64_t q_stride;            // the float rows the candidates are scored against
  const uint32_t* fids; uint32_t beam;            // nq x beam frontier ids of the quantised search
  const uint32_t* fsize;                          // nq
  uint64_t nq;
  uint32_t k, want;                               // want = k * rerank_factor (clamped to beam)
  uint32_t kcap;                                  // LDS form: keys per query
  uint32_t qbytes;                                // LDS bytes of one query (0: registers)
  uint32_t* out_ids; float* out_dists; uint32_t* out_fsize; uint32_t* status;
};

// sorts one key per lane ascending across the wave: 21 compare-exchange steps with the lane `j` away
__device__ __forceinline__ uint64_t wave_sort64(uint64_t key, int lane) {
#pragma unroll
  for (int span = 2; span <= PANN_WAVE; span <<= 1) {
#pragma unroll
    for (int j = span >> 1; j > 0; j >>= 1) {
      const uint64_t other = __shfl_xor(key, j);
      const bool up = (lane & span) == 0, low = (lane & j) == 0;
      const bool keep_min = low == up;
      key = ((other < key) == keep_min) ? other : key;
    }
  }
  return key;
}

template <int METRIC, int LPC, bool NCH1, bool REG>
__global__ void __launch_bounds__(REG ? RR_WAVES * PANN_WAVE : PANN_WAVE) rerank_frontier_kernel(RerankArgs P) {
  constexpr int DT = PANN_F32;
  const int lane = threadIdx.x & (PANN_WAVE - 1);
  const uint32_t w = REG ? threadIdx.x / PANN_WAVE : 0u;
  const uint64_t qi = REG ? (uint64_t)blockIdx.x * (blockDim.x / PANN_WAVE) + w : (uint64_t)blockIdx.x;
  if (qi >= P.nq) return;                          // a whole wave leaves; the waves of a block share no data and no barrier
  extern __shared__ __align__(16) uint8_t smem[];
  // per wave: [keys (LDS form)] [query, qbytes] [64 candidate ids]
  const uint32_t key_bytes = REG ? 0u : ((P.kcap + 1) & ~1u) * 8u;
  uint8_t* base = smem + (size_t)w * (P.qbytes + PANN_WAVE * 4);
  uint64_t* K = reinterpret_cast<uint64_t*>(base);
  uint4* qlds = reinterpret_cast<uint4*>(base + key_bytes);
  uint32_t* Pl = reinterpret_cast<uint32_t*>(base + key_bytes + P.qbytes);
  QReg<DT> qreg{};
  load_query<DT, LPC, NCH1>(P.q + qi * P.q_stride, P.dbytes, P.pv.nch, qreg, qlds, lane);
  const uint32_t fs = P.fsize[qi];
  const uint32_t cn = min(min(fs, P.want), P.beam);                 // num_check, beamSearch.h:428
  const uint32_t* ids = P.fids + qi * P.beam;
  if (lane == 0) {
    if (P.out_fsize) P.out_fsize[qi] = fs;
    if (fs < P.k) atomicOr(P.status, (uint32_t)PANN_STATUS_SHORT_FRONTIER);   // :416-419
  }
  const size_t ro = (size_t)qi * P.k;
  if constexpr (REG) {                             // cn <= 64, k <= 64
    if (lane < (int)cn) Pl[lane] = ids[lane];
    wave_lds_sync();
    uint64_t key = KEY_INF;
    if (cn) {
      const bool per_lane = !NCH1 && P.pv.exact;   // exact float order: lane j already holds candidate j
      gather_tile<DT, METRIC, LPC, NCH1, 4>(P.pv, qreg, qlds, Pl, cn, lane,
        [&](bool has, uint32_t ci, uint32_t id, float dist) {
          const uint64_t mine = make_key(dist, id);
          if (per_lane) { if (has) key = mine; return; }
          // every lane of group g holds candidate first + g of this step: lane j takes candidate j from group j - first
          constexpr int G = PANN_WAVE / LPC;
          const int first = (int)ci - lane / LPC, g = lane - first;
          const uint64_t got = __shfl(mine, (g & (G - 1)) * LPC);
          if (g >= 0 && g < G && lane < (int)cn) key = got;
        });
    }
    key = wave_sort64(key, lane);                   // lanes >= cn hold KEY_INF: they sort behind every candidate
    if (lane < (int)P.k) {
      const bool ok = lane < (int)cn;
      P.out_ids[ro + lane] = ok ? key_id(key) : SENTINEL;
      P.out_dists[ro + lane] = ok ? key_dist(key) : __builtin_inff();
    }
  } else {
    for (uint32_t j0 = 0; j0 < cn; j0 += PANN_WAVE) {
      const uint32_t mm = min(cn - j0, (uint32_t)PANN_WAVE);
      if (lane < (int)mm) Pl[lane] = ids[j0 + lane];
      wave_lds_sync();
      gather_tile<DT, METRIC, LPC, NCH1, 4>(P.pv, qreg, qlds, Pl, mm, lane,
        [&](bool has, uint32_t ci, uint32_t id, float dist) { if (has) K[j0 + ci] = make_key(dist, id); });
      wave_lds_sync();
    }
    for (uint32_t j0 = 0; j0 < max(cn, P.k); j0 += PANN_WAVE) {
      const uint32_t j = j0 + lane;
      if (j < cn) {
        const uint64_t key = K[j];
        uint32_t r = 0;
        for (uint32_t i = 0; i < cn; i++) { const uint64_t o = K[i]; r += (o < key || (o == key && i < j)) ? 1u : 0u; }
        if (r < P.k) { P.out_ids[ro + r] = key_id(key); P.out_dists[ro + r] = key_dist(key); }
      } else if (j < P.k) {
        P.out_ids[ro + j] = SENTINEL; P.out_dists[ro + j] = __builtin_inff();
      }
    }
  }
}

// The masked form: the candidates are the result list of the masked search.  RerankArgs as above with fids = the nq x pool
// lists, beam = pool (<= 64), fsize = the lists' lengths (result_count); want, kcap, out_fsize and status are not read -- the
// search itself writes frontier_size, and a short row is an answer, not a SHORT_FRONTIER.  Slots past a list's length hold
// 0xFFFFFFFF: only lanes below the length load an id, and an empty list pads its row without entering the gather.
template <int METRIC, int LPC, bool NCH1>
__global__ void __launch_bounds__(RR_WAVES * PANN_WAVE) rerank_list_kernel(RerankArgs P) {
  constexpr int DT = PANN_F32;
  const int lane = threadIdx.x & (PANN_WAVE - 1);
  const uint32_t w = threadIdx.x / PANN_WAVE;
  const uint64_t qi = (uint64_t)blockIdx.x * (blockDim.x / PANN_WAVE) + w;
  if (qi >= P.nq) return;                          // a whole wave leaves; the waves of a block share no data and no barrier
  extern __shared__ __align__(16) uint8_t smem[];
  uint8_t* base = smem + (size_t)w * (P.qbytes + PANN_WAVE * 4);       // per wave: [query, qbytes] [64 candidate ids]
  uint4* qlds = reinterpret_cast<uint4*>(base);
  uint32_t* Pl = reinterpret_cast<uint32_t*>(base + P.qbytes);
  const uint32_t cn = min(min(P.fsize[qi], P.beam), (uint32_t)PANN_WAVE);      // num_check = result_count
  const size_t ro = (size_t)qi * P.k;
  uint64_t key = KEY_INF;
  if (cn) {                                        // wave-uniform
    QReg<DT> qreg{};
    load_query<DT, LPC, NCH1>(P.q + qi * P.q_stride, P.dbytes, P.pv.nch, qreg, qlds, lane);
    if (lane < (int)cn) Pl[lane] = P.fids[qi * P.beam + lane];
    wave_lds_sync();
    const bool per_lane = !NCH1 && P.pv.exact;     // exact float order: lane j already holds candidate j
    gather_tile<DT, METRIC, LPC, NCH1, 4>(P.pv, qreg, qlds, Pl, cn, lane,
      [&](bool has, uint32_t ci, uint32_t id, float dist) {
        const uint64_t mine = make_key(dist, id);
        if (per_lane) { if (has) key = mine; return; }
        constexpr int G = PANN_WAVE / LPC;           // as rerank_frontier_kernel: lane j takes candidate j from group j - first
        const int first = (int)ci - lane / LPC, g = lane - first;
        const uint64_t got = __shfl(mine, (g & (G - 1)) * LPC);
        if (g >= 0 && g < G && lane < (int)cn) key = got;
      });
    key = wave_sort64(key, lane);                   // lanes >= cn hold KEY_INF: they sort behind every candidate
  }
  if (lane < (int)P.k) {                           // k <= 64
    const bool ok = lane < (int)cn;
    P.out_ids[ro + lane] = ok ? key_id(key) : SENTINEL;
    P.out_dists[ro + lane] = ok ? key_dist(key) : __builtin_inff();
  }
}

struct Scratch { uint8_t* qb; uint64_t qb_stride; uint8_t* sk; uint64_t sk_stride; uint8_t* nr; uint64_t nr_stride; uint32_t* fids; uint32_t* fsize; size_t bytes; };

Scratch cut_scratch(const DeviceIndex& quant, uint64_t nq, uint32_t beam, int normalize_first, int use_filter, void* base) {
  Scratch s{};
  Carve c(base);
  s.qb_stride = (quant.dbytes + 15) / 16 * 16;
  s.qb = c.take<uint8_t>(nq * s.qb_stride);
  if (use_filter) { s.sk_stride = sketch_row_bytes(quant.sk_kind, quant.d); s.sk = c.take<uint8_t>(nq * s.sk_stride); }
  if (normalize_first) { s.nr_stride = ((uint64_t)quant.d * 4 + 15) / 16 * 16; s.nr = c.take<uint8_t>(nq * s.nr_stride); }
  s.fids = c.take<uint32_t>(nq * (size_t)beam);
  s.fsize = c.take<uint32_t>(nq);
  s.bytes = c.bytes();
  return s;
}

}  // namespace

size_t search_rerank_scratch_bytes(const DeviceIndex& quant, uint64_t nq, uint32_t beam, int normalize_first, int use_filter) {
  return cut_scratch(quant, nq, beam, normalize_first, use_filter, nullptr).bytes;
}

// ids kept per query between search and rerank: the frontier, or the masked search's result list
static uint32_t list_length(const RerankCall& r) { return r.filter.given() ? masked_rerank_pool(r.qp) : (uint32_t)r.qp->beam; }

// step 2 as a request: the search on the one-byte index, over the prepared rows of the scratch
static SearchCall quant_search(const RerankCall& r, const Scratch& s) {
  SearchCall c;
  c.queries = s.qb; c.qstride = s.qb_stride; c.nq = r.nq;
  c.starts = r.starts; c.nstarts = r.nstarts; c.qp = r.qp; c.dev = true;
  c.out.ids = s.fids; c.out.out_k = list_length(r); c.out.frontier_size = s.fsize;
  c.out.visited_count = r.out.visited_count; c.out.dist_cmps = r.out.dist_cmps;
  if (r.filter.given()) {                          // bitmap rows, or the labels of `full` with the queries' predicates
    c.out.frontier_size = r.out.frontier_size;
    c.filter = r.filter; c.result_count = r.result_count ? r.result_count : s.fsize; c.allowed_cmps = r.allowed_cmps;
  }
  if (r.use_filter) { c.sketch = true; c.sketch_queries = s.sk; c.sq_stride = s.sk_stride; c.pruned_cmps = r.out.pruned_cmps; }
  return c;
}

// The workspace is sized by the plan of the same request that search_rerank_dev launches, so the two cannot disagree.  The scratch
// is cut from a null base here: the plan reads counts, parameters and modes of the launch arguments (plan_of, beam_search.hip), never a
// pointer, and nothing is dereferenced.
size_t search_rerank_ws_bytes(const DeviceIndex& quant, const RerankCall& r) {
  const Scratch s = cut_scratch(quant, r.nq, list_length(r), r.normalize_first, r.use_filter, nullptr);
  return search_workspace_bytes(quant, slice(quant_search(r, s), 0, r.nq, r.dcap));
}

int search_rerank_dev(const DeviceIndex& full, const DeviceIndex& quant, const Workspace& search_ws, void* scratch,
                      const pann_sketch_params* sparams, const RerankCall& r) {
  const uint64_t nq = r.nq, q_stride = r.qstride;
  const pann_query_params* qp = r.qp;
  const pann_quant_params* qparams = r.qparams;
  const float* d_queries = r.queries;
  const int normalize_first = r.normalize_first, use_filter = r.use_filter;
  const pann_rerank_out& d_out = r.out;
  const bool mask = r.filter.given();
  hipStream_t st = (hipStream_t)r.stream;
  if (nq == 0) return PANN_OK;
  const uint32_t d = full.d, beam = (uint32_t)qp->beam, k = (uint32_t)qp->k;
  if (beam == 0 || beam > 4096) { set_error("pann_rerank: candidates per query must be in [1,4096]"); return PANN_ERR_BAD_ARG; }
  const uint32_t pool = mask ? masked_rerank_pool(qp) : 0u;        // masked: ids per result list
  if (mask && (use_filter || k > PANN_WAVE)) { set_error("pann_batch_search_masked_rerank: no sketch filter, k <= 64"); return PANN_ERR_UNSUPPORTED; }
  const Scratch s = cut_scratch(quant, nq, list_length(r), normalize_first, use_filter, scratch);

  // ---- 1. the queries ----
  const size_t prep_lds = normalize_first ? (size_t)d * 4 : 0;
  if (prep_lds > 64 * 1024) { set_error("normalize: rows of more than 16382 floats are not supported"); return PANN_ERR_UNSUPPORTED; }
  const int sk_kind = use_filter ? sparams->kind : -1;
  hipLaunchKernelGGL(prepare_queries_kernel, dim3((uint32_t)std::min<uint64_t>(nq, PREP_MAX_BLOCKS)), dim3(PANN_WAVE), prep_lds, st,
                     reinterpret_cast<const uint8_t*>(d_queries), q_stride, nq, d, normalize_first ? 1 : 0, make_qparams(qparams), s.qb,
                     s.qb_stride, s.nr, s.nr_stride, sk_kind, use_filter ? sketch_threshold(sparams) : 0.0f, s.sk, s.sk_stride,
                     (uint32_t)(s.sk_stride / 8));
  PANN_HIP(hipGetLastError());

  // ---- 2. the search on the one-byte index ----
  const SearchArgs a = slice(quant_search(r, s), 0, nq, r.dcap);
  uint32_t* rcount = mask ? a.result_count : s.fsize;      // masked: the lists' lengths, in the caller's array when there is one
  if (int rc = launch_beam_search(quant, a, search_ws.buf, search_ws.bytes, st)) return rc;
  uint32_t* status = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(search_ws.buf) + 64);      // the search's status word

  // ---- 3. rerank from the frontier ----
  RerankArgs R{};
  R.pv = PointsView{full.points, full.pstride, full.nch, full.exact}; R.dbytes = full.dbytes;
  R.q = normalize_first ? s.nr : reinterpret_cast<const uint8_t*>(d_queries);
  R.q_stride = normalize_first ? s.nr_stride : q_stride;
  R.fids = s.fids; R.beam = beam; R.fsize = s.fsize; R.nq = nq; R.k = k;
  R.want = (uint32_t)std::min<int64_t>(std::max<int64_t>((int64_t)qp->k * qp->rerank_factor, 0), beam);
  R.kcap = R.want;
  R.qbytes = (uint32_t)query_lds_bytes(full);
  R.out_ids = d_out.ids; R.out_dists = d_out.dists; R.out_fsize = d_out.frontier_size; R.status = status;
  // masked: the lists (pool <= 64 ids each) and their lengths; the search has written frontier_size itself
  if (mask) { R.beam = pool; R.fsize = rcount; R.want = R.kcap = pool; R.out_fsize = nullptr; }
  const bool reg = std::max(R.want, k) <= PANN_WAVE;       // always true for the masked form
  const size_t wave_lds = (size_t)R.qbytes + PANN_WAVE * 4;
  uint32_t waves = RR_WAVES;                       // rows of a thousand floats and more: fewer queries per workgroup, as rerank_kernel
  while (waves > 1 && waves * wave_lds > 64 * 1024) waves >>= 1;
  const size_t lds = reg ? waves * wave_lds : (size_t)((R.kcap + 1) & ~1u) * 8 + wave_lds;
  if (lds > 64 * 1024) { set_error("pann_batch_search_rerank: rows too long for the rerank's LDS state"); return PANN_ERR_UNSUPPORTED; }
#define CALL_RF(DT, MT, L, N1)                                                                                                    \
  do {                                                                                                                            \
    if (reg) hipLaunchKernelGGL((rerank_frontier_kernel<MT, L, N1, true>), dim3((uint32_t)((nq + waves - 1) / waves)),             \
                                dim3(waves * PANN_WAVE), lds, st, R);                                                              \
    else hipLaunchKernelGGL((rerank_frontier_kernel<MT, L, N1, false>), dim3((uint32_t)nq), dim3(PANN_WAVE), lds, st, R);          \
  } while (0)
#define CALL_RL(DT, MT, L, N1)                                                                                                    \
  hipLaunchKernelGGL((rerank_list_kernel<MT, L, N1>), dim3((uint32_t)((nq + waves - 1) / waves)), dim3(waves * PANN_WAVE), lds, st, R)
  if (mask) {
    if (full.metric == PANN_L2) PANN_LAYOUT_SWITCH(full, PANN_F32, PANN_L2, CALL_RL);
    else PANN_LAYOUT_SWITCH(full, PANN_F32, PANN_MIPS, CALL_RL);
  } else if (full.metric == PANN_L2) PANN_LAYOUT_SWITCH(full, PANN_F32, PANN_L2, CALL_RF);
  else PANN_LAYOUT_SWITCH(full, PANN_F32, PANN_MIPS, CALL_RF);
#undef CALL_RL
#undef CALL_RF
  PANN_HIP(hipGetLastError());
  if (d_out.status) PANN_HIP(hipMemcpyAsync(d_out.status, status, 4, hipMemcpyDeviceToDevice, st));
  return PANN_OK;
}

}  // namespace pann
