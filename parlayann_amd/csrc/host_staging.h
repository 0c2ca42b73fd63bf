// host_staging.h -- the pure arithmetic behind the host-pointer search calls of api.hip: where the pieces of a packed transfer
// lie, and how a search batch is run again when its dropped lists were too small.  No HIP and nothing of pann_internal.h in
// here: a plain host compiler builds it (tests/test_host_staging_cpu.py does, under sanitizers).
#pragma once
#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>

#include "../../include/pann.h"
#include "scratch_carve.h"

namespace pann {

// One packed region: host arrays laid out one after the other, each on a 256-byte boundary, so that a call moves them in ONE
// transfer (inputs: copy() into pinned memory and send up; outputs: bring down into pinned memory and copy() out).  A piece whose
// host pointer is null takes no room and has no device address: optional arrays are simply added.  A scratch piece has room and
// a device address but no host array: copy() passes it by (what never leaves the device, or leaves it by a transfer of its own).
// A direct piece is a contiguous host array of direct_from bytes or more: it has its place in the region too, but copy() passes
// it by and the caller moves it between the host array and that place in a transfer of its own (a large array gains nothing
// from the pinned copy and would keep as much pinned memory on the handle).  Behind a direct piece every later one-row piece is
// direct too, whatever its size, so the packed pieces end at host_end and nothing behind it needs pinned room or is carried by
// the packed transfer; small arrays are therefore added first.
struct PackedLayout {
  static constexpr int kMaxPieces = 12;
  struct Piece { void* host; size_t bytes, off, rows, host_stride; bool direct; };
  Piece pc[kMaxPieces];
  int count = 0;
  size_t total = 0;      // bytes of the region: the sum of the aligned piece sizes
  size_t host_end = 0;   // where the last packed piece ends: scratch and direct pieces behind it need no pinned room and no packed transfer
  size_t direct_from = SIZE_MAX;      // one-row pieces of this many bytes or more are direct (set before the first add)
  bool any_direct = false;

  static size_t align(size_t x) { return Carve::align(x); }

  // `rows` rows of row_bytes each, host_stride bytes apart on the host and dense in the region (bitmap rows of a wider table)
  int add_rows(const void* host, size_t rows, size_t row_bytes, size_t host_stride, size_t slack = 0) {
    assert(count < kMaxPieces);
    const size_t bytes = host ? rows * row_bytes : 0;
    const bool direct = rows == 1 && bytes && (bytes >= direct_from || any_direct);
    any_direct = any_direct || direct;
    pc[count] = Piece{const_cast<void*>(host), bytes, total, rows, host_stride, direct};
    total += align(bytes ? bytes + slack : 0);
    if (bytes && !direct) host_end = total;
    return count++;
  }
  // `slack`: bytes kept free behind the piece before the next one is aligned (kernels that read a query row in 16-byte chunks)
  int add(const void* host, size_t bytes, size_t slack = 0) { return add_rows(host, 1, bytes, bytes, slack); }
  int add_scratch(size_t bytes) {
    assert(count < kMaxPieces);
    pc[count] = Piece{nullptr, bytes, total, 1, bytes, false};
    total += align(bytes);
    return count++;
  }
  // an output that the kernel writes whether or not the caller asked for it
  int add_or_scratch(const void* host, size_t bytes) { return host ? add(host, bytes) : add_scratch(bytes); }

  // the piece's address in a region that starts at `base` (null for an empty piece)
  void* at(void* base, int i) const { return pc[i].bytes ? (void*)((uint8_t*)base + pc[i].off) : nullptr; }

  // where the region ends that holds the first npieces pieces
  size_t end_of(int npieces) const { return npieces < count ? pc[npieces].off : total; }

  // host arrays -> region (pack the inputs) or back (unpack the outputs), pieces [first, last)
  void copy(void* region, bool to_region, int first = 0, int last = kMaxPieces) const {
    for (int i = first; i < std::min(last, count); i++) {
      const size_t rb = pc[i].bytes / std::max<size_t>(pc[i].rows, 1);
      for (size_t r = 0; r < pc[i].rows && pc[i].bytes && pc[i].host && !pc[i].direct; r++) {
        uint8_t* in_region = (uint8_t*)region + pc[i].off + r * rb, *on_host = (uint8_t*)pc[i].host + r * pc[i].host_stride;
        memcpy(to_region ? in_region : on_host, to_region ? on_host : in_region, rb);
      }
    }
  }
};

// The "dropped" scratch of a search is nq * dcap * 8 bytes.  When a launch reports that it was too small the list is grown (x8,
// up to min(limit, n): a query drops at most one entry per visited vertex) and the batch runs again; a grown list that would
// take more than kDropBudget for the whole batch makes the batch run in ranges of queries instead, and the handle keeps at most
// kDropKeep entries per query for later calls (10K queries x 2048 x 8 B = 160 MB), not the worst case of one odd batch.
// launch(q0, cnt, dcap, &word): queries [q0, q0 + cnt) with a list of dcap entries, synchronised, word = the launch's status
// word.  *status: the bits of the last pass over the batch; *whole: that pass was one launch of all nq queries.  `kept`: the
// handle's capacity, read at the start and raised at a successful end only.  Returns a launch's own error code as it is; a list
// that overflows at its largest size is PANN_ERR_OVERFLOW with the message in *err (the caller's error slot).
template <class Launch>
int run_with_dropped_growth(uint32_t& kept, uint64_t n, uint64_t nq, int64_t limit, const char* fn, uint32_t* status, bool* whole,
                            std::string* err, Launch&& launch) {
  constexpr uint64_t kDropBudget = 1ull << 30;
  constexpr uint32_t kDropKeep = 2048;
  const uint64_t dneed = (uint64_t)std::min<int64_t>(std::max<int64_t>(limit, 1), (int64_t)n);
  uint32_t dcap = kept;
  for (;;) {
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(nq, kDropBudget / ((uint64_t)std::max<uint32_t>(dcap, 64) * 8)));
    *status = 0; *whole = chunk >= nq;
    for (uint64_t q0 = 0; q0 < nq; q0 += chunk) {
      uint32_t st_word = 0;      // the launch's status word (the next launch clears it)
      if (int rc = launch(q0, std::min(chunk, nq - q0), dcap, &st_word)) return rc;
      *status |= st_word;
      if (*status & PANN_STATUS_DROPPED_OVERFLOW) break;
    }
    if (!(*status & PANN_STATUS_DROPPED_OVERFLOW)) break;
    // The reference has no such list (its `visited` vector grows as needed, beamSearch.h:80,113): grow ours and run the batch again.
    if ((uint64_t)dcap >= dneed) { *err = std::string(fn) + ": internal dropped-list overflow"; return PANN_ERR_OVERFLOW; }
    dcap = (uint32_t)std::min<uint64_t>((uint64_t)dcap * 8, (dneed + 63) / 64 * 64);
  }
  kept = std::max(kept, std::min(dcap, kDropKeep));
  return PANN_OK;
}

}  // namespace pann
