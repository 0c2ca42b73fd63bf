// scratch_carve_check.cpp -- parlayann_amd/csrc/scratch_carve.h on its own, built by a plain host compiler under sanitizers and run
// by tests/test_scratch_carve_cpu.py: a layout of several arrays carved into a malloc-backed stand-in for the device Workspace.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../parlayann_amd/csrc/scratch_carve.h"

using pann::Carve;
using pann::carve_into;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

// Workspace on the host: grown on demand, never shrunk, and EXACTLY as large as asked, so that AddressSanitizer sees every byte
// written behind the ensured size
struct HostBuf {
  void* buf = nullptr; size_t bytes = 0; int allocs = 0; int fail_with = 0;
  ~HostBuf() { free(buf); }
  int ensure(size_t need) {
    if (fail_with) return fail_with;
    if (need <= bytes) return 0;
    free(buf); buf = nullptr; bytes = 0;
    if (posix_memalign(&buf, 256, need)) return 2;
    bytes = need; allocs++;
    return 0;
  }
};

struct Piece { uint8_t* p; size_t bytes; };      // a piece with its slack

int main() {
  static_assert(Carve::align(0) == 0 && Carve::align(1) == 256 && Carve::align(256) == 256 && Carve::align(257) == 512, "align rounds up to 256");

  // ---- a layout with odd sizes, slack behind two pieces and an empty piece in the middle ----
  const size_t n = 37, tail = 4096;
  uint32_t *a, *empty, *d; uint64_t* b; uint8_t* c;
  std::vector<Piece> pieces;
  auto layout = [&](Carve& cv) {
    pieces.clear();
    a = cv.take<uint32_t>(n);            pieces.push_back({(uint8_t*)a, n * 4});
    b = cv.take<uint64_t>(n + 1, 16);    pieces.push_back({(uint8_t*)b, (n + 1) * 8 + 16});
    empty = cv.take<uint32_t>(0);        pieces.push_back({(uint8_t*)empty, 0});
    c = cv.take<uint8_t>(255, 1);        pieces.push_back({c, 256});
    d = cv.take<uint32_t>(64);           pieces.push_back({(uint8_t*)d, 256});
  };

  Carve dry(nullptr);
  layout(dry);
  for (const Piece& p : pieces) CHECK(p.p == nullptr);      // a dry run hands out no address
  CHECK(dry.bytes() % 256 == 0 && dry.bytes() == 256 + 512 + 0 + 256 + 256);

  HostBuf ws;
  CHECK(carve_into(ws, tail, layout) == 0);
  uint8_t* base = (uint8_t*)ws.buf;
  CHECK(ws.allocs == 1 && ws.bytes == dry.bytes() + tail);
  {
    Carve bound(base);
    layout(bound);
    CHECK(bound.bytes() == dry.bytes());                     // the dry total is the bound end
  }
  for (size_t i = 0; i < pieces.size(); i++) {
    const Piece& p = pieces[i];
    CHECK(p.p >= base && (size_t)(p.p - base) % 256 == 0 && (uintptr_t)p.p % 256 == 0);
    CHECK(p.p + p.bytes <= base + dry.bytes());
    if (i + 1 < pieces.size()) CHECK(p.p + p.bytes <= pieces[i + 1].p);      // in order, slack included, no overlap
  }
  CHECK(pieces[2].bytes == 0 && pieces[2].p == pieces[3].p);   // the empty piece takes no room
  CHECK((uint8_t*)b == base + 256 && c == base + 768 && (uint8_t*)d == base + 1024);
  // every byte of every piece and its slack, and the tail behind the last piece, can be written
  for (size_t i = 0; i < pieces.size(); i++) memset(pieces[i].p, (int)(i + 1), pieces[i].bytes);
  CHECK(base + dry.bytes() + tail == base + ws.bytes);
  memset(base + dry.bytes(), 0xEE, tail);
  for (size_t i = 0; i < pieces.size(); i++)      // and no piece was written over by a later one
    for (size_t j = 0; j < pieces[i].bytes; j++) CHECK(pieces[i].p[j] == (uint8_t)(i + 1));

  // ---- a second carve into a buffer that is large enough: no reallocation, the same addresses ----
  const std::vector<Piece> before = pieces;
  CHECK(carve_into(ws, tail, layout) == 0);
  CHECK(ws.allocs == 1 && ws.buf == base);
  for (size_t i = 0; i < pieces.size(); i++) CHECK(pieces[i].p == before[i].p);
  // a smaller layout in the same buffer, and a larger one that grows it
  uint32_t* one;
  CHECK(carve_into(ws, 0, [&](Carve& cv) { one = cv.take<uint32_t>(1); }) == 0);
  CHECK(ws.allocs == 1 && (uint8_t*)one == base);
  uint8_t* big;
  CHECK(carve_into(ws, 16, [&](Carve& cv) { one = cv.take<uint32_t>(1); big = cv.take<uint8_t>(1 << 20); }) == 0);
  CHECK(ws.allocs == 2 && ws.bytes == 256 + (1 << 20) + 16 && big == (uint8_t*)ws.buf + 256);
  memset(big, 1, (1 << 20) + 16);

  // ---- a layout whose counts differ between the two passes is an error, whichever way they differ ----
  size_t pass = 0;
  CHECK(carve_into(ws, 0, [&](Carve& cv) { cv.take<uint32_t>(pass++ ? 65 : 64); }) != 0);
  pass = 0;
  CHECK(carve_into(ws, 0, [&](Carve& cv) { cv.take<uint32_t>(pass++ ? 64 : 65); }) != 0);
  pass = 0;
  CHECK(carve_into(ws, 0, [&](Carve& cv) { cv.take<uint32_t>(64); if (pass++) cv.take<uint8_t>(1); }) != 0);

  // ---- a failing ensure() returns its own code, and the layout is not run on a buffer ----
  HostBuf bad;
  bad.fail_with = 7;
  int runs = 0;
  CHECK(carve_into(bad, 0, [&](Carve& cv) { runs++; CHECK(cv.take<uint32_t>(8) == nullptr); }) == 7);
  CHECK(runs == 1);

  // ---- an empty layout is legal: nothing but the tail ----
  HostBuf none;
  CHECK(carve_into(none, 0, [](Carve&) {}) == 0 && none.allocs == 0);
  CHECK(carve_into(none, 256, [](Carve&) {}) == 0 && none.bytes == 256);

  printf("scratch_carve: ok\n");
  return 0;
}
