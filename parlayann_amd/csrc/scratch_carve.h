// scratch_carve.h -- how one growable device buffer is cut into several arrays: ONE layout function per buffer both sizes it and
// places the pointers, so the two can never disagree.  No HIP and nothing of pann_internal.h in here: a plain host compiler
// builds it (tests/test_scratch_carve_cpu.py does, under sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pann {

// Arrays taken one after the other from `base`, each on a 256-byte boundary.  A null base is a dry run: every take() returns
// null and only the offsets are counted.  What is transferred or cleared as one block is ONE take(); what a kernel may touch
// behind an array (a row read in 16-byte chunks, rocprim's temporary storage) is that take()'s slack_bytes.
struct Carve {
  uint8_t* base; size_t off = 0;
  explicit Carve(void* b) : base((uint8_t*)b) {}
  static constexpr size_t align(size_t x) { return (x + 255) & ~(size_t)255; }
  template <class T> T* take(size_t count, size_t slack_bytes = 0) {
    off = align(off);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T) + slack_bytes;
    return p;
  }
  size_t bytes() const { return align(off); }
};

// layout(Carve&) takes the arrays of `buf` (anything with ensure(size_t) and buf: a Workspace): once dry to size the buffer,
// tail_slack bytes behind the last array included, once on the buffer to set the pointers.  A layout whose counts change between
// the two passes is an error (-1), not an overrun; an ensure() that fails returns its own code.
template <class Buf, class Layout> int carve_into(Buf& buf, size_t tail_slack, Layout&& layout) {
  Carve dry(nullptr);
  layout(dry);
  if (int rc = buf.ensure(dry.bytes() + tail_slack)) return rc;
  Carve c(buf.buf);
  layout(c);
  return c.bytes() == dry.bytes() ? 0 : -1;
}

}  // namespace pann
