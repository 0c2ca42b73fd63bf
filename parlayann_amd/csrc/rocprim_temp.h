// rocprim_temp.h -- the temporary-storage sizes of the rocprim calls the builders make, asked of rocprim with the argument types
// of the real call.  Included only by the translation units that use rocprim (templates: a unit instantiates what it calls).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace pann {

// radix_sort_keys of `size` keys, all 64 bits (a sort of fewer bits takes no more)
template <class Key = uint64_t, class Size> size_t sort_temp_bytes(Size size) {
  size_t t = 0;
  (void)rocprim::radix_sort_keys(nullptr, t, (Key*)nullptr, (Key*)nullptr, size, 0, 64, (hipStream_t)0);
  return t;
}
// segmented_radix_sort_keys of `size` keys in `segs` segments with 32-bit offsets
template <class Key = uint64_t> size_t seg_sort_temp_bytes(uint32_t size, uint32_t segs) {
  size_t t = 0;
  (void)rocprim::segmented_radix_sort_keys(nullptr, t, (Key*)nullptr, (Key*)nullptr, size, segs, (const uint32_t*)nullptr,
                                           (const uint32_t*)nullptr, 0, 64, (hipStream_t)0);
  return t;
}
// exclusive_scan (plus) of `size` uint32 values into sums of type Sum: uint32_t or uint64_t
template <class Sum, class Size> size_t scan_temp_bytes(Size size) {
  size_t t = 0;
  (void)rocprim::exclusive_scan(nullptr, t, (uint32_t*)nullptr, (Sum*)nullptr, (Sum)0, size, rocprim::plus<Sum>(), (hipStream_t)0);
  return t;
}

}  // namespace pann
