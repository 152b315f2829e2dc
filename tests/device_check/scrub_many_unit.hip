// Forwarders to launch_scrub_compare and launch_scrub_compare_many (csrc/kernels.hpp) for tests/test_gpu_scrub_many_unit.py: device
// pointers and plain integers in, stream 0, the hipError_t out as an int.  Nothing is allocated, copied or checked here; the buffers,
// the address tables and their guards are torch tensors of the test.  Built by the package Makefile as libscrub_many_unit.so and linked
// against libcodex_p2.so (cp2k::launch_* are exported there), so what runs are the code objects the product ships.  No entry point of
// the boundary (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" {

size_t smu_scrub_tile() { return cp2k::SCRUB_TILE; }

int smu_scrub_compare(const void* fresh, size_t fstride, const void* kept, size_t kstride, size_t rows, size_t n_items, uint64_t* bits,
                      uint32_t* counts) {
  return (int)cp2k::launch_scrub_compare(fresh, fstride, kept, kstride, rows, n_items, bits, counts, nullptr);
}

int smu_scrub_compare_many(const void* fresh, size_t fstride, const uint64_t* kept_addr, size_t rows, size_t n_items, uint64_t* bits,
                           uint32_t* counts) {
  return (int)cp2k::launch_scrub_compare_many(fresh, fstride, kept_addr, rows, n_items, bits, counts, nullptr);
}

}  // extern "C"
