// Forwarder to launch_scatter_rows_addr (csrc/kernels.hpp) for tests/test_gpu_build_many_unit.py: device pointers and plain integers in,
// stream 0, the hipError_t out as an int.  Nothing is allocated, copied or checked here; the source, the destinations, the address table
// and their guards are torch tensors of the test.  Built by the package Makefile as libbuild_many_unit.so and linked against
// libcodex_p2.so (cp2k::launch_* are exported there), so what runs is the code object the product ships.  No entry point of the boundary
// (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" {

int bmu_scatter_rows_addr(const void* src, size_t sstride, const uint64_t* dst_addr, size_t rows, size_t n_items, size_t slice) {
  return (int)cp2k::launch_scatter_rows_addr(src, sstride, dst_addr, rows, n_items, nullptr, slice);
}

}  // extern "C"
