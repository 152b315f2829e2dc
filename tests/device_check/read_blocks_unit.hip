// Forwarders to launch_repair_compare and launch_repair_compare_addr (csrc/kernels.hpp) for tests/test_gpu_read_blocks_unit.py: device
// pointers and plain integers in, stream 0, the hipError_t out as an int.  Nothing is allocated, copied or checked here; the buffers,
// the address table and their guards are torch tensors of the test.  Built by the package Makefile as libread_blocks_unit.so and linked
// against libcodex_p2.so (cp2k::launch_* are exported there), so what runs are the code objects the product ships.  No entry point of
// the boundary (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" {

int rbu_repair_compare(const void* fresh, const void* kept, size_t kept_rows, const uint64_t* rows, size_t n, uint32_t* verdict) {
  return (int)cp2k::launch_repair_compare(fresh, kept, kept_rows, rows, n, verdict, nullptr);
}

// slice: the most requests one launch takes (0: a whole grid's worth, as the product calls it)
int rbu_repair_compare_addr(const void* fresh, const uint64_t* kept_addr, size_t n, uint32_t* verdict, size_t slice) {
  return (int)cp2k::launch_repair_compare_addr(fresh, kept_addr, n, verdict, nullptr, slice);
}

}  // extern "C"
