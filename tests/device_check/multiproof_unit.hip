// Forwarders to launch_multiproof_layers and launch_multiproof_commit (csrc/kernels.hpp) for tests/test_gpu_multiproof_unit.py: device pointers, host tables and plain
// integers in, stream 0, the hipError_t out as an int.  Nothing is allocated, copied or checked here; the work table, the tables and
// their guards are torch tensors of the caller.  Built by the package Makefile as libmultiproof_unit.so and linked against
// libcodex_p2.so (cp2k::launch_* are exported there), so what runs is the code object the product ships.  No entry point of the boundary
// (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" {

int mpu_multiproof_layers(void* work, uint64_t n_work, const void* jobs, const uint64_t* level_off, const uint64_t* level_base, size_t n_levels,
                          const uint64_t* want_addr, uint32_t* verdict) {
  return (int)cp2k::launch_multiproof_layers(work, n_work, static_cast<const cp2k::MultiproofJob*>(jobs), level_off, level_base, n_levels, want_addr,
                                             verdict, nullptr);
}

int mpu_multiproof_commit(const void* work, uint64_t n_work, const uint32_t* src_row, const uint64_t* dst_addr, const uint32_t* group_of,
                          const uint32_t* verdict, uint32_t n_groups, size_t n) {
  return (int)cp2k::launch_multiproof_commit(work, n_work, src_row, dst_addr, group_of, verdict, n_groups, n, nullptr);
}

}  // extern "C"
