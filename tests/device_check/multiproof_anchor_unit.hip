// Forwarders to launch_multiproof_tops and, for the cases that run the layers first, launch_multiproof_layers (csrc/kernels.hpp) for
// tests/test_gpu_multiproof_anchor_unit.py: device pointers, host tables and plain integers in, stream 0, the hipError_t out as an int.
// Nothing is allocated, copied or checked here; the work table, the tables and their guards are torch tensors of the caller.  Built by
// the package Makefile as libmultiproof_anchor_unit.so and linked against libcodex_p2.so (cp2k::launch_* are exported there), so what runs
// is the code object the product ships.  No entry point of the boundary (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" {

int mau_multiproof_tops(const void* work, uint64_t n_work, const void* tops, const uint64_t* want_addr, size_t n_tops, const uint64_t* top_off,
                        const uint64_t* d_top_off, size_t n_groups, uint32_t* top_verdict, uint32_t* verdict) {
  return (int)cp2k::launch_multiproof_tops(work, n_work, static_cast<const cp2k::MultiproofTop*>(tops), want_addr, n_tops, top_off, d_top_off, n_groups,
                                           top_verdict, verdict, nullptr);
}

int mau_multiproof_layers(void* work, uint64_t n_work, const void* jobs, const uint64_t* level_off, const uint64_t* level_base, size_t n_levels,
                          const uint64_t* want_addr, uint32_t* verdict) {
  return (int)cp2k::launch_multiproof_layers(work, n_work, static_cast<const cp2k::MultiproofJob*>(jobs), level_off, level_base, n_levels, want_addr,
                                             verdict, nullptr);
}

}  // extern "C"
