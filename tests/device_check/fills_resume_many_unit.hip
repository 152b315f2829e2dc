// Forwarder to launch_block_root_recheck_addr (csrc/kernels.hpp) for tests/test_gpu_fills_resume_many_unit.py: device pointers and plain
// integers in, stream 0, the hipError_t out as an int.  Nothing is allocated, copied or checked here; the buffers and their guards are
// torch tensors of the test.  Built by the package Makefile as libfills_resume_many_unit.so and linked against libcodex_p2.so, so what
// runs is the code object the product ships.  No entry point of the boundary (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" int frmu_block_root_recheck_addr(const void* fresh, const uint64_t* addr, size_t n, uint32_t* verdict) {
  return (int)cp2k::launch_block_root_recheck_addr(fresh, addr, n, verdict, nullptr);
}
