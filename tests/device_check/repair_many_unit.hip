// Forwarder to launch_repair_judge_many (csrc/kernels.hpp) for tests/test_gpu_repair_many_unit.py: device pointers and plain integers in,
// stream 0, the hipError_t out as an int.  Nothing is allocated, copied or checked here; the roots, the paths, the descriptor table and
// their guards are torch tensors of the test.  Built by the package Makefile as librepair_many_unit.so and linked against libcodex_p2.so
// (cp2k::launch_* are exported there), so what runs are the code objects the product ships.  The two kernels it is held against go through
// the forwarders that exist (libread_blocks_unit.so, libkernel_unit.so).  No entry point of the boundary (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" {

// reqs: n descriptors of 40 bytes (cp2k::RepairManyReq); slice: the most requests one launch takes (0: a whole grid's worth)
int rmu_repair_judge_many(const void* fresh, const void* paths, const void* reqs, size_t n, uint32_t* verdict, size_t slice) {
  return (int)cp2k::launch_repair_judge_many(fresh, paths, static_cast<const cp2k::RepairManyReq*>(reqs), n, verdict, nullptr, slice);
}

size_t rmu_req_bytes(void) { return sizeof(cp2k::RepairManyReq); }

}  // extern "C"
