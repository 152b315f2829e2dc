// Forwarder to launch_block_path_commit_many (csrc/kernels.hpp) for tests/test_gpu_fill_many_unit.py: device pointers and plain integers
// in, stream 0, the hipError_t out as an int.  Nothing is allocated, copied or checked here; the buffers and their guards are torch tensors
// of the test, and the session table is an array of 7 x 8 bytes per session as kernels.hpp lays FillManySession out.  Built by the package
// Makefile as libfill_many_unit.so and linked against libcodex_p2.so, so what runs is the code object the product ships.  No entry point
// of the boundary (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

static_assert(sizeof(cp2k::FillManySession) == 56, "the test lays a descriptor out as 7 x 8 bytes");

extern "C" int fmu_block_path_commit_many(const void* fresh, const void* paths, const void* sessions, uint64_t n_sessions, const uint64_t* session_of,
                                          const uint32_t* levels, const uint64_t* path_off, uint64_t path_base, const uint64_t* slot_block,
                                          const uint64_t* dest, const uint64_t* anchor_row, int keep_top, size_t n, uint32_t* verdict,
                                          void* scratch) {
  return (int)cp2k::launch_block_path_commit_many(fresh, paths, static_cast<const cp2k::FillManySession*>(sessions), n_sessions, session_of, levels,
                                                  path_off, path_base, slot_block, dest, anchor_row, keep_top != 0, n, verdict, scratch, nullptr);
}
