// Forwarder to launch_finish_layers_many (csrc/kernels.hpp) for tests/test_gpu_fill_finish_many_unit.py and tools/fill_finish_many_rate.py:
// device pointers, host tables and plain integers in, stream 0, the hipError_t out as an int.  Nothing is allocated, copied or checked
// here; the session buffers, the tables and their guards are torch tensors of the caller.  Built by the package Makefile as
// libfill_finish_many_unit.so and linked against libcodex_p2.so (cp2k::launch_* are exported there), so what runs is the code object the
// product ships.  No entry point of the boundary (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" {

int ffm_finish_layers_many(const void* sessions, uint64_t n_sessions, const uint64_t* voff, const uint64_t* prefix, const uint32_t* sess_of,
                           const uint64_t* level_off, const uint64_t* level_cnt, const uint64_t* level_work, size_t n_levels, uint32_t* verdict) {
  return (int)cp2k::launch_finish_layers_many(static_cast<const cp2k::FillManySession*>(sessions), n_sessions, voff, prefix, sess_of, level_off,
                                              level_cnt, level_work, n_levels, verdict, nullptr);
}

}  // extern "C"
