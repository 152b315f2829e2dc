// Forwarder to launch_compress_layers_ragged (csrc/kernels.hpp) for tests/test_gpu_set_roots_many_unit.py: device pointers, host tables
// and plain integers in, stream 0, the hipError_t out as an int.  Nothing is allocated, copied or checked here; the tree buffer, the
// tables and their guards are torch tensors of the test.  Built by the package Makefile as libset_roots_many_unit.so and linked against
// libcodex_p2.so (cp2k::launch_* are exported there), so what runs is the code object the product ships.  No entry point of the boundary
// (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" {

int srm_compress_layers_ragged(void* rows, const uint64_t* tree_tab, const uint64_t* prefix, const uint32_t* tree_of, const uint64_t* level_off,
                               const uint64_t* level_cnt, const uint64_t* level_work, size_t n_levels) {
  return (int)cp2k::launch_compress_layers_ragged(rows, tree_tab, prefix, tree_of, level_off, level_cnt, level_work, n_levels, nullptr);
}

}  // extern "C"
