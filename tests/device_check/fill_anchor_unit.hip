// Forwarder to launch_block_path_commit_anchored (csrc/kernels.hpp) for tests/test_gpu_fill_anchor_unit.py: device pointers and plain
// integers in, stream 0, the hipError_t out as an int.  Nothing is allocated, copied or checked here; the buffers and their guards are torch
// tensors of the test.  Built by the package Makefile as libfill_anchor_unit.so and linked against libcodex_p2.so, so what runs is the code
// object the product ships.  No entry point of the boundary (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" int fau_block_path_commit_anchored(const void* fresh, const void* paths, const uint32_t* levels, const uint64_t* path_off,
                                              uint64_t path_base, const uint64_t* slot_block, const void* slot_roots, const uint64_t* dest,
                                              const uint64_t* anchor_row, const uint64_t* layer_off, const uint64_t* layer_size,
                                              uint64_t n_blocks, uint32_t depth, size_t n, uint32_t* verdict, void* tree, uint64_t n_rows,
                                              void* scratch) {
  return (int)cp2k::launch_block_path_commit_anchored(fresh, paths, levels, path_off, path_base, slot_block, slot_roots, dest, anchor_row, layer_off,
                                                      layer_size, n_blocks, depth, n, verdict, tree, n_rows, scratch, nullptr);
}
