// Forwarders to launch_nodes_restore_layer and launch_nodes_restore_layers (csrc/kernels.hpp) for tests/test_gpu_fill_node_ckpt_unit.py: device
// pointers and plain integers in, stream 0, the hipError_t out as an int.  The layer tables of launch_nodes_restore_layers are host arrays, as
// the launcher takes them.  Nothing is allocated, copied or checked here; the buffers and their guards are torch tensors of the test.  Built
// by the package Makefile as libfill_node_ckpt_unit.so and linked against libcodex_p2.so, so what runs is the code object the product ships.
// No entry point of the boundary (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" int fnc_restore_layer(void* tree, const void* cand, uint8_t* flags, const void* slot_roots, uint64_t off_in, uint64_t m_in,
                                 uint64_t off_out, uint64_t n_local, int bottom, int top, uint64_t n_rows) {
  return (int)cp2k::launch_nodes_restore_layer(tree, cand, flags, slot_roots, off_in, m_in, off_out, n_local, bottom != 0, top != 0, n_rows, nullptr);
}

extern "C" int fnc_restore_layers(void* tree, const void* cand, uint8_t* flags, const void* slot_roots, const uint64_t* layer_off_host,
                                  const uint64_t* layer_size_host, uint32_t depth, uint64_t n_local, uint64_t n_rows) {
  return (int)cp2k::launch_nodes_restore_layers(tree, cand, flags, slot_roots, layer_off_host, layer_size_host, depth, n_local, n_rows, nullptr);
}
