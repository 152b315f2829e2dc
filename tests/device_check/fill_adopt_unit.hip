// Forwarders to launch_adopt_layers and launch_adopt_resolve (csrc/kernels.hpp) for tests/test_gpu_fill_adopt_unit.py: device pointers and
// plain integers in, stream 0, the hipError_t out as an int.  The layer tables of launch_adopt_layers are host arrays, those of
// launch_adopt_resolve device arrays, as the launchers take them.  Nothing is allocated, copied or checked here; the buffers and their guards
// are torch tensors of the test.  Built by the package Makefile as libfill_adopt_unit.so and linked against libcodex_p2.so, so what runs is
// the code object the product ships.  No entry point of the boundary (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" int fad_adopt_layers(const void* tree, void* cand, uint8_t* flags, const void* slot_roots, const uint64_t* layer_off_host,
                                const uint64_t* layer_size_host, uint32_t depth, uint64_t n_local, uint64_t first_sel, uint64_t n_sel,
                                uint64_t n_rows) {
  return (int)cp2k::launch_adopt_layers(tree, cand, flags, slot_roots, layer_off_host, layer_size_host, depth, n_local, first_sel, n_sel, n_rows,
                                        nullptr);
}

extern "C" int fad_adopt_resolve(void* tree, const void* cand, const uint8_t* flags, uint8_t* out, const uint64_t* layer_off,
                                 const uint64_t* layer_size, uint32_t depth, uint64_t n_local, uint64_t first_sel, uint64_t n_sel, uint64_t n_below,
                                 uint64_t n_rows) {
  return (int)cp2k::launch_adopt_resolve(tree, cand, flags, out, layer_off, layer_size, depth, n_local, first_sel, n_sel, n_below, n_rows, nullptr);
}
