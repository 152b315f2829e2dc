// Forwarders to the launch wrappers of csrc/kernels.hpp, one per launcher that tests/test_gpu_kernel_units.py checks on its own:
// device pointers and plain integers in, stream 0, the hipError_t out as an int.  Nothing is allocated, copied or checked here; the
// buffers and their guards are torch tensors of the test.  Built by the package Makefile as libkernel_unit.so and linked against
// libcodex_p2.so (cp2k::launch_* are exported there), so what runs are the code objects the product ships.  No entry point of the
// boundary (include/codex_p2.h) comes from here.
#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

extern "C" {

size_t ku_sizeof_tree_geom() { return sizeof(cp2k::TreeGeom); }
size_t ku_sizeof_many_req() { return sizeof(cp2k::ManyReq); }
size_t ku_sizeof_verify_geom() { return sizeof(cp2k::VerifyGeom); }
size_t ku_scrub_tile() { return cp2k::SCRUB_TILE; }

int ku_scrub_compare(const void* fresh, size_t fstride, const void* kept, size_t kstride, size_t rows, size_t n_items, uint64_t* bits,
                     uint32_t* counts) {
  return (int)cp2k::launch_scrub_compare(fresh, fstride, kept, kstride, rows, n_items, bits, counts, nullptr);
}

int ku_repair_compare(const void* fresh, const void* kept, size_t kept_rows, const uint64_t* rows, size_t n, uint32_t* verdict) {
  return (int)cp2k::launch_repair_compare(fresh, kept, kept_rows, rows, n, verdict, nullptr);
}

int ku_sample_paths(const cp2k::TreeGeom* g, const void* nodes, const void* d_entropy, const uint64_t* slots, uint64_t slot0, size_t n_items,
                    uint32_t ns, uint32_t md, uint64_t* indices, uint64_t* gcell, uint64_t* rows) {
  return (int)cp2k::launch_sample_paths(*g, nodes, d_entropy, slots, slot0, n_items, ns, md, indices, gcell, rows, nullptr);
}

int ku_sample_many(const cp2k::ManyReq* reqs, const cp2k::TreeGeom* geoms, size_t n_req, uint32_t ns, uint32_t md, uint64_t* indices,
                   uint64_t* blocks, uint64_t* addr) {
  return (int)cp2k::launch_sample_many(reqs, geoms, n_req, ns, md, indices, blocks, addr, nullptr);
}

int ku_gather_rows(const void* src, const uint64_t* index, size_t nrows, size_t row_bytes, void* out) {
  return (int)cp2k::launch_gather_rows(src, index, nrows, row_bytes, out, nullptr);
}

int ku_gather_addr(const uint64_t* addr, size_t nrows, size_t row_bytes, void* out) {
  return (int)cp2k::launch_gather_addr(addr, nrows, row_bytes, out, nullptr);
}

int ku_gen_fake_cells(uint64_t seed0, uint64_t cells_per_slot, uint64_t first, const uint64_t* list, size_t n_cells, size_t cell_size, void* out,
                      uint64_t units_per_slot, uint64_t first_unit) {
  return (int)cp2k::launch_gen_fake_cells(seed0, cells_per_slot, first, list, n_cells, cell_size, out, nullptr, units_per_slot, first_unit);
}

int ku_gen_fake_cells_many(const uint64_t* seeds, const uint64_t* firsts, uint64_t per, size_t n_rows, size_t cell_size, void* out) {
  return (int)cp2k::launch_gen_fake_cells_many(seeds, firsts, per, n_rows, cell_size, out, nullptr);
}

int ku_compress_layer(const void* in, void* out, size_t m_in, size_t nseg, int bottom, size_t in_seg_stride, size_t out_seg_stride) {
  return (int)cp2k::launch_compress_layer(in, out, m_in, nseg, bottom != 0, in_seg_stride, out_seg_stride, nullptr);
}

int ku_block_path_roots(const void* fresh, const void* paths, const uint64_t* root_block, const void* slot_roots, uint64_t n_blocks,
                        uint32_t depth, size_t n, uint32_t* verdict, void* roots_out) {
  return (int)cp2k::launch_block_path_roots(fresh, paths, root_block, slot_roots, n_blocks, depth, n, verdict, roots_out, nullptr);
}

int ku_block_path_commit(const void* fresh, const void* paths, const uint64_t* slot_block, const void* slot_roots, const uint64_t* dest,
                         uint64_t n_blocks, uint32_t depth, size_t n, uint32_t* verdict, void* layer0, uint64_t n_rows) {
  return (int)cp2k::launch_block_path_commit(fresh, paths, slot_block, slot_roots, dest, n_blocks, depth, n, verdict, layer0, n_rows, nullptr);
}

int ku_verify_samples(const cp2k::VerifyGeom* g, const uint64_t* prm, const void* heads, const void* cells, const void* paths, uint8_t* ok) {
  return (int)cp2k::launch_verify_samples(*g, prm, heads, cells, paths, ok, nullptr);
}

}  // extern "C"
