// The host side of cp2_datasets_build_many (csrc/build_many.cpp): how the requests of one call become work.  File-sourced requests are
// grouped into CLASSES of equal (cell size, block size, cells per slot); a class's ITEMS are its (request, local slot) pairs in request
// order -- a request of n_local slots is n_local consecutive items, which may straddle a batch boundary --; a class runs in BATCHES cut by
// the compact build's rule (half a staging chunk of nodes, at least one item).  A finished batch holds every layer of its items
// layer-major; what the call's mode keeps of it is copied, layer by layer, to where each item's dataset keeps that layer: the plan gives
// the row of every kept layer inside the batch and inside the request's own buffer, and fills the table of absolute addresses that
// k_scatter_rows_addr writes through.  Pure arithmetic over offsets -- no HIP in here: tests/host_check/build_many_plan_check.cpp runs it
// on the CPU under AddressSanitizer + UBSan and tests/build_many_models.py restates it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "batch_loop.hpp"   // batch_items

namespace cp2i {

// what the plan knows of one request (already validated: block_size a multiple of cell_size, n_cells a multiple of cells per block)
struct BuildRequest {
  size_t cell_size = 0, block_size = 0;
  uint64_t n_cells = 0, first_slot = 0, n_local = 0;
  bool from_file = false;
};

// layer sizes of a tree over n leaves, bottom first: n, ceil(n / 2), ... 1, the bottom layer always compressed once (layer_sizes_of)
inline std::vector<uint64_t> build_many_layer_sizes(uint64_t n) {
  std::vector<uint64_t> s;
  if (n == 0) return s;
  bool bottom = true;
  for (uint64_t m = n;; m = (m + 1) / 2, bottom = false) {
    s.push_back(m);
    if (m == 1 && !bottom) break;
  }
  return s;
}

// The kept layers of one geometry under one mode.  Per kept layer: `rows` per item; `src_prefix`, the rows per item of every layer
// that lies before it in a batch (a batch of n items holds the layer at row n * src_prefix, item j at + j * rows: trees_layout's
// layer-major order, the block-tree layers below their roots first, then the big tree's); `dst_prefix`, the same inside what a request
// keeps (a request of n_local slots keeps the layer at row n_local * dst_prefix, local slot s at + s * rows).
//   mode 1  every node: every layer of the batch, src_prefix == dst_prefix (the request's own cp2_slot_trees has trees_layout's layout)
//   mode 2  compact: the big tree's layers, from the block roots up (dataset_alloc_kept: coff[k] + s * csizes[k])
//   mode 0  roots only: the big tree's last layer, row s of local_roots
struct BuildLayers {
  std::vector<uint64_t> rows, src_prefix, dst_prefix;
  uint64_t item_rows = 0;       // every layer of one item: what a batch holds of it (trees_node_bytes / 32)
  uint64_t kept_rows = 0;       // what one local slot keeps
  size_t n() const { return rows.size(); }
};

inline BuildLayers build_many_layers(size_t cell_size, size_t block_size, uint64_t n_cells, int mode) {
  BuildLayers L;
  const uint64_t cpb = block_size / cell_size, nblocks = n_cells / cpb;
  const std::vector<uint64_t> b = build_many_layer_sizes(cpb), t = build_many_layer_sizes(nblocks);
  uint64_t src = 0;
  for (size_t k = 0; k + 1 < b.size(); ++k) {           // the block roots are layer 0 of the big tree
    if (mode == 1) { L.rows.push_back(nblocks * b[k]); L.src_prefix.push_back(src); L.dst_prefix.push_back(src); }
    src += nblocks * b[k];
  }
  uint64_t dst = mode == 1 ? src : 0;
  for (size_t k = 0; k < t.size(); ++k) {
    if (mode != 0 || k + 1 == t.size()) { L.rows.push_back(t[k]); L.src_prefix.push_back(src); L.dst_prefix.push_back(mode == 0 ? 0 : dst); }
    src += t[k];
    dst += t[k];
  }
  L.item_rows = src;
  for (uint64_t r : L.rows) L.kept_rows += r;
  return L;
}

inline uint64_t build_many_src_row(const BuildLayers& L, size_t layer, uint64_t batch_items) { return batch_items * L.src_prefix[layer]; }
inline uint64_t build_many_dst_row(const BuildLayers& L, size_t layer, uint64_t n_local, uint64_t local) {
  return n_local * L.dst_prefix[layer] + local * L.rows[layer];
}

struct BuildClass {
  size_t cell_size = 0, block_size = 0;
  uint64_t n_cells = 0;
  std::vector<size_t> request;          // per item
  std::vector<uint64_t> local;          // per item: local slot of its request
  size_t batch = 1;
  size_t n_items() const { return request.size(); }
  size_t n_batches() const { return (n_items() + batch - 1) / batch; }
};

struct BuildPlan {
  std::vector<BuildClass> classes;      // in order of first appearance
  std::vector<size_t> fake;             // the fake-source requests, built one by one
  size_t n_items = 0, n_batches = 0;    // over the classes
};

inline BuildPlan build_many_plan(const std::vector<BuildRequest>& req, size_t stage_bytes) {
  BuildPlan p;
  for (size_t i = 0; i < req.size(); ++i) {
    const BuildRequest& r = req[i];
    if (!r.from_file) { p.fake.push_back(i); continue; }
    BuildClass* k = nullptr;
    for (auto& q : p.classes)
      if (q.cell_size == r.cell_size && q.block_size == r.block_size && q.n_cells == r.n_cells) { k = &q; break; }
    if (!k) {
      p.classes.emplace_back();
      k = &p.classes.back();
      k->cell_size = r.cell_size;
      k->block_size = r.block_size;
      k->n_cells = r.n_cells;
    }
    for (uint64_t s = 0; s < r.n_local; ++s) { k->request.push_back(i); k->local.push_back(s); }
  }
  for (auto& k : p.classes) {
    k.batch = batch_items(stage_bytes, build_many_layers(k.cell_size, k.block_size, k.n_cells, 1).item_rows * 32, k.n_items());   // every build's rule
    p.n_items += k.n_items();
    p.n_batches += k.n_batches();
  }
  return p;
}

// The address table of the batch that holds items [i0, i0 + n) of class k: entry layer * n + j is the absolute address of row 0 of what
// item i0 + j's request keeps of that kept layer, base[request] being the address of row 0 of the request's own buffer (0: the request
// keeps nothing, every entry of it is 0 and k_scatter_rows_addr leaves its rows alone).  false -- nothing may be launched -- when an
// entry's rows would not lie inside [base, base + kept_rows of the request * 32): never, for a base that has the plan's own size.
inline bool build_many_addr_table(const BuildClass& k, const BuildLayers& L, const std::vector<BuildRequest>& req, const uint64_t* base,
                                  size_t i0, size_t n, uint64_t* out) {
  for (size_t layer = 0; layer < L.n(); ++layer)
    for (size_t j = 0; j < n; ++j) {
      const size_t r = k.request[i0 + j];
      if (base[r] == 0) { out[layer * n + j] = 0; continue; }
      const uint64_t row = build_many_dst_row(L, layer, req[r].n_local, k.local[i0 + j]);
      if (k.local[i0 + j] >= req[r].n_local || row + L.rows[layer] > req[r].n_local * L.kept_rows) return false;
      out[layer * n + j] = base[r] + row * 32;
    }
  return true;
}

// ---- refusals: before any device or file work -----------------------------------------------------------------------------------------
// The words for a request that dataset_check / trees_check_geometry refuse (proof_input.cpp, slot_trees.cpp: those decide; this names the
// first rule broken, in their order).  max_cell: the slot.nim:60-61 cap on the cells of slot files.  Empty: nothing found to name.
inline std::string build_many_refusal(uint64_t n_slots, uint64_t first_slot, uint64_t n_local, int max_depth, int max_log2_nslots, uint64_t cell_size,
                                      uint64_t block_size, uint64_t n_cells, bool from_file, uint64_t max_cell) {
  if (n_local == 0) return "n_local is 0";
  if (first_slot > n_slots || n_local > n_slots - first_slot)
    return "slots " + std::to_string(first_slot) + " + " + std::to_string(n_local) + " are not inside the dataset's " + std::to_string(n_slots);
  if (max_depth < 0 || max_log2_nslots < 0) return "max_depth and max_log2_nslots must not be negative";
  if (from_file && cell_size > max_cell) return "slot-file cells of " + std::to_string(cell_size) + " bytes (at most " + std::to_string(max_cell) + ")";
  if (cell_size == 0 || block_size == 0 || n_cells == 0) return "cell_size, block_size and n_cells must not be 0";
  if (block_size % cell_size != 0) return "block_size " + std::to_string(block_size) + " is no multiple of cell_size " + std::to_string(cell_size);
  if (n_cells % (block_size / cell_size) != 0)
    return "n_cells " + std::to_string(n_cells) + " is no multiple of the " + std::to_string(block_size / cell_size) + " cells of a block";
  if (cell_size > ((uint64_t)1 << 30) || n_cells > ((uint64_t)1 << 40) || n_local > ((uint64_t)1 << 32) ||
      (unsigned __int128)n_cells * n_local > ((unsigned __int128)1 << 44))
    return "a geometry beyond what the kernels address";
  return std::string();
}

}  // namespace cp2i
