// The proof-input object behind the C ABI (cp2_proof_input, include/codex_p2.h), shared by proof_input.cpp (producers, writer),
// proof_many.cpp (the pass over many requests) and verify.cpp (parser, verifier), and the one function that makes such objects from a
// pass's BatchStore (proof_inputs_from_store: it reads the dataset object, so dataset_obj.hpp comes with this header).  Not installed.
#pragma once
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "dataset_obj.hpp"
#include "internal.hpp"

// cell bytes, Merkle paths and indices of a whole batch live in pinned blocks that every proof input of the batch
// shares (one download each, no per-slot copies); the blocks return to the context's pool with the last reference
struct BatchStore {
  cp2i::PinBuf idx, paths, leaves, cells;
  std::vector<uint8_t> cells_heap;   // SlotFile / Host sources: sampled cells are read on the host
  std::vector<uint8_t> heap;         // cp2_proof_input_create: everything copied from the caller
};

struct cp2_proof_input {
  cp2_config cfg{};
  uint64_t slot_idx = 0;
  uint8_t entropy[32], dataset_root[32], slot_root[32];
  size_t n_samples = 0;
  std::vector<uint8_t> slot_proof;
  std::shared_ptr<BatchStore> store;
  const uint64_t* indices = nullptr;    // nSamples, inside store->idx
  const uint8_t* cell_data = nullptr;   // nSamples x cellSize, inside store->cells / cells_heap
  const uint8_t* paths = nullptr;       // nSamples x maxDepth x 32, inside store->paths
  const uint8_t* leaves = nullptr;      // nSamples x 32: hash of each sampled cell (may be null for caller-made inputs)
  const uint8_t* cell_felts = nullptr;  // nSamples x cp2_felts_per_bytes(cellSize) x 32: set on parsed inputs only (cell_data is then NULL unless every row encodes bytes)
};

// The objects of one pass over `store`: item j is slot `slot` of `ds` under the canonical `entropy`, its samples are rows
// [j * nSamples, (j + 1) * nSamples) of the store's arrays (`cells`: store->cells or store->cells_heap) and its object goes to *out.
// All items are of one circuit.  All or nothing: CP2_ERR_ALLOC leaves every *out NULL.
struct ProofItem {
  const cp2_dataset* ds;
  uint64_t slot;
  const uint8_t* entropy;
  cp2_proof_input** out;
};
inline int proof_inputs_from_store(const ProofItem* items, size_t n, const std::shared_ptr<BatchStore>& store, const uint8_t* cells) {
  for (size_t j = 0; j < n; ++j) {
    const cp2_dataset* ds = items[j].ds;
    const size_t ns = ds->cfg.n_samples, md = (size_t)ds->cfg.max_depth, cs = ds->cfg.cell_size;
    cp2_proof_input* p = new (std::nothrow) cp2_proof_input();
    if (!p) {
      for (size_t k = 0; k < j; ++k) { delete *items[k].out; *items[k].out = nullptr; }
      return CP2_ERR_ALLOC;
    }
    p->cfg = ds->cfg;
    p->slot_idx = items[j].slot;
    std::memcpy(p->entropy, items[j].entropy, 32);
    std::memcpy(p->dataset_root, &ds->dlayers[ds->dlayers.size() - 32], 32);
    std::memcpy(p->slot_root, &ds->dlayers[items[j].slot * 32], 32);     // layer 0 of the dataset tree = slot roots
    fill_slot_proof(ds, items[j].slot, p->slot_proof);
    p->n_samples = ns;
    p->store = store;
    if (ns) {
      p->indices = static_cast<const uint64_t*>(store->idx.p) + j * ns;
      p->cell_data = cells + j * ns * cs;
      p->paths = store->paths.u8() + j * ns * md * 32;
      p->leaves = store->leaves.u8() + j * ns * 32;
    }
    *items[j].out = p;
  }
  return CP2_OK;
}
