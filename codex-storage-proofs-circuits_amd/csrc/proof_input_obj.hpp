// The proof-input object behind the C ABI (cp2_proof_input, include/codex_p2.h), shared by proof_input.cpp (producers, writer)
// and verify.cpp (parser, verifier).  Not installed.
#pragma once
#include <memory>
#include <vector>

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
