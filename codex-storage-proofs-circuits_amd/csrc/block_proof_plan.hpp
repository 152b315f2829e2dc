// The host side of block proofs (csrc/block_proofs.cpp): how long the proof of a network block is, where the siblings of its path are
// kept in a dataset's node buffer, in which order and under which key reconstructRoot (reference/nim/proof_input/src/merkle.nim:51-74)
// compresses them, and which requests a check accepts.  No HIP in here: tests/host_check/block_proof_plan_check.cpp walks it over random
// geometries and request sets on the CPU, under AddressSanitizer + UBSan.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "repair_plan.hpp"

namespace cp2i {

// a path entry the tree does not hold (the sibling index lies past its layer's end): gathered as zeros, as merkleProof pads
// (merkle.nim:33-34).  The value of NO_ROW (trees.hpp).
constexpr uint64_t BLOCK_PROOF_NO_ROW = ~0ULL;

// ---- the proof's length -----------------------------------------------------------------------------------------------------------
// The big tree over n_blocks block roots has layers n, ceil(n / 2), ... 1 and its bottom layer always gets one round of compression
// (merkle/bn254.nim:29-58), so the proof of a block holds ceil(log2(n_blocks)) siblings, and ONE for a slot of a single block (the
// singleton is compressed once, with key 3, against zero).  0 for n_blocks == 0.  Never padded: this proof is not circuit input.
inline size_t block_proof_depth(uint64_t n_blocks) {
  if (n_blocks == 0) return 0;
  size_t d = 1;
  for (uint64_t m = (n_blocks + 1) >> 1; m > 1; m = (m + 1) >> 1) ++d;
  return d;
}

// ---- where the siblings are kept (32-byte rows of the dataset's node buffer) ----------------------------------------------------------
// Layer l of the big tree of local slot `local` starts at row layer_off + local * layer_size in both layouts: every node kept
// (cp2_slot_trees: layer_off = toff[l], layer_size = tsizes[l]) and compact (cp2_dataset: coff[l], csizes[l]).  The sibling of block
// `block` on level l is node (block >> l) ^ 1 of that layer; past the layer's end (an odd layer's last node, the singleton) the path
// holds zero.
inline uint64_t block_proof_sibling_row(uint64_t layer_off, uint64_t layer_size, uint64_t local, uint64_t block, size_t level) {
  const uint64_t sib = (block >> level) ^ 1;
  return sib < layer_size ? layer_off + local * layer_size + sib : BLOCK_PROOF_NO_ROW;
}
// the `depth` sibling rows of one request, bottom first; offs / sizes hold at least `depth` layers (toff / tsizes, or coff / csizes)
template <class Offs, class Sizes>
inline void block_proof_rows(const Offs& offs, const Sizes& sizes, uint64_t local, uint64_t block, size_t depth, uint64_t* rows) {
  for (size_t l = 0; l < depth; ++l) rows[l] = block_proof_sibling_row(offs[l], sizes[l], local, block, l);
}
// The block root itself is the row repair compares with: repair_row_full / repair_row_compact (repair_plan.hpp).

// ---- reconstructRoot's schedule -----------------------------------------------------------------------------------------------------
// merkle.nim:51-74 with running index j and layer size m, starting at (block, n_blocks): on every level
//   j odd                 h = compress(sibling, h, key)        the node is the RIGHT child
//   j even and j == m - 1 h = compress(h, sibling, key + 2)    the odd tail: the sibling is the zero merkleProof wrote
//   j even otherwise      h = compress(h, sibling, key)
// with key = 1 on level 0 (the bottom layer) and 0 above; then j >>= 1, m = (m + 1) >> 1.  k_block_path_roots (kernels.hip) computes
// exactly these two values per level and lane, `right` as a limb mask and the key by arithmetic.
struct BlockPathStep {
  bool right;      // the running node is the right input of the compression
  uint32_t key;    // 0..3
};
inline std::vector<BlockPathStep> block_proof_schedule(uint64_t n_blocks, uint64_t block) {
  std::vector<BlockPathStep> s(block_proof_depth(n_blocks));
  uint64_t j = block, m = n_blocks;
  for (size_t l = 0; l < s.size(); ++l) {
    const uint32_t odd = (uint32_t)(j & 1), last = j == m - 1 ? 1u : 0u;
    s[l].right = odd != 0;
    s[l].key = (l == 0 ? 1u : 0u) + 2u * (last & (odd ^ 1u));
    j >>= 1;
    m = (m + 1) >> 1;
  }
  return s;
}

// ---- validation -------------------------------------------------------------------------------------------------------------------
// cp2_blocks_verify: requests are (index into the caller's slot roots, block of the slot) pairs.  Every root index below n_roots, every
// block below n_blocks; the same pair twice is allowed (two peers may send the same block).  false with *err naming the lowest request
// index that breaks a rule.
inline bool block_verify_validate(const uint64_t* root_block, size_t n, uint64_t n_roots, uint64_t n_blocks, std::string* err) {
  for (size_t i = 0; i < n; ++i) {
    const uint64_t r = root_block[2 * i], b = root_block[2 * i + 1];
    if (r >= n_roots) {
      *err = "block verify: request " + std::to_string(i) + ": root index " + std::to_string(r) + " is not below n_roots = " + std::to_string(n_roots);
      return false;
    }
    if (b >= n_blocks) {
      *err = "block verify: request " + std::to_string(i) + ": block " + std::to_string(b) + " is not below nBlocks = " + std::to_string(n_blocks);
      return false;
    }
  }
  return true;
}
// cp2_dataset_block_proofs: (dataset slot, block of the slot) pairs, every slot inside [first_slot, first_slot + n_local), every block
// below n_blocks; repeats are allowed (serving is read-only).  false with *err naming the lowest request index that breaks a rule.
inline bool block_proofs_validate(const uint64_t* slot_block, size_t n, uint64_t first_slot, uint64_t n_local, uint64_t n_blocks, std::string* err) {
  for (size_t i = 0; i < n; ++i) {
    const uint64_t s = slot_block[2 * i], b = slot_block[2 * i + 1];
    if (s < first_slot || s - first_slot >= n_local) {
      *err = "block proofs: request " + std::to_string(i) + ": slot " + std::to_string(s) + " is not inside the local range " +
             std::to_string(first_slot) + " + " + std::to_string(n_local);
      return false;
    }
    if (b >= n_blocks) {
      *err = "block proofs: request " + std::to_string(i) + ": block " + std::to_string(b) + " of slot " + std::to_string(s) +
             " is not below nBlocks = " + std::to_string(n_blocks);
      return false;
    }
  }
  return true;
}

}  // namespace cp2i
