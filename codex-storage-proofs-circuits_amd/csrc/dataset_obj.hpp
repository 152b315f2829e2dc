// The dataset object behind the C ABI (cp2_dataset, include/codex_p2.h), shared by proof_input.cpp (builders, per-dataset proof
// inputs) and proof_many.cpp (proof inputs across datasets).  Not installed.
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "body_store.hpp"
#include "proof_export.hpp"   // proof_shape_refusal, slot_proof_of: the host-only pieces every proof-input route shares
#include "trees.hpp"

struct cp2_dataset {
  cp2_ctx* ctx = nullptr;
  cp2_config cfg{};
  std::string file_base;
  bool from_file = false;
  uint64_t first_slot = 0, n_local = 0;
  cp2_slot_trees* trees = nullptr;            // every local slot tree (null for a roots-only dataset)
  // Roots-only dataset: the slot trees of a dataset whose nodes do not fit the device (3.1 % of the data: 256 MiB per 8 GiB
  // slot, 8 TiB for config 5's nominal 32 768 slots) are built batch by batch in pooled scratch and dropped again, only the
  // 32-byte roots stay; the tree of a slot that is proved is rebuilt on demand (0.2 s per 8 GiB), which is what the reference
  // does on EVERY run and once more per sample (gen_input/bn254.nim:42,57).
  cp2i::DevBuf local_roots;                   // roots-only: n_local x 32 bytes
  // Compact dataset (between the two): of every local slot tree the part from the BLOCK ROOTS up stays (2 x nBlocks - 1 nodes:
  // 8 MiB per 8 GiB slot, 1/32 of the full tree), layer-major over the local slots: layer k of slot s starts at element
  // coff[k] + s * csizes[k].  The bottom of a path -- inside one network block -- is recomputed from the block's own cells
  // (<= nSamples blocks of 64 KiB per proof input: SURVEY.md section 7, "keep only block roots + upper layers and re-hash the
  // touched blocks"), checked against the stored block root.
  cp2i::DevBuf compact;
  std::vector<size_t> csizes, coff;
  int tree_mode = 1;                          // 1 every node resident, 2 compact, 0 roots only
  bool have_roots = false;
  std::vector<size_t> dsizes;                 // dataset-tree layer sizes
  std::vector<uint8_t> dlayers;               // all dataset-tree layers, bottom first (host copy)
  // streamed build: one JSON body (", \"cellData\": ... }") per local slot, made while later slots were hashing
  bool prepared = false;
  uint8_t prep_entropy[32] = {};
  BodyStore bodies;
  // cp2_datasets_build_many: what this dataset keeps (`trees->nodes`, `compact` or `local_roots`, then a borrowed view) is a slice of an
  // allocation shared with other datasets of the same call; the allocation goes with the last of them
  std::shared_ptr<cp2i::DevBuf> arena;
  ~cp2_dataset() { cp2_slot_trees_free(trees); }
};

// The field modulus r as four little-endian 64-bit words (README.md:76 of the reference), and a 32-byte value reduced into [0, r):
// `Entropy` is a field element in the reference (types/bn254.nim:21), so what is stored and printed is the canonical
// representative even when the caller hands in 32 arbitrary bytes (at most five subtractions: 2^256 / r < 5.3).
inline constexpr uint64_t FR_MODULUS_LE64[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
inline void canonical_felt(const uint8_t in[32], uint8_t out[32]) {
  uint64_t w[4];
  std::memcpy(w, in, 32);
  for (;;) {
    bool ge = true;
    for (int i = 3; i >= 0; --i)
      if (w[i] != FR_MODULUS_LE64[i]) { ge = w[i] > FR_MODULUS_LE64[i]; break; }
    if (!ge) break;
    unsigned __int128 borrow = 0;
    for (int i = 0; i < 4; ++i) {
      unsigned __int128 d = (unsigned __int128)w[i] - FR_MODULUS_LE64[i] - borrow;
      w[i] = (uint64_t)d;
      borrow = (d >> 64) & 1;
    }
  }
  std::memcpy(out, w, 32);
}

// the device buffer holding the roots of the local slots (n_local x 32 bytes)
const void* dataset_roots_dev(const cp2_dataset* ds);
// slotProof of a slot of a dataset whose dataset tree is set (slot_proof_of, proof_export.hpp)
inline void fill_slot_proof(const cp2_dataset* ds, uint64_t slot_idx, std::vector<uint8_t>& out) {
  cp2i::slot_proof_of(ds->dlayers, ds->dsizes, ds->cfg.n_slots, (size_t)ds->cfg.max_log2_nslots, slot_idx, out);
}
// What proof_shape_refusal (proof_export.hpp) is asked about a built dataset: the depth of every slot tree of the configuration -- the
// block tree under the tree over the block roots, what cp2_slot_trees_depth says of built trees -- and of the tree over its slot roots
inline size_t config_slot_tree_depth(const cp2_config& c) {
  const size_t cpb = c.block_size / c.cell_size;
  return (cp2i::layer_sizes_of(cpb).size() - 1) + (cp2i::layer_sizes_of(c.n_cells / cpb).size() - 1);
}
inline size_t config_dataset_tree_depth(const cp2_config& c) { return cp2i::layer_sizes_of(c.n_slots).size() - 1; }

// What cp2_datasets_build_many (build_many.cpp) shares with cp2_dataset_build (proof_input.cpp): the request checks, the object, the
// named mode (0 / 1 / 2; -1 with the context's error set: CODEX_P2_KEEP_TREES is malformed; -2: automatic), the automatic choice over
// totals, the sizes the choice and the batches go by, one build attempt in a given mode and the step down after an allocation failure.
int dataset_check(const cp2_config* cfg, uint64_t first_slot, uint64_t n_local);
cp2_dataset* dataset_new(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local);
int dataset_named_mode(cp2_ctx* ctx, bool* automatic);
int dataset_mode_that_fits(cp2_ctx* ctx, unsigned __int128 data, unsigned __int128 nodes_all, unsigned __int128 compact_all,
                           unsigned __int128 in_flight);
size_t compact_bytes(const cp2_config& c, size_t n_slots);
size_t dataset_kept_layout(cp2_dataset* ds, int mode);   // compact / roots only: sets tree_mode, csizes and coff; the bytes of what is kept
int dataset_build_in_mode(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, int mode, cp2_dataset** out);
bool step_down(cp2_ctx* ctx, int* mode, const char* what);

namespace cp2i {
// The one pass that makes proof inputs for n (dataset, slot, entropy) requests of one circuit (proof_many.cpp): every request's
// out[i], or none.  `named`: error texts start with "request <at0 + i>: " (the *_many entry points) or with nothing (the compact
// branch of cp2_proof_inputs_generate_batch).  proof_many.cpp and proof_input.cpp call each other here: a compact one-dataset batch
// comes in through this, and a roots-only request goes back out through cp2_proof_inputs_generate_batch, one slot at a time.
int prove_requests(cp2_ctx* ctx, cp2_dataset* const* ds, const uint64_t* slot_idx, const uint8_t* entropies, size_t n, size_t at0,
                   bool named, cp2_proof_input** out);
// The dataset trees of n datasets of one context in one pass (set_roots_many.cpp): what cp2_dataset_set_roots(ds[i], all_roots[i]) leaves
// behind for every i, or no dataset changed.  Already validated by the caller: no dataset twice, and where all_roots or all_roots[i] is
// NULL every slot of ds[i] is local.  own (n, may be NULL): whether request i's own rows of the roots equal its built roots.
int set_roots_pass(cp2_ctx* ctx, cp2_dataset* const* ds, const uint8_t* const* all_roots, size_t n, uint8_t* own);
}  // namespace cp2i
