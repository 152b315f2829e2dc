// The host side of a fill session (csrc/fill.cpp: cp2_fill_begin / _add / _missing / _finish): which sessions and requests are accepted,
// where a proved block root goes in the compact layout, which blocks are present, how the device's verdicts become NEW / DUPLICATE, how a
// failed write takes its blocks back, the ordered list of what is missing, and when a session may finish; for a session that serves
// (cp2_fill_keep_nodes, cp2_fill_block_proofs): which rows of the compact layout hold authentic nodes, and which proofs can be served; for
// an add whose paths stop at a node the session holds (cp2_fill_anchors, cp2_fill_add_anchored): the lowest such node of a block, which
// stated levels are accepted, the packed tables the device reads and the rows a proved request makes known.  No HIP in here:
// tests/host_check/fill_plan_check.cpp, fill_nodes_check.cpp and fill_anchor_check.cpp walk it over random geometries and request sets on
// the CPU, under AddressSanitizer + UBSan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "block_proof_plan.hpp"
#include "repair_plan.hpp"

namespace cp2i {

// the per-request results of cp2_fill_add: the values of CP2_FILL_* (include/codex_p2.h)
constexpr uint32_t FILL_NEW = 0, FILL_MISMATCH = 1, FILL_DUPLICATE = 2, FILL_UNWRITTEN = 3;
// what the writer (repair_write) takes and leaves: the values of CP2_REPAIR_MATCH / _MISMATCH / _UNWRITTEN
constexpr uint32_t FILL_WRITE = 0, FILL_SKIP = 1, FILL_WRITE_FAILED = 2;
// the per-request results of cp2_fill_block_proofs: the values of CP2_FILL_PROOF_* (include/codex_p2.h)
constexpr uint32_t FILL_PROOF_OK = 0, FILL_PROOF_ABSENT = 1, FILL_PROOF_PARTIAL = 2;

// ---- the session's range -----------------------------------------------------------------------------------------------------------
// What cp2_dataset_build asks of (cfg, first_slot, n_local) before it looks at the geometry, and the power of two proof inputs need
// (sample/bn254.nim:19-20).  max_cell: the largest cell a slot file holds (0: fake source, no limit).
inline bool fill_check_range(uint64_t n_slots, uint64_t first_slot, uint64_t n_local, int max_depth, int max_log2_nslots, uint64_t n_cells,
                             uint64_t cell_size, uint64_t max_cell, std::string* err) {
  if (n_local == 0 || first_slot > n_slots || n_local > n_slots - first_slot) {   // (no wrap-around)
    *err = "fill: slots " + std::to_string(first_slot) + " + " + std::to_string(n_local) + " are not a range inside the dataset's " +
           std::to_string(n_slots);
    return false;
  }
  if (max_depth < 0 || max_log2_nslots < 0) {
    *err = "fill: negative maxDepth or maxLog2NSlots";
    return false;
  }
  if (n_cells == 0 || (n_cells & (n_cells - 1))) {
    *err = "fill: nCells = " + std::to_string(n_cells) + " is not a power of two";
    return false;
  }
  if (max_cell && cell_size > max_cell) {
    *err = "fill: slot files hold cells of at most " + std::to_string(max_cell) + " bytes";
    return false;
  }
  return true;
}

// ---- the session ------------------------------------------------------------------------------------------------------------------
struct FillPlan {
  uint64_t first_slot = 0, n_local = 0, n_blocks = 0;
  // the compact layout of n_local slot trees (cp2_dataset: csizes / coff): layer k of local slot s starts at row coff[k] + s * csizes[k];
  // layer 0 holds the block roots, the last layer the slot roots
  std::vector<size_t> csizes, coff;
  size_t rows = 0;                       // rows of all layers
  std::vector<uint64_t> bits;            // bit (local * n_blocks + block): the block is proved AND written; the authority on presence
  uint64_t n_present = 0;
  bool finished = false;
  // a session that serves (cp2_fill_keep_nodes): bit r: row r of the compact layout holds the authentic node of its place in the tree,
  // stored by a proved path (mark_proved) or built from children that were (derive_from_presence).  All clear until nodes are kept.
  std::vector<uint64_t> known;
  bool keeps_nodes = false;

  // layer sizes n, ceil(n / 2), ... 1 with at least one round of compression (merkle/bn254.nim:29-58, layer_sizes_of)
  void init(uint64_t first, uint64_t local, uint64_t blocks) {
    first_slot = first; n_local = local; n_blocks = blocks;
    csizes.clear(); coff.clear();
    rows = 0;
    bool bottom = true;
    for (size_t m = (size_t)blocks; blocks;) {
      csizes.push_back(m);
      coff.push_back(rows);
      rows += (size_t)local * m;
      if (m == 1 && !bottom) break;
      m = (m + 1) / 2;
      bottom = false;
    }
    bits.assign((size_t)((total() + 63) / 64), 0);
    known.assign((rows + 63) / 64, 0);
    keeps_nodes = false;
    n_present = 0;
    finished = false;
  }
  size_t depth() const { return csizes.size() - 1; }     // siblings of a block's path: block_proof_depth(n_blocks)
  uint64_t total() const { return n_local * n_blocks; }
  uint64_t n_missing() const { return total() - n_present; }
  bool present(uint64_t local, uint64_t block) const {
    const uint64_t g = local * n_blocks + block;
    return (bits[(size_t)(g >> 6)] >> (g & 63)) & 1;
  }
  // the row of layer 0 that keeps the root of `block` of dataset slot `slot` (the row repair compares with in a compact dataset)
  uint64_t dest_row(uint64_t slot, uint64_t block) const { return repair_row_compact(coff[0], csizes[0], slot - first_slot, block); }

  // ---- validation ----------------------------------------------------------------------------------------------------------------
  // Requests are (dataset slot, block) pairs.  A finished session takes none; every slot inside the local range, every block below
  // n_blocks; the same pair twice is allowed (two peers may answer).  false with *err naming the lowest request index that breaks a rule.
  bool validate(const uint64_t* slot_block, size_t n, std::string* err) const {
    if (finished) {
      *err = "fill: the session is finished: it accepts only cp2_fill_free";
      return false;
    }
    for (size_t i = 0; i < n; ++i)
      if (!validate_pair(i, slot_block[2 * i], slot_block[2 * i + 1], err)) return false;
    return true;
  }
  bool validate_pair(size_t i, uint64_t s, uint64_t b, std::string* err) const {
    if (s < first_slot || s - first_slot >= n_local) {
      *err = "fill: request " + std::to_string(i) + ": slot " + std::to_string(s) + " is not inside the local range " +
             std::to_string(first_slot) + " + " + std::to_string(n_local);
      return false;
    }
    if (b >= n_blocks) {
      *err = "fill: request " + std::to_string(i) + ": block " + std::to_string(b) + " of slot " + std::to_string(s) + " is not below nBlocks = " +
             std::to_string(n_blocks);
      return false;
    }
    return true;
  }

  // ---- what the device reads -------------------------------------------------------------------------------------------------------
  // per request the (local slot, block) pair the walk indexes the slot roots and starts from, and the destination row
  void device_requests(const uint64_t* slot_block, size_t n, std::vector<uint64_t>* local_block, std::vector<uint64_t>* dest) const {
    local_block->resize(2 * n);
    dest->resize(n);
    for (size_t i = 0; i < n; ++i) {
      (*local_block)[2 * i] = slot_block[2 * i] - first_slot;
      (*local_block)[2 * i + 1] = slot_block[2 * i + 1];
      (*dest)[i] = dest_row(slot_block[2 * i], slot_block[2 * i + 1]);
    }
  }

  // ---- NEW / DUPLICATE ---------------------------------------------------------------------------------------------------------------
  // verdict[i] == 0: the device proved request i.  A proved block that is present already, or that a LOWER proved index of this call
  // names, is a DUPLICATE; the first is NEW.  Changes nothing of the session.
  void resolve(const uint64_t* slot_block, const uint32_t* verdict, size_t n, uint32_t* status) const {
    std::vector<size_t> proved;
    for (size_t i = 0; i < n; ++i) {
      status[i] = FILL_MISMATCH;
      if (verdict[i] == 0) proved.push_back(i);
    }
    // by (slot, block), the lowest index first: repair's write order, whose groups put equal pairs side by side
    for (const WriteGroup& g : repair_write_groups(slot_block, proved)) {
      std::vector<size_t> reqs(g.reqs);
      std::stable_sort(reqs.begin(), reqs.end(), [&](size_t a, size_t b) {
        if (slot_block[2 * a + 1] != slot_block[2 * b + 1]) return slot_block[2 * a + 1] < slot_block[2 * b + 1];
        return a < b;
      });
      for (size_t k = 0; k < reqs.size(); ++k) {
        const size_t i = reqs[k];
        const bool again = k > 0 && slot_block[2 * reqs[k - 1] + 1] == slot_block[2 * i + 1];
        status[i] = again || present(g.slot - first_slot, slot_block[2 * i + 1]) ? FILL_DUPLICATE : FILL_NEW;
      }
    }
  }

  // ---- writing -------------------------------------------------------------------------------------------------------------------
  // what the writer is handed: the NEW blocks to write, everything else to skip
  static std::vector<uint32_t> write_mask(const uint32_t* status, size_t n) {
    std::vector<uint32_t> w(n);
    for (size_t i = 0; i < n; ++i) w[i] = status[i] == FILL_NEW ? FILL_WRITE : FILL_SKIP;
    return w;
  }
  // ... and the roll-back: a NEW block whose file failed (or came after the failing one) is UNWRITTEN and stays missing, and so is every
  // DUPLICATE of it in this call: "already present" would be untrue of a block that is still missing
  static void roll_back(const uint64_t* slot_block, const std::vector<uint32_t>& written, uint32_t* status) {
    std::vector<size_t> failed;
    for (size_t i = 0; i < written.size(); ++i)
      if (status[i] == FILL_NEW && written[i] == FILL_WRITE_FAILED) {
        status[i] = FILL_UNWRITTEN;
        failed.push_back(i);
      }
    if (failed.empty()) return;
    for (size_t i = 0; i < written.size(); ++i) {
      if (status[i] != FILL_DUPLICATE) continue;
      for (size_t k : failed)
        if (slot_block[2 * k] == slot_block[2 * i] && slot_block[2 * k + 1] == slot_block[2 * i + 1]) { status[i] = FILL_UNWRITTEN; break; }
    }
  }
  // the presence bits of the blocks that are still NEW (after the files were synced; at once for the fake source): returns how many
  size_t commit(const uint64_t* slot_block, const uint32_t* status, size_t n) {
    size_t set = 0;
    for (size_t i = 0; i < n; ++i) {
      if (status[i] != FILL_NEW) continue;
      const uint64_t g = (slot_block[2 * i] - first_slot) * n_blocks + slot_block[2 * i + 1];
      uint64_t& w = bits[(size_t)(g >> 6)];
      if (!((w >> (g & 63)) & 1)) {
        w |= 1ULL << (g & 63);
        ++set;
      }
    }
    n_present += set;
    return set;
  }
  // ... and its reverse (cp2_fill_resume): the presence bits of blocks the disk no longer backs, as global indices local * n_blocks + block;
  // returns how many were set.  A dropped block is missing like one that never arrived.
  size_t drop(const uint64_t* global, size_t n) {
    size_t cleared = 0;
    for (size_t i = 0; i < n; ++i) {
      if (global[i] >= total()) continue;
      uint64_t& w = bits[(size_t)(global[i] >> 6)];
      if ((w >> (global[i] & 63)) & 1) {
        w &= ~(1ULL << (global[i] & 63));
        ++cleared;
      }
    }
    n_present -= cleared;
    return cleared;
  }
  // ... and commit by global index (cp2_fill_adopt, adopt_plan.hpp): the presence bits of blocks whose bytes the disk already holds and the
  // device has proved; returns how many were clear
  size_t set_present(const uint64_t* global, size_t n) {
    size_t set = 0;
    for (size_t i = 0; i < n; ++i) {
      if (global[i] >= total()) continue;
      uint64_t& w = bits[(size_t)(global[i] >> 6)];
      if (!((w >> (global[i] & 63)) & 1)) {
        w |= 1ULL << (global[i] & 63);
        ++set;
      }
    }
    n_present += set;
    return set;
  }
  // a saved bitmap taken over (cp2_fill_resume): false when it is not a bitmap of this session (its size, or a bit past the last block)
  bool restore(const std::vector<uint64_t>& saved) {
    if (saved.size() != bits.size()) return false;
    if ((total() & 63) && (saved.back() >> (total() & 63))) return false;
    bits = saved;
    n_present = 0;
    for (uint64_t w : bits) n_present += (uint64_t)__builtin_popcountll(w);
    return true;
  }

  // ---- the nodes a serving session keeps ---------------------------------------------------------------------------------------------
  // the row of node `index` of layer `level` of local slot `local`: what k_block_path_commit_nodes computes from its two device tables
  // (layer_off = coff, layer_size = csizes), and block_proof_sibling_row's row for an in-range sibling
  uint64_t node_row(size_t level, uint64_t local, uint64_t index) const { return coff[level] + local * csizes[level] + index; }
  bool is_known(uint64_t row) const { return (known[(size_t)(row >> 6)] >> (row & 63)) & 1; }
  void set_known(uint64_t row) { known[(size_t)(row >> 6)] |= 1ULL << (row & 63); }
  // The rows the kernel stored for the requests it proved (verdict[i] == 0): the block root, and per level the sibling (unless its index
  // lies past its layer: the zero of an odd layer's last node or of the one-block slot, which has no row) and the ancestor.  Whether the
  // block was then written does not matter: an UNWRITTEN block is still missing, but its nodes are authentic and stored.
  void mark_proved(const uint64_t* slot_block, const uint32_t* verdict, size_t n) {
    for (size_t i = 0; i < n; ++i) {
      if (verdict[i] != 0) continue;
      const uint64_t local = slot_block[2 * i] - first_slot, b = slot_block[2 * i + 1];
      set_known(node_row(0, local, b));
      for (size_t l = 0; l < depth(); ++l) {
        const uint64_t sib = (b >> l) ^ 1;
        if (sib < csizes[l]) set_known(node_row(l, local, sib));
        set_known(node_row(l + 1, local, b >> (l + 1)));
      }
    }
  }
  // The same bits for groups proved by multiproofs (cp2_fill_add_multi): the rows k_multiproof_commit stored are the rows of the call's
  // work table -- leaves, sent rows and computed nodes, row r being node row_index[r] of layer row_level[r] of the tree of local slot
  // group_local[row_group[r]] (multiproof_plan.hpp) -- of every group whose verdict is 0.  For a group of blocks that is the union of
  // what mark_proved sets for each of them: a sibling on some block's path is a leaf, a sent row or another block's ancestor.
  void mark_proved_multi(const uint32_t* row_group, const uint32_t* row_level, const uint64_t* row_index, size_t n_work, const uint64_t* group_local,
                         const uint32_t* group_verdict) {
    for (size_t r = 0; r < n_work; ++r)
      if (group_verdict[row_group[r]] == 0) set_known(node_row(row_level[r], group_local[row_group[r]], row_index[r]));
  }
  // What a session knows when node keeping is turned on, after every upper layer was built once from layer 0 (absent rows zeroed): a
  // block root is known where the block is present, and a parent where both children are; the last node of an odd layer (and the
  // singleton) has one child.  Parents of unknown children hold values nobody reads: their bits stay clear until a proved path stores them.
  void derive_from_presence() {
    std::fill(known.begin(), known.end(), 0);
    for (uint64_t s = 0; s < n_local; ++s)
      for (uint64_t b = 0; b < n_blocks; ++b)
        if (present(s, b)) set_known(node_row(0, s, b));
    for (size_t l = 0; l < depth(); ++l)
      for (uint64_t s = 0; s < n_local; ++s)
        for (uint64_t k = 0; k < csizes[l + 1]; ++k) {
          const bool left = is_known(node_row(l, s, 2 * k));
          const bool right = 2 * k + 1 < csizes[l] ? is_known(node_row(l, s, 2 * k + 1)) : true;
          if (left && right) set_known(node_row(l + 1, s, k));
        }
  }
  // can the proof of (local, block) be served: the block present, and every sibling of its path that has a row (block_proof_rows) known
  bool servable(uint64_t local, uint64_t block) const {
    if (!present(local, block)) return false;
    for (size_t l = 0; l < depth(); ++l) {
      const uint64_t r = block_proof_sibling_row(coff[l], csizes[l], local, block, l);
      if (r != BLOCK_PROOF_NO_ROW && !is_known(r)) return false;
    }
    return true;
  }
  uint32_t proof_status(uint64_t local, uint64_t block) const {
    return !present(local, block) ? FILL_PROOF_ABSENT : servable(local, block) ? FILL_PROOF_OK : FILL_PROOF_PARTIAL;
  }

  // ---- paths that stop at a node the session holds (cp2_fill_anchors, cp2_fill_add_anchored) -------------------------------------------
  // A computed node that equals an authentic node proves everything below it, by the collision argument the whole walk rests on: so a
  // block whose ancestor at level a is known needs its a lowest siblings only.  Level depth() is the stated slot root, which a session
  // holds from the start whether or not the top row's bit is set.
  // the lowest level whose node on the block's way up is known; depth() throughout for a session that keeps no nodes
  size_t anchor_level(uint64_t local, uint64_t block) const {
    if (!keeps_nodes) return depth();
    for (size_t l = 0; l < depth(); ++l)
      if (is_known(node_row(l, local, block >> l))) return l;
    return depth();
  }
  // validate's rules, a session that keeps nodes, and per request a level of at most depth() whose node is known NOW (a node another
  // request of the same call would prove does not count: the device reads every anchor before any request of the call is judged) or
  // that is depth() itself.  Any known level may be stated, not only the lowest.  false with *err naming the lowest offending index.
  bool validate_anchored(const uint64_t* slot_block, const uint32_t* levels, size_t n, std::string* err) const {
    if (finished) {
      *err = "fill: the session is finished: it accepts only cp2_fill_free";
      return false;
    }
    if (!keeps_nodes) {
      *err = "fill: this session does not keep the nodes of the paths it proves: call cp2_fill_keep_nodes first";
      return false;
    }
    for (size_t i = 0; i < n; ++i) {
      const uint64_t s = slot_block[2 * i], b = slot_block[2 * i + 1];
      if (!validate_pair(i, s, b, err)) return false;
      const size_t a = levels[i];
      if (a > depth()) {
        *err = "fill: request " + std::to_string(i) + ": level " + std::to_string(a) + " is above the depth " + std::to_string(depth());
        return false;
      }
      if (a < depth() && !is_known(node_row(a, s - first_slot, b >> a))) {
        *err = "fill: request " + std::to_string(i) + ": the node at level " + std::to_string(a) + " above block " + std::to_string(b) +
               " of slot " + std::to_string(s) + " is not known to the session";
        return false;
      }
    }
    return true;
  }
  static constexpr uint64_t ANCHOR_SLOT_ROOT = UINT64_MAX;   // anchor_row: compare with the stated slot root instead of a row
  // device_requests, and per request where its siblings start in the packed path buffer (path_off: n + 1 entries, rows; the last is the
  // sum of all levels) and the row its walk must arrive at
  void device_requests_anchored(const uint64_t* slot_block, const uint32_t* levels, size_t n, std::vector<uint64_t>* local_block,
                                std::vector<uint64_t>* dest, std::vector<uint64_t>* path_off, std::vector<uint64_t>* anchor_row) const {
    device_requests(slot_block, n, local_block, dest);
    path_off->resize(n + 1);
    anchor_row->resize(n);
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) {
      const size_t a = levels[i];
      (*path_off)[i] = at;
      at += a;
      (*anchor_row)[i] = a >= depth() ? ANCHOR_SLOT_ROOT : node_row(a, slot_block[2 * i] - first_slot, slot_block[2 * i + 1] >> a);
    }
    (*path_off)[n] = at;
  }
  // The rows the kernel stored for the anchored requests it proved: the block root, the in-range siblings below the level and the
  // ancestors strictly between; the anchor and everything above it were known already (or are not this request's to vouch for).
  void mark_proved_anchored(const uint64_t* slot_block, const uint32_t* levels, const uint32_t* verdict, size_t n) {
    for (size_t i = 0; i < n; ++i) {
      if (verdict[i] != 0) continue;
      const uint64_t local = slot_block[2 * i] - first_slot, b = slot_block[2 * i + 1];
      const size_t a = std::min<size_t>(levels[i], depth());
      if (a > 0) set_known(node_row(0, local, b));     // (at level 0 the block root is the anchor)
      for (size_t l = 0; l < a; ++l) {
        const uint64_t sib = (b >> l) ^ 1;
        if (sib < csizes[l]) set_known(node_row(l, local, sib));
        if (l + 1 < a) set_known(node_row(l + 1, local, b >> (l + 1)));
      }
    }
  }

  // ---- what is missing ----------------------------------------------------------------------------------------------------------------
  // the lowest min(cap, n_missing) absent (dataset slot, block) pairs in ascending order into `out` (may be NULL when cap == 0); returns
  // the number of all absent blocks
  uint64_t missing(uint64_t* out, size_t cap) const {
    size_t k = 0;
    const uint64_t all = total();
    for (size_t w = 0; k < cap && w < bits.size(); ++w) {
      uint64_t absent = ~bits[w];
      while (absent && k < cap) {
        const uint64_t g = (uint64_t)w * 64 + (uint64_t)__builtin_ctzll(absent);
        absent &= absent - 1;
        if (g >= all) break;
        out[2 * k] = first_slot + g / n_blocks;
        out[2 * k + 1] = g % n_blocks;
        ++k;
      }
    }
    return n_missing();
  }

  // ---- finishing -----------------------------------------------------------------------------------------------------------------------
  // every block present and the session not finished yet; else false with *err naming the count and the first missing pair
  bool may_finish(std::string* err) const {
    if (finished) {
      *err = "fill: the session is finished: it accepts only cp2_fill_free";
      return false;
    }
    if (n_missing()) {
      uint64_t first[2] = {0, 0};
      (void)missing(first, 1);
      *err = "fill: " + std::to_string(n_missing()) + " block(s) are missing, the first is (slot " + std::to_string(first[0]) + ", block " +
             std::to_string(first[1]) + ")";
      return false;
    }
    return true;
  }
};

}  // namespace cp2i
