// The host side of a fill session's checkpoint WITH its kept nodes (csrc/fill.cpp: cp2_fill_save_nodes / cp2_fill_resume_nodes): the file
// layout, writing and parsing it with every size bounded before anything is allocated, which saved rows a resumed session has to have
// authenticated (the candidates), the flag byte per row that travels to the device, a host model of what k_nodes_restore_layer makes of
// those bytes, and how the bytes that come back become known bits and the three counts.  No HIP in here:
// tests/host_check/node_ckpt_check.cpp walks it over random geometries and known sets on the CPU, under AddressSanitizer + UBSan.
//
// The file, every integer a little-endian 64-bit word:
//   offset 0    "CP2FILL2"
//   then        the ten words, the file base name, the stated slot roots and the presence bitmap of CP2FILL1 (fill_checkpoint.hpp), each
//               where and what it is there
//   then        the known bitmap: ceil(rows / 64) words, bit r = row r of the compact layout (FillPlan::node_row); bits past the last row 0
//   then        layer 0 of the compact buffer: n_local x n_blocks rows of 32 bytes; a row is 0 unless its block is present or its row known
//   then        the known rows of the layers strictly between layer 0 and the top, 32 bytes each, packed in ascending row order
//   then        one word: Checksum64 over every byte before it
// The top rows are not stored: their bits are, and their value is the stated root the header holds.
//
// The rule of a resume.  Nothing the file says about a node is believed.  D is what presence gives the resumed session (FillPlan::
// derive_from_presence after the re-check); the candidates C are the file's known rows below the top that are not in D, with the values
// the file states.  Top-down, layer by layer, a parent that is known (in D, restored, or a top row: the stated slot root) and whose
// children are all known or candidates, at least one a candidate, is recomputed from them: where the result equals the parent's value the
// candidate children are authentic by the collision argument every walk rests on, and are RESTORED; where it differs they are REJECTED.  A
// candidate whose parent is not known in the resumed session, or whose sibling is undefined, is reached by no parent: it stays unproved.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "fill_checkpoint.hpp"
#include "fill_plan.hpp"

namespace cp2i {

// the states of a flag byte: the values of cp2k::NODE_* (kernels.hpp); a row is in one of them or in none (0: undefined)
constexpr uint8_t NODE_F_KNOWN = 1, NODE_F_CAND = 2, NODE_F_RESTORED = 4, NODE_F_REJECTED = 8;

// what a CP2FILL2 file holds beside a CP2FILL1's fields
struct NodeCheckpoint {
  FillCheckpoint base;                     // meta, presence bitmap, layer 0 (as the file states it: known rows of absent blocks included)
  std::vector<uint64_t> known;             // the known bitmap over the rows of the compact layout
  std::vector<uint8_t> mid;                // the packed known rows of the layers between layer 0 and the top
};

// where the parts of a CP2FILL2 file lie; `size` needs the number of packed rows
struct NodeCkptLayout {
  FillCkptLayout base;                     // roots_at, bits_at as in CP2FILL1; layer0_at / sum_at / size of base are NOT this file's
  uint64_t rows = 0, mid_begin = 0, mid_end = 0, known_words = 0;   // rows of all layers; the rows of the middle layers are [mid_begin, mid_end)
  size_t known_at = 0, layer0_at = 0, mid_at = 0;
  size_t size_for(uint64_t n_mid) const { return mid_at + (size_t)n_mid * 32 + 8; }
};

// the layout for (base_len, n_local, n_blocks); false when the counts are out of CP2FILL1's bounds.  rows < 2 x total + 64 x n_local.
inline bool node_ckpt_layout(uint64_t base_len, uint64_t n_local, uint64_t n_blocks, NodeCkptLayout* l) {
  if (!fill_ckpt_layout(base_len, n_local, n_blocks, &l->base)) return false;
  uint64_t rows = 0, first_upper = 0, top = 0;
  bool bottom = true;
  for (uint64_t m = n_blocks;;) {           // FillPlan::init's layers
    if (!bottom && first_upper == 0) first_upper = rows;
    top = rows;
    rows += n_local * m;
    if (m == 1 && !bottom) break;
    m = (m + 1) / 2;
    bottom = false;
  }
  l->rows = rows;
  l->mid_begin = first_upper;               // == total
  l->mid_end = top;                         // depth 1: mid_begin == mid_end, no middle layer
  l->known_words = (rows + 63) / 64;
  l->known_at = l->base.layer0_at;          // where CP2FILL1 has layer 0, the known bitmap comes first
  l->layer0_at = l->known_at + (size_t)l->known_words * 8;
  l->mid_at = l->layer0_at + (size_t)l->base.total * 32;
  return true;
}

inline bool node_ckpt_bit(const std::vector<uint64_t>& bits, uint64_t r) { return (bits[(size_t)(r >> 6)] >> (r & 63)) & 1; }
inline uint64_t node_ckpt_count(const std::vector<uint64_t>& bits, uint64_t from, uint64_t to) {
  uint64_t n = 0;
  for (uint64_t r = from; r < to; ++r) n += node_ckpt_bit(bits, r);
  return n;
}

// ---- writing ----------------------------------------------------------------------------------------------------------------------------
// The whole file from the session's plan and a host image of its compact buffer (`rows` x 32 bytes; rows that are neither present nor
// known may hold anything: they are written as zeros or left out).  false: the session is out of the layout's bounds, or the plan keeps no
// shape the image has.
inline bool node_ckpt_serialise(const FillCkptMeta& m, const FillPlan& p, const uint8_t* image, std::vector<uint8_t>* buf) {
  NodeCkptLayout l;
  if (m.cell_size == 0 || m.block_size < m.cell_size || !node_ckpt_layout(m.file_base.size(), m.n_local, m.n_blocks(), &l)) return false;
  if (p.bits.size() != l.base.words || p.known.size() != l.known_words || p.rows != l.rows || m.roots.size() != m.n_local * 32) return false;
  const uint64_t n_mid = node_ckpt_count(p.known, l.mid_begin, l.mid_end);
  buf->assign(l.size_for(n_mid), 0);
  uint8_t* out = buf->data();
  std::memcpy(out, "CP2FILL2", 8);
  const uint64_t w[10] = {m.cell_size, m.block_size, m.n_cells, m.n_slots, m.first_slot, m.n_local, m.src, m.seed, m.file_base.size(), l.base.n_blocks};
  for (int i = 0; i < 10; ++i) fill_ckpt_put(out + 8 + 8 * i, w[i]);
  if (!m.file_base.empty()) std::memcpy(out + FILL_CKPT_FIXED, m.file_base.data(), m.file_base.size());
  std::memcpy(out + l.base.roots_at, m.roots.data(), m.roots.size());
  std::memcpy(out + l.base.bits_at, p.bits.data(), (size_t)l.base.words * 8);
  std::memcpy(out + l.known_at, p.known.data(), (size_t)l.known_words * 8);
  for (uint64_t g = 0; g < l.base.total; ++g)
    if (node_ckpt_bit(p.bits, g) || node_ckpt_bit(p.known, g)) std::memcpy(out + l.layer0_at + (size_t)g * 32, image + (size_t)g * 32, 32);
  size_t at = l.mid_at;
  for (uint64_t r = l.mid_begin; r < l.mid_end; ++r)
    if (node_ckpt_bit(p.known, r)) {
      std::memcpy(out + at, image + (size_t)r * 32, 32);
      at += 32;
    }
  Checksum64 sum;
  sum.update(out, at);
  fill_ckpt_put(out + at, sum.finish());
  return true;
}

// ---- reading ----------------------------------------------------------------------------------------------------------------------------
// The layout the first FILL_CKPT_FIXED bytes announce (CP2FILL1's rules for the ten words) and the sizes a file of that header can have:
// a reader compares them with the file's length before it allocates.  false with *err saying what is wrong.
inline bool node_ckpt_fixed(const uint8_t* p, size_t n, FillCkptMeta* m, NodeCkptLayout* l, std::string* err) {
  if (n < FILL_CKPT_FIXED + 8) { *err = "is truncated: shorter than a checkpoint's header"; return false; }
  if (std::memcmp(p, "CP2FILL2", 8) != 0) { *err = "is not a fill checkpoint with nodes of this version (magic)"; return false; }
  uint8_t as1[FILL_CKPT_FIXED];
  std::memcpy(as1, p, FILL_CKPT_FIXED);
  std::memcpy(as1, "CP2FILL1", 8);            // the ten words are CP2FILL1's: its rules judge them
  FillCkptLayout b;
  if (!fill_ckpt_fixed(as1, n, m, &b, err)) return false;
  if (!node_ckpt_layout(b.base_len, b.n_local, b.n_blocks, l)) { *err = "is corrupt: its header states sizes no session has"; return false; }
  return true;
}
// is `n` a length a file of this header can have: the fixed parts, a whole number of packed rows, no more of them than there are middle rows
inline bool node_ckpt_size_ok(const NodeCkptLayout& l, size_t n, std::string* err) {
  const size_t least = l.size_for(0);
  if (n < least) { *err = "is truncated: " + std::to_string(n) + " bytes of at least " + std::to_string(least); return false; }
  if ((n - least) % 32 != 0 || (n - least) / 32 > l.mid_end - l.mid_begin) {
    *err = "is corrupt: " + std::to_string(n) + " bytes is no size its header allows";
    return false;
  }
  return true;
}
// the whole file: sizes, checksum, padding, the two bitmaps, the packed count, then (and only then) the copies
inline bool node_ckpt_parse(const uint8_t* p, size_t n, NodeCheckpoint* c, std::string* err) {
  NodeCkptLayout l;
  FillCkptMeta m;
  if (!node_ckpt_fixed(p, n, &m, &l, err) || !node_ckpt_size_ok(l, n, err)) return false;
  const size_t sum_at = n - 8;
  Checksum64 sum;
  sum.update(p, sum_at);
  if (sum.finish() != fill_ckpt_word(p + sum_at)) { *err = "is corrupt (checksum)"; return false; }
  for (size_t i = FILL_CKPT_FIXED + (size_t)l.base.base_len; i < l.base.roots_at; ++i)
    if (p[i]) { *err = "is corrupt: bytes after the file base name"; return false; }
  if ((l.base.total & 63) && (fill_ckpt_word(p + l.base.bits_at + (l.base.words - 1) * 8) >> (l.base.total & 63))) {
    *err = "is corrupt: presence bits past the last block";
    return false;
  }
  if ((l.rows & 63) && (fill_ckpt_word(p + l.known_at + (l.known_words - 1) * 8) >> (l.rows & 63))) {
    *err = "is corrupt: known bits past the last row";
    return false;
  }
  std::vector<uint64_t> known((size_t)l.known_words);
  std::memcpy(known.data(), p + l.known_at, (size_t)l.known_words * 8);
  const uint64_t n_mid = node_ckpt_count(known, l.mid_begin, l.mid_end);
  if (l.size_for(n_mid) != n) {
    *err = "is corrupt: " + std::to_string((n - l.size_for(0)) / 32) + " packed row(s) where its known bitmap states " + std::to_string(n_mid);
    return false;
  }
  m.file_base.assign(reinterpret_cast<const char*>(p) + FILL_CKPT_FIXED, (size_t)l.base.base_len);
  m.roots.assign(p + l.base.roots_at, p + l.base.bits_at);
  c->base.meta = std::move(m);
  c->base.bits.resize((size_t)l.base.words);
  std::memcpy(c->base.bits.data(), p + l.base.bits_at, (size_t)l.base.words * 8);
  c->base.layer0.assign(p + l.layer0_at, p + l.mid_at);
  c->known = std::move(known);
  c->mid.assign(p + l.mid_at, p + sum_at);
  return true;
}

// ---- the candidates ---------------------------------------------------------------------------------------------------------------------
// What travels to the device for a plan that holds D (derive_from_presence on what survived the re-check) and the file's known bitmap:
// the flag byte per row, and the candidate values where they lie in the compact layout (rows x 32 bytes, zeros where there is none).
struct NodeRestorePlan {
  std::vector<uint8_t> flags;              // rows: NODE_F_KNOWN on D and on every top row, NODE_F_CAND on saved \ D below the top, else 0
  std::vector<uint8_t> cand;               // rows x 32
  uint64_t n_cand = 0;
};
// false when `saved` / `layer0` / `mid` are not those of a checkpoint of this plan's shape (node_ckpt_parse has made sure they are)
inline bool node_restore_plan(const FillPlan& p, const std::vector<uint64_t>& saved, const std::vector<uint8_t>& layer0,
                              const std::vector<uint8_t>& mid, NodeRestorePlan* out) {
  const uint64_t top = p.coff[p.depth()], total = p.total();
  if (saved.size() != p.known.size() || layer0.size() != total * 32) return false;
  if (mid.size() != node_ckpt_count(saved, total, top) * 32) return false;
  out->flags.assign(p.rows, 0);
  out->cand.assign(p.rows * 32, 0);
  out->n_cand = 0;
  size_t at = 0;
  for (uint64_t r = 0; r < top; ++r) {
    const bool k = node_ckpt_bit(saved, r);
    const uint8_t* v = r < total ? &layer0[(size_t)r * 32] : k ? &mid[at] : nullptr;
    if (r >= total && k) at += 32;
    if (p.is_known(r)) out->flags[(size_t)r] = NODE_F_KNOWN;
    else if (k) {
      out->flags[(size_t)r] = NODE_F_CAND;
      std::memcpy(&out->cand[(size_t)r * 32], v, 32);
      ++out->n_cand;
    }
  }
  for (uint64_t r = top; r < p.rows; ++r) out->flags[(size_t)r] = NODE_F_KNOWN;
  return true;
}

// ---- the model of the kernel ------------------------------------------------------------------------------------------------------------
// k_nodes_restore_layer over every layer, top first: `tree` and `cand` hold one value per row, `roots` one per local slot;
// compress(left, right, key) with key = (layer 0 ? 1 : 0) + (single child ? 2 : 0) and `zero` for the missing sibling.  Writes rows of
// `tree` and bytes of `flags` of candidate children, nothing else.
template <class V, class Compress>
void node_restore_model(const FillPlan& p, std::vector<V>* tree, const std::vector<V>& cand, const std::vector<V>& roots, const V& zero,
                        std::vector<uint8_t>* flags, Compress compress) {
  for (size_t l = p.depth(); l-- > 0;)
    for (uint64_t s = 0; s < p.n_local; ++s)
      for (uint64_t j = 0; j < p.csizes[l + 1]; ++j) {
        const uint64_t rl = p.node_row(l, s, 2 * j), rp = p.node_row(l + 1, s, j);
        const bool pair = 2 * j + 1 < p.csizes[l];
        if (!((*flags)[(size_t)rp] & (NODE_F_KNOWN | NODE_F_RESTORED))) continue;
        const uint8_t fl = (*flags)[(size_t)rl], fr = pair ? (*flags)[(size_t)rl + 1] : NODE_F_KNOWN;
        if (!(fl & (NODE_F_KNOWN | NODE_F_CAND)) || !(fr & (NODE_F_KNOWN | NODE_F_CAND)) || !((fl | fr) & NODE_F_CAND)) continue;
        const V& left = (fl & NODE_F_KNOWN) ? (*tree)[(size_t)rl] : cand[(size_t)rl];
        const V& right = !pair ? zero : (fr & NODE_F_KNOWN) ? (*tree)[(size_t)rl + 1] : cand[(size_t)rl + 1];
        const V v = compress(left, right, (uint32_t)((l == 0 ? 1 : 0) + (pair ? 0 : 2)));
        const bool ok = v == (l + 1 == p.depth() ? roots[(size_t)s] : (*tree)[(size_t)rp]);
        for (uint64_t r = rl; r <= rl + (pair ? 1 : 0); ++r) {
          if (!((*flags)[(size_t)r] & NODE_F_CAND)) continue;
          if (ok) (*tree)[(size_t)r] = cand[(size_t)r];
          (*flags)[(size_t)r] = ok ? NODE_F_RESTORED : NODE_F_REJECTED;
        }
      }
}

// ---- what comes back ---------------------------------------------------------------------------------------------------------------------
struct NodeRestoreCounts {
  uint64_t restored = 0, rejected = 0, unproved = 0;
};
// The restored rows become known; a top row's bit is taken over as saved.  `up` are the bytes sent, `down` the bytes that came back: a
// byte that claims what the bytes sent up rule out -- a restored or rejected row that was no candidate -- is ignored.
inline NodeRestoreCounts node_restore_apply(FillPlan* p, const std::vector<uint64_t>& saved, const std::vector<uint8_t>& up,
                                            const std::vector<uint8_t>& down) {
  NodeRestoreCounts c;
  const uint64_t top = p->coff[p->depth()];
  for (uint64_t r = 0; r < top; ++r) {
    if (up[(size_t)r] != NODE_F_CAND) continue;
    const uint8_t f = down[(size_t)r];
    if (f == NODE_F_RESTORED) {
      p->set_known(r);
      ++c.restored;
    } else if (f == NODE_F_REJECTED) ++c.rejected;
    else ++c.unproved;
  }
  for (uint64_t r = top; r < p->rows; ++r)
    if (node_ckpt_bit(saved, r)) p->set_known(r);
  return c;
}

}  // namespace cp2i
