// The host side of a fill session's checkpoint (csrc/fill.cpp: cp2_fill_save / cp2_fill_resume): the file layout, writing and parsing it
// with every size checked before anything is allocated, whether a checkpoint describes the session that is being resumed (and the first
// field that does not), which blocks a slot file is too short to back, the plan of the re-check's reads, and the two readers the re-check
// and cp2_fill_adopt share: how many whole blocks each slot file holds, and a chunk of the plan read into a host buffer.  No HIP in here:
// tests/host_check/fill_checkpoint_check.cpp walks it on the CPU and against real files, under AddressSanitizer + UBSan.
//
// The file, every integer a little-endian 64-bit word:
//   offset 0    "CP2FILL1"
//   offset 8    ten words: cell_size, block_size, n_cells, n_slots, first_slot, n_local, source (0 fake, 1 slot files), seed,
//               file_base_len, n_blocks (= n_cells / (block_size / cell_size), stated so that a reader need not derive it)
//   offset 88   the file base name, file_base_len bytes (0 for the fake source), zero-padded to a multiple of 8
//   then        the stated slot roots, canonical: n_local x 32 bytes
//   then        the presence bitmap: ceil(n_local x n_blocks / 64) words, bit (local x n_blocks + block); the bits past the last block are 0
//   then        layer 0 of the compact buffer: n_local x n_blocks rows of 32 bytes, row (local x n_blocks + block); rows of absent blocks are 0
//   then        one word: Checksum64 (checksum64.hpp, the checksum of the kept form) over every byte before it
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "checksum64.hpp"
#include "fill_pipeline.hpp"   // fill_slot_file_name and the slot-file read rule: slot_file_read_rest, slot_file_error

namespace cp2i {

constexpr uint64_t FILL_SRC_FAKE = 0, FILL_SRC_FILE = 1;
constexpr size_t FILL_CKPT_FIXED = 8 + 10 * 8;            // magic and the ten words
constexpr uint64_t FILL_CKPT_MAX_BASE = 4096;             // as the tree cache and the kept form bound their base names
constexpr uint64_t FILL_CKPT_MAX_BLOCKS = 1ULL << 40;     // n_local x n_blocks: 32 TiB of layer 0, far beyond any HBM

// what a checkpoint says about its session, and what a resume states about the session it wants
struct FillCkptMeta {
  uint64_t cell_size = 0, block_size = 0, n_cells = 0, n_slots = 0, first_slot = 0, n_local = 0, src = FILL_SRC_FAKE, seed = 0;
  std::string file_base;
  std::vector<uint8_t> roots;                              // n_local x 32, canonical
  uint64_t n_blocks() const { return n_cells / (block_size / cell_size); }
  uint64_t total() const { return n_local * n_blocks(); }
};

struct FillCheckpoint {
  FillCkptMeta meta;
  std::vector<uint64_t> bits;                              // the presence bitmap
  std::vector<uint8_t> layer0;                             // total x 32
};

// where the parts of a checkpoint lie
struct FillCkptLayout {
  uint64_t base_len = 0, n_local = 0, n_blocks = 0, total = 0, words = 0;
  size_t roots_at = 0, bits_at = 0, layer0_at = 0, sum_at = 0, size = 0;
};

inline uint64_t fill_ckpt_word(const uint8_t* p) { uint64_t v; std::memcpy(&v, p, 8); return v; }
inline void fill_ckpt_put(uint8_t* p, uint64_t v) { std::memcpy(p, &v, 8); }

// the layout for (base_len, n_local, n_blocks); false when the counts are out of bounds (no product wraps: every factor is bounded first)
inline bool fill_ckpt_layout(uint64_t base_len, uint64_t n_local, uint64_t n_blocks, FillCkptLayout* l) {
  if (base_len > FILL_CKPT_MAX_BASE || n_local == 0 || n_blocks == 0 || n_local > FILL_CKPT_MAX_BLOCKS || n_blocks > FILL_CKPT_MAX_BLOCKS) return false;
  const unsigned __int128 total = (unsigned __int128)n_local * n_blocks;
  if (total > FILL_CKPT_MAX_BLOCKS) return false;
  l->base_len = base_len; l->n_local = n_local; l->n_blocks = n_blocks;
  l->total = (uint64_t)total;
  l->words = (l->total + 63) / 64;
  l->roots_at = FILL_CKPT_FIXED + (size_t)((base_len + 7) / 8 * 8);
  l->bits_at = l->roots_at + (size_t)n_local * 32;
  l->layer0_at = l->bits_at + (size_t)l->words * 8;
  l->sum_at = l->layer0_at + (size_t)l->total * 32;
  l->size = l->sum_at + 8;
  return true;
}

// ---- writing ----------------------------------------------------------------------------------------------------------------------------
// A buffer of the checkpoint's size with everything but layer 0 and the checksum in place; the caller puts the rows of layer 0 at
// buf + l->layer0_at (one download) and seals it.  false: the session is out of the layout's bounds.
inline bool fill_ckpt_begin(const FillCkptMeta& m, const std::vector<uint64_t>& bits, std::vector<uint8_t>* buf, FillCkptLayout* l) {
  if (m.cell_size == 0 || m.block_size < m.cell_size || !fill_ckpt_layout(m.file_base.size(), m.n_local, m.n_blocks(), l)) return false;
  if (bits.size() != l->words || m.roots.size() != m.n_local * 32) return false;
  buf->assign(l->size, 0);
  uint8_t* p = buf->data();
  std::memcpy(p, "CP2FILL1", 8);
  const uint64_t w[10] = {m.cell_size, m.block_size, m.n_cells, m.n_slots, m.first_slot, m.n_local, m.src, m.seed, m.file_base.size(), l->n_blocks};
  for (int i = 0; i < 10; ++i) fill_ckpt_put(p + 8 + 8 * i, w[i]);
  if (!m.file_base.empty()) std::memcpy(p + FILL_CKPT_FIXED, m.file_base.data(), m.file_base.size());
  std::memcpy(p + l->roots_at, m.roots.data(), m.roots.size());
  if (l->words) std::memcpy(p + l->bits_at, bits.data(), l->words * 8);
  return true;
}
// the rows of absent blocks as zeros (whatever the compact buffer held there never reaches a file), then the checksum
inline void fill_ckpt_seal(std::vector<uint8_t>* buf, const FillCkptLayout& l) {
  uint8_t* p = buf->data();
  for (uint64_t g = 0; g < l.total; ++g)
    if (!((fill_ckpt_word(p + l.bits_at + (g >> 6) * 8) >> (g & 63)) & 1)) std::memset(p + l.layer0_at + g * 32, 0, 32);
  Checksum64 sum;
  sum.update(p, l.sum_at);
  fill_ckpt_put(p + l.sum_at, sum.finish());
}
inline bool fill_ckpt_serialise(const FillCheckpoint& c, std::vector<uint8_t>* buf) {
  FillCkptLayout l;
  if (c.layer0.size() != c.meta.total() * 32 || !fill_ckpt_begin(c.meta, c.bits, buf, &l)) return false;
  if (!c.layer0.empty()) std::memcpy(buf->data() + l.layer0_at, c.layer0.data(), c.layer0.size());
  fill_ckpt_seal(buf, l);
  return true;
}

// ---- reading ----------------------------------------------------------------------------------------------------------------------------
// The layout the first FILL_CKPT_FIXED bytes of a file announce, every field bounded before anything is sized from it: a reader compares
// l->size with the file's length before it allocates.  false with *err saying what is wrong.
inline bool fill_ckpt_fixed(const uint8_t* p, size_t n, FillCkptMeta* m, FillCkptLayout* l, std::string* err) {
  if (n < FILL_CKPT_FIXED + 8) { *err = "is truncated: shorter than a checkpoint's header"; return false; }
  if (std::memcmp(p, "CP2FILL1", 8) != 0) { *err = "is not a fill checkpoint of this version (magic)"; return false; }
  uint64_t w[10];
  for (int i = 0; i < 10; ++i) w[i] = fill_ckpt_word(p + 8 + 8 * i);
  const uint64_t cell = w[0], block = w[1], cells = w[2], slots = w[3], first = w[4], local = w[5], src = w[6], base_len = w[8], blocks = w[9];
  if (cell == 0 || block < cell || block % cell != 0 || cells == 0 || cells % (block / cell) != 0 || blocks != cells / (block / cell) || src > FILL_SRC_FILE ||
      (src == FILL_SRC_FAKE && base_len != 0) || first > slots || local > slots - first || !fill_ckpt_layout(base_len, local, blocks, l)) {
    *err = "is corrupt: its header states sizes no session has";
    return false;
  }
  m->cell_size = cell; m->block_size = block; m->n_cells = cells; m->n_slots = slots; m->first_slot = first; m->n_local = local; m->src = src; m->seed = w[7];
  return true;
}
// the whole file: sizes, checksum, padding, then (and only then) the copies
inline bool fill_ckpt_parse(const uint8_t* p, size_t n, FillCheckpoint* c, std::string* err) {
  FillCkptLayout l;
  FillCkptMeta m;
  if (!fill_ckpt_fixed(p, n, &m, &l, err)) return false;
  if (n != l.size) {
    *err = n < l.size ? "is truncated: " + std::to_string(n) + " bytes of " + std::to_string(l.size)
                      : "is corrupt: " + std::to_string(n) + " bytes where its header states " + std::to_string(l.size);
    return false;
  }
  Checksum64 sum;
  sum.update(p, l.sum_at);
  if (sum.finish() != fill_ckpt_word(p + l.sum_at)) { *err = "is corrupt (checksum)"; return false; }
  for (size_t i = FILL_CKPT_FIXED + (size_t)l.base_len; i < l.roots_at; ++i)
    if (p[i]) { *err = "is corrupt: bytes after the file base name"; return false; }
  if (l.total & 63) {
    if (fill_ckpt_word(p + l.bits_at + (l.words - 1) * 8) >> (l.total & 63)) { *err = "is corrupt: presence bits past the last block"; return false; }
  }
  m.file_base.assign(reinterpret_cast<const char*>(p) + FILL_CKPT_FIXED, (size_t)l.base_len);
  m.roots.assign(p + l.roots_at, p + l.bits_at);
  c->meta = std::move(m);
  c->bits.resize((size_t)l.words);
  if (l.words) std::memcpy(c->bits.data(), p + l.bits_at, (size_t)l.words * 8);
  c->layer0.assign(p + l.layer0_at, p + l.sum_at);
  return true;
}

// ---- does the checkpoint describe this session? ---------------------------------------------------------------------------------------------
// Empty when `got` (a checkpoint) describes the session `want` states; otherwise the first field that differs, with both values: geometry,
// range, source kind, the seed (fake source), the file base name (slot files), then the stated roots (canonical on both sides), by slot.
inline std::string fill_ckpt_differs(const FillCkptMeta& got, const FillCkptMeta& want) {
  const struct { const char* name; uint64_t a, b; } f[] = {
      {"cell_size", got.cell_size, want.cell_size}, {"block_size", got.block_size, want.block_size}, {"n_cells", got.n_cells, want.n_cells},
      {"n_slots", got.n_slots, want.n_slots},       {"first_slot", got.first_slot, want.first_slot}, {"n_local", got.n_local, want.n_local}};
  for (const auto& x : f)
    if (x.a != x.b) return std::string(x.name) + " differs (checkpoint " + std::to_string(x.a) + ", session " + std::to_string(x.b) + ")";
  if (got.src != want.src)
    return std::string("source differs (checkpoint ") + (got.src == FILL_SRC_FILE ? "slot files" : "fake") + ", session " +
           (want.src == FILL_SRC_FILE ? "slot files" : "fake") + ")";
  if (want.src == FILL_SRC_FAKE && got.seed != want.seed)
    return "seed differs (checkpoint " + std::to_string(got.seed) + ", session " + std::to_string(want.seed) + ")";
  if (want.src == FILL_SRC_FILE && got.file_base != want.file_base)
    return "file base name differs (checkpoint " + got.file_base + ", session " + want.file_base + ")";
  if (got.roots.size() != want.roots.size()) return "slot roots differ in number";
  for (uint64_t s = 0; s < want.n_local; ++s)
    if (std::memcmp(&got.roots[s * 32], &want.roots[s * 32], 32) != 0) return "stated root of slot " + std::to_string(want.first_slot + s) + " differs";
  return std::string();
}

// ---- what the slot files can still back ----------------------------------------------------------------------------------------------------
// (*whole)[i]: how many whole blocks "<base><first_slot + i>.dat" holds, i < n; 0 for a file that does not exist (ENOENT, ENOTDIR): absence is
// a state.  false: a stat failed otherwise and *bad names the file -- slot_file_error(*bad, 0) says so.
inline bool fill_slot_files_cover(const std::string& base, uint64_t first_slot, uint64_t n, size_t block_size, std::vector<uint64_t>* whole,
                                  std::string* bad) {
  whole->assign((size_t)n, 0);
  for (uint64_t i = 0; i < n; ++i) {
    const std::string fname = fill_slot_file_name(base, first_slot + i);
    struct stat sb;
    if (stat(fname.c_str(), &sb) == 0) (*whole)[(size_t)i] = (uint64_t)sb.st_size / block_size;
    else if (errno != ENOENT && errno != ENOTDIR) { *bad = fname; return false; }
  }
  return true;
}

// whole_blocks[local]: how many whole blocks the file of that local slot holds (size / block_size; 0 for a file that does not exist).  Every
// present block at or past it is dropped without a read: its bit cleared, its row of layer 0 zeroed, its global index (local x n_blocks +
// block) appended to `dropped` in ascending order.
inline void fill_ckpt_drop_short(const std::vector<uint64_t>& whole_blocks, uint64_t n_blocks, std::vector<uint64_t>* bits, std::vector<uint8_t>* layer0,
                                 std::vector<uint64_t>* dropped) {
  for (uint64_t local = 0; local < whole_blocks.size(); ++local)
    for (uint64_t b = whole_blocks[local]; b < n_blocks; ++b) {
      const uint64_t g = local * n_blocks + b;
      uint64_t& w = (*bits)[(size_t)(g >> 6)];
      if (!((w >> (g & 63)) & 1)) continue;
      w &= ~(1ULL << (g & 63));
      std::memset(&(*layer0)[(size_t)g * 32], 0, 32);
      dropped->push_back(g);
    }
}

// ---- the read plan of the re-check ---------------------------------------------------------------------------------------------------------
// Every present block exactly once, as its global index in ascending order -- by file, and inside a file by offset -- cut into chunks of at
// most `chunk` blocks; a chunk's blocks are read file by file (runs).
struct FillReadPlan {
  std::vector<uint64_t> g;                 // present blocks: local x n_blocks + block, ascending
  uint64_t n_blocks = 1;
  size_t chunk = 1;
  struct Run { uint64_t local; size_t i0, i1; };   // entries [i0, i1) of g lie in the file of local slot `local`
  size_t n_chunks() const { return (g.size() + chunk - 1) / chunk; }
  size_t chunk_begin(size_t c) const { return c * chunk; }
  size_t chunk_end(size_t c) const { return g.size() - c * chunk < chunk ? g.size() : (c + 1) * chunk; }
  std::vector<Run> runs(size_t c) const {
    std::vector<Run> r;
    for (size_t i = chunk_begin(c); i < chunk_end(c); ++i) {
      const uint64_t local = g[i] / n_blocks;
      if (r.empty() || r.back().local != local) r.push_back({local, i, i});
      r.back().i1 = i + 1;
    }
    return r;
  }
};
inline FillReadPlan fill_read_plan(const std::vector<uint64_t>& bits, uint64_t total, uint64_t n_blocks, size_t chunk) {
  FillReadPlan p;
  p.n_blocks = n_blocks;
  p.chunk = chunk ? chunk : 1;
  for (size_t w = 0; w < bits.size(); ++w) {
    uint64_t present = bits[w];
    while (present) {
      const uint64_t g = (uint64_t)w * 64 + (uint64_t)__builtin_ctzll(present);
      present &= present - 1;
      if (g < total) p.g.push_back(g);
    }
  }
  return p;
}

// Chunk k of the plan into `host` (chunk x block_size bytes; entry i of the chunk at i - chunk_begin(k)), run by run: each file
// "<base><first_slot + local>.dat" opened once, read in ascending offset order by the slot-file read rule, and closed.  false: *bad names the
// first file that could not be opened (*err 0) or whose read failed (*err its errno), as slot_file_error takes them; a read that fails is an
// error, never a dropped block.
inline bool fill_read_chunk(const FillReadPlan& rp, size_t k, const std::string& base, uint64_t first_slot, size_t block_size, uint8_t* host,
                            std::string* bad, int* err) {
  const size_t i0 = rp.chunk_begin(k);
  for (const FillReadPlan::Run& run : rp.runs(k)) {
    const std::string fname = fill_slot_file_name(base, first_slot + run.local);
    const int e = slot_file_read_list(fname, run.i1 - run.i0, [&](size_t) { return block_size; },
                                      [&](size_t i) { return (rp.g[run.i0 + i] % rp.n_blocks) * block_size; },
                                      [&](size_t i) { return host + (run.i0 + i - i0) * block_size; });
    if (e >= 0) { *bad = fname; *err = e; return false; }
  }
  return true;
}

}  // namespace cp2i
