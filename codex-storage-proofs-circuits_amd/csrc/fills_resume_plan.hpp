// The host side of cp2_fills_resume_many (csrc/fills_resume_many.cpp): many fill sessions resumed from their checkpoints in one pass.  The
// call is defined by the call that exists -- cp2_fill_resume per entry -- so the words of a refusal are that call's, with the entry index
// in front.  Here: the order of the checks over plain inputs (arguments, then per entry what cp2_fill_begin refuses and the one shape of
// the data path; then the checkpoints; then the slot files), the lowest index winning inside each stage; and the plan of the re-check
// from N (bitmap, n_blocks, first_slot, source) tuples after the short-file drop: the request list -- every present block of every
// entry once, in (entry, global index) order, as the (owner, slot, block) triples read_blocks_plan.hpp groups and reads --, the owner
// descriptions its reader needs (from_file, same_as, base), the address table (session buffer + layer-0 row x 32) that
// k_block_root_recheck_addr judges against, the seeds and first cells of fake-source requests, the turn from a verdict index back to
// (entry, global index), and the per-entry drop lists.  No HIP in here: tests/host_check/fills_resume_many_check.cpp runs all of it on
// the CPU and against real files, under AddressSanitizer + UBSan (the reader under ThreadSanitizer too), and
// tests/fills_resume_many_models.py restates it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "fill_checkpoint.hpp"
#include "read_blocks_plan.hpp"

namespace cp2i {

constexpr int FILLS_RESUME_TRUST_FILES = 1;           // CP2_RESUME_TRUST_FILES (include/codex_p2.h; fills_resume_many.cpp asserts the equality)
constexpr int FILLS_RESUME_INVALID = -1, FILLS_RESUME_IO = -5;   // CP2_ERR_INVALID, CP2_ERR_IO (asserted there too)

// which of the call's pointers are there
struct ResumeManyArgs {
  bool cfgs = false, ranges = false, slot_roots = false, paths = false, out = false;
  size_t n_fills = 0;
  int flags = 0;
};
// what the argument checks look at of one entry
struct ResumeManyEntry {
  bool cfg = false, slot_roots = false, path = false;   // cfgs[k], slot_roots[k], paths[k] are not NULL
  size_t cell_size = 0, block_size = 0;
};
// which entry broke a rule (n_fills: none in particular), the status and the text
struct ResumeManyRefusal {
  size_t index = 0;
  int status = 0;
  std::string text;
};

inline std::string fills_resume_entry(size_t k) { return "fills: entry " + std::to_string(k) + ": "; }

// ---- stage 1: arguments, then every entry in order ---------------------------------------------------------------------------------------
// begin_refuses(k, &text): whether cp2_fill_begin refuses entry k (its cfg, range and roots are there), in its words.  false with the
// first refusal: unknown flag bits, a NULL array with n_fills > 0, then per entry a NULL, what cp2_fill_begin refuses, a shape other
// than entry 0's.  Always CP2_ERR_INVALID.
template <class Begin>
inline bool fills_resume_check_args(const ResumeManyArgs& a, const ResumeManyEntry* e, Begin begin_refuses, ResumeManyRefusal* why) {
  const auto refuse = [&](size_t k, const std::string& text) {
    *why = {k, FILLS_RESUME_INVALID, text};
    return false;
  };
  if (a.flags & ~FILLS_RESUME_TRUST_FILES) {
    char b[16];
    std::snprintf(b, sizeof b, "%x", (unsigned)(a.flags & ~FILLS_RESUME_TRUST_FILES));
    return refuse(a.n_fills, std::string("fills: unknown resume flag bits 0x") + b);
  }
  if (a.n_fills == 0) return true;
  if (!a.cfgs || !a.ranges || !a.slot_roots || !a.paths || !a.out)
    return refuse(a.n_fills, "fills: cfgs, ranges, slot_roots, paths and out must not be NULL when n_fills > 0");
  for (size_t k = 0; k < a.n_fills; ++k) {
    if (!e[k].cfg) return refuse(k, fills_resume_entry(k) + "cfgs[" + std::to_string(k) + "] is NULL");
    if (!e[k].slot_roots) return refuse(k, fills_resume_entry(k) + "slot_roots[" + std::to_string(k) + "] is NULL");
    if (!e[k].path) return refuse(k, fills_resume_entry(k) + "paths[" + std::to_string(k) + "] is NULL");
    std::string text;
    if (begin_refuses(k, &text)) return refuse(k, fills_resume_entry(k) + text);
    if (e[k].cell_size != e[0].cell_size || e[k].block_size != e[0].block_size)
      return refuse(k, fills_resume_entry(k) + "cell_size " + std::to_string(e[k].cell_size) + ", block_size " + std::to_string(e[k].block_size) +
                           " differ from entry 0's " + std::to_string(e[0].cell_size) + ", " + std::to_string(e[0].block_size) +
                           ": the sessions of one call share the data path's shape");
  }
  return true;
}

// ---- stages 2 and 3: what was found per entry, possibly on many threads, and the lowest index that failed ----------------------------------
// status 0: fine
struct ResumeManyFound {
  int status = 0;
  std::string text;
};
// the checkpoint of one entry, read and parsed (`got`), against the session the entry states: CP2_ERR_INVALID in cp2_fill_resume's words
inline ResumeManyFound fills_resume_describes(const FillCkptMeta& got, const FillCkptMeta& want, const std::string& path) {
  const std::string differs = fill_ckpt_differs(got, want);
  if (differs.empty()) return {};
  return {FILLS_RESUME_INVALID, "fill: checkpoint " + path + " describes another session: " + differs};
}
inline bool fills_resume_first_failed(const std::vector<ResumeManyFound>& found, ResumeManyRefusal* why) {
  for (size_t k = 0; k < found.size(); ++k)
    if (found[k].status != 0) {
      *why = {k, found[k].status, fills_resume_entry(k) + found[k].text};
      return true;
    }
  return false;
}

// ---- the plan of the re-check ------------------------------------------------------------------------------------------------------------
// one entry after the short-file drop
struct ResumeManySession {
  std::vector<uint64_t> bits;                          // presence: bit (local x n_blocks + block)
  uint64_t n_blocks = 0, first_slot = 0, n_local = 0;
  bool from_file = false;
  std::string base;                                    // slot files "<base><slot>.dat"
  uint64_t seed = 0;                                   // fake source: the dataset seed
  uint64_t layer0 = 0;                                 // device address of row 0 of the session's compact buffer (layer 0 starts there)
};

struct FillsResumePlan {
  size_t block_size = 0;
  std::vector<ReadDataset> owners;                     // one per entry: what read_blocks_plan and read_blocks_read_chunk look at
  std::vector<uint64_t> req;                           // n x 3: entry, dataset slot, block of the slot
  std::vector<uint64_t> first;                         // n_fills + 1: the requests of entry k are [first[k], first[k + 1])
  std::vector<uint64_t> g;                             // request i's global index in its entry: local x n_blocks + block
  std::vector<uint64_t> addr;                          // request i's kept row: layer0 of its entry + g x 32
  std::vector<uint8_t> fake;                           // empty: no fake-source request; else per request 1 = regenerated on the device
  std::vector<uint64_t> seeds, firsts;                 // ... from this slot seed and first cell
  uint64_t n_file = 0;                                 // requests read from slot files

  size_t n() const { return g.size(); }
  size_t n_fills() const { return owners.size(); }

  // seed_of(dataset seed, slot): cp2_slot_seed
  template <class SeedOf>
  void build(const std::vector<ResumeManySession>& s, size_t cell_size, size_t block, SeedOf seed_of) {
    block_size = block;
    const uint64_t cpb = block / cell_size;
    owners.assign(s.size(), ReadDataset());
    req.clear(); g.clear(); addr.clear(); fake.clear(); seeds.clear(); firsts.clear();
    first.assign(s.size() + 1, 0);
    n_file = 0;
    bool any_fake = false;
    for (size_t k = 0; k < s.size(); ++k) {
      ReadDataset& d = owners[k];
      d.same_as = k;
      d.from_file = s[k].from_file;
      d.base = s[k].base;
      if (d.from_file)                                 // two entries over one base share its files: a chunk opens each once
        for (size_t j = 0; j < k; ++j)
          if (s[j].from_file && s[j].base == s[k].base) { d.same_as = j; break; }
      d.cell_size = cell_size; d.block_size = block;
      d.n_cells = s[k].n_blocks * cpb;
      d.first_slot = s[k].first_slot; d.n_local = s[k].n_local;
      d.seed = s[k].seed;
      const uint64_t total = s[k].n_local * s[k].n_blocks;
      for (size_t w = 0; w < s[k].bits.size(); ++w) {
        uint64_t present = s[k].bits[w];
        while (present) {
          const uint64_t gi = (uint64_t)w * 64 + (uint64_t)__builtin_ctzll(present);
          present &= present - 1;
          if (gi >= total) continue;
          const uint64_t slot = s[k].first_slot + gi / s[k].n_blocks, b = gi % s[k].n_blocks;
          req.push_back(k); req.push_back(slot); req.push_back(b);
          g.push_back(gi);
          addr.push_back(s[k].layer0 + gi * 32);
          fake.push_back(s[k].from_file ? 0 : 1);
          seeds.push_back(s[k].from_file ? 0 : seed_of(s[k].seed, slot));
          firsts.push_back(s[k].from_file ? 0 : b * cpb);
          if (s[k].from_file) ++n_file; else any_fake = true;
        }
      }
      first[k + 1] = g.size();
    }
    if (!any_fake) { fake.clear(); seeds.clear(); firsts.clear(); }
  }

  // the read plan over `chunk` requests a chunk (read_blocks_chunk), and chunk k of it read into row_of(i): read_blocks_plan.hpp's
  ReadPlan read_plan(size_t chunk) const { return read_blocks_plan(owners, req.data(), n(), chunk); }
  template <typename RowOf>
  bool read_chunk(const ReadPlan& p, size_t k, RowOf row_of, int threads, std::string* bad, int* err) const {
    return read_blocks_read_chunk(p, k, owners, req.data(), block_size, row_of, threads, bad, err);
  }

  // request i belongs to entry *k, block *gi of it
  void where(size_t i, size_t* k, uint64_t* gi) const {
    *k = (size_t)(std::upper_bound(first.begin(), first.end(), (uint64_t)i) - first.begin()) - 1;
    *gi = g[i];
  }
  // per entry, ascending: the global indices of the blocks whose verdict is not 0 -- what FillPlan::drop takes
  std::vector<std::vector<uint64_t>> drops(const uint32_t* verdict) const {
    std::vector<std::vector<uint64_t>> d(n_fills());
    for (size_t k = 0; k < n_fills(); ++k)
      for (uint64_t i = first[k]; i < first[k + 1]; ++i)
        if (verdict[i] != 0) d[k].push_back(g[i]);
    return d;
  }
};

// ---- the uploads of the open step ----------------------------------------------------------------------------------------------------------
// Segments of the given sizes (per session its roots, then its layer 0) travel through one staging buffer of `piece` bytes: cut into
// (segment, offset in it, bytes, offset in the buffer) in order, a piece closed (flush true on its last cut) when the buffer is full.
struct ResumeManyCut {
  size_t seg = 0, off = 0, len = 0, at = 0;
  bool flush = false;
};
inline std::vector<ResumeManyCut> fills_resume_cuts(const std::vector<size_t>& sizes, size_t piece) {
  std::vector<ResumeManyCut> cuts;
  piece = std::max<size_t>(piece, 1);
  size_t at = 0;
  for (size_t s = 0; s < sizes.size(); ++s)
    for (size_t off = 0; off < sizes[s];) {
      const size_t len = std::min(sizes[s] - off, piece - at);
      cuts.push_back({s, off, len, at, false});
      off += len;
      at += len;
      if (at == piece) { cuts.back().flush = true; at = 0; }
    }
  if (!cuts.empty()) cuts.back().flush = true;
  return cuts;
}

}  // namespace cp2i
