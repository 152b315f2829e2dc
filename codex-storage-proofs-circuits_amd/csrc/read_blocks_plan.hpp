// The host side of a verified read-back of listed blocks across datasets (csrc/read_blocks.cpp: cp2_datasets_read_blocks and
// cp2_dataset_read_blocks): which calls are refused and with which words, in which order the blocks of a chunk are read, how the requests
// are cut into chunks, where each request's path starts in the packed output, and the two device address tables -- the kept block root of
// every request and every row of every path -- from a dataset's layout and the base address of its kept node buffer.  The reader at the
// end runs the read plan of one chunk against the slot files under the builders' read rule (slot_file_read_rest: zeros past the end,
// errors are errors).  Reads are buffered preads: O_DIRECT and the mapped mode of the ingestion pipe are not used here (a listed block is
// 64 KiB somewhere in a file, not a stream).  No HIP in here: tests/host_check/read_blocks_check.cpp runs all of it on the CPU, under
// AddressSanitizer + UBSan, and tests/read_blocks_models.py restates the arithmetic.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "block_proof_plan.hpp"
#include "fill_pipeline.hpp"   // fill_slot_file_name and the slot-file read rule: slot_file_read_rest, slot_file_error
#include "repair_plan.hpp"
#include "workers.hpp"

namespace cp2i {

constexpr int READ_BLOCKS_CHECK_ONLY = 1;             // CP2_READ_CHECK_ONLY (include/codex_p2.h; read_blocks.cpp asserts the equality)

// what the plan knows of one listed dataset
struct ReadDataset {
  bool null = false;                                  // ds[k] == NULL
  bool foreign = false;                               // a dataset of another context
  size_t same_as = 0;                                 // the lowest index in `ds` that lists the same handle (k itself when it is the first)
  size_t cell_size = 0, block_size = 0;
  uint64_t n_cells = 0, first_slot = 0, n_local = 0;
  int mode = 0;                                       // 1 every node kept, 2 compact, 0 roots only
  bool whole = false;                                 // the kept layers are those of whole slot trees (not the unit builds)
  bool from_file = false;
  std::string base;                                   // slot files "<base><slot>.dat"
  uint64_t seed = 0;                                  // fake source: the dataset seed
  uint64_t nodes = 0;                                 // device address of row 0 of the kept node buffer
  uint64_t roots = 0;                                 // device address of the local slot roots, n_local x 32 bytes (repair_many_plan.hpp)
  // where the block roots are kept: every node -- boff.back(), bsizes.back() (repair_row_full); compact -- coff[0], csizes[0]
  uint64_t root_off = 0, root_size = 0;
  std::vector<uint64_t> offs, sizes;                  // the big tree's layers, depth + 1 of them: toff / tsizes, or coff / csizes
  uint64_t n_blocks() const { return cell_size && block_size >= cell_size ? n_cells / (block_size / cell_size) : 0; }
  size_t depth() const { return block_proof_depth(n_blocks()); }
};

// which of the call's pointers are there
struct ReadArgs {
  bool ds = false, req = false, data = false, paths = false, path_off = false, status = false;
  size_t n_ds = 0, n = 0;
  int flags = 0;
};

// ---- validation: before any device or file work ---------------------------------------------------------------------------------------
// false with *err naming the rule and the dataset or request index (the lowest that breaks one; arguments first, then datasets, then
// requests).  req holds n x 3: index into ds, dataset slot, block of the slot.
inline bool read_blocks_validate(const ReadArgs& a, const std::vector<ReadDataset>& ds, const uint64_t* req, std::string* err) {
  if (a.flags & ~READ_BLOCKS_CHECK_ONLY) {
    char b[16];
    std::snprintf(b, sizeof b, "%x", (unsigned)(a.flags & ~READ_BLOCKS_CHECK_ONLY));
    *err = std::string("read blocks: unknown flag bits 0x") + b;
    return false;
  }
  if ((a.paths && !a.path_off) || (!a.paths && a.path_off)) {
    *err = a.paths ? "read blocks: paths without path_off" : "read blocks: path_off without paths";
    return false;
  }
  if (a.n == 0) return true;
  if (!a.ds || !a.req || !a.status) {
    *err = "read blocks: ds, req and status must not be NULL when n > 0";
    return false;
  }
  if (!a.data && !(a.flags & READ_BLOCKS_CHECK_ONLY)) {
    *err = "read blocks: data is NULL without CP2_READ_CHECK_ONLY";
    return false;
  }
  for (size_t k = 0; k < ds.size(); ++k) {
    const ReadDataset& d = ds[k];
    const std::string who = "read blocks: dataset " + std::to_string(k) + ": ";
    if (d.null) { *err = who + "NULL dataset"; return false; }
    if (d.foreign) { *err = who + "it belongs to another context"; return false; }
    if (d.cell_size != ds[0].cell_size || d.block_size != ds[0].block_size) {
      *err = who + "cell_size " + std::to_string(d.cell_size) + ", block_size " + std::to_string(d.block_size) + " differ from dataset 0's " +
             std::to_string(ds[0].cell_size) + ", " + std::to_string(ds[0].block_size);
      return false;
    }
    if (d.mode == 0) {
      *err = who + "block proofs: this dataset keeps only its slot roots, no block roots and no layers above them to take a path from: build it with every "
                   "node or the compact layers kept (cp2_set_keep_trees)";
      return false;
    }
    if (!d.whole || d.offs.size() != d.depth() + 1 || d.sizes.size() != d.depth() + 1) {
      *err = who + "block proofs: the kept layers of this dataset are not those of whole slot trees";
      return false;
    }
  }
  for (size_t i = 0; i < a.n; ++i) {
    const uint64_t k = req[3 * i], s = req[3 * i + 1], b = req[3 * i + 2];
    const std::string who = "read blocks: request " + std::to_string(i) + ": ";
    if (k >= a.n_ds) {
      *err = who + "dataset index " + std::to_string(k) + " is not below n_ds = " + std::to_string(a.n_ds);
      return false;
    }
    const ReadDataset& d = ds[k];
    if (s < d.first_slot || s - d.first_slot >= d.n_local) {
      *err = who + "slot " + std::to_string(s) + " is not inside the local range " + std::to_string(d.first_slot) + " + " + std::to_string(d.n_local) +
             " of dataset " + std::to_string(k);
      return false;
    }
    if (b >= d.n_blocks()) {
      *err = who + "block " + std::to_string(b) + " of slot " + std::to_string(s) + " is not below nBlocks = " + std::to_string(d.n_blocks()) + " of dataset " +
             std::to_string(k);
      return false;
    }
  }
  return true;
}

// ---- chunks ----------------------------------------------------------------------------------------------------------------------------
// requests per chunk: repair_check_with's expression (repair.cpp), so that a chunk of the plan is a chunk of the data path
inline size_t read_blocks_chunk(size_t stage_bytes, size_t block_size, size_t n) {
  return std::max<size_t>(1, std::min<size_t>(n, (stage_bytes / 2) / block_size));
}

// ---- the read plan --------------------------------------------------------------------------------------------------------------------
// Chunk k holds requests [k * chunk, min(n, (k + 1) * chunk)) in request order -- request i lands in row i, whatever the order it is
// read in.  Inside a chunk the file-sourced requests are grouped by slot file (the dataset listed first under that handle, the slot),
// files in ascending (dataset, slot) order, each file's requests in ascending offset, a repeated block once per request: a chunk opens
// every file it needs once and reads it front to back.  Fake-source requests are in no group (the device regenerates them).
struct ReadGroup {
  size_t ds = 0;                                      // same_as of the requests' dataset
  uint64_t slot = 0;
  size_t begin = 0, end = 0;                          // its requests: order[begin, end)
};
struct ReadPlan {
  size_t n = 0, chunk = 1;
  std::vector<size_t> order;                          // request indices of every group, chunk after chunk
  std::vector<ReadGroup> groups;
  std::vector<size_t> first_group;                    // groups of chunk k: [first_group[k], first_group[k + 1])
  size_t n_chunks() const { return n ? (n + chunk - 1) / chunk : 0; }
  size_t chunk_begin(size_t k) const { return k * chunk; }
  size_t chunk_end(size_t k) const { return std::min(n, (k + 1) * chunk); }
};
inline ReadPlan read_blocks_plan(const std::vector<ReadDataset>& ds, const uint64_t* req, size_t n, size_t chunk) {
  ReadPlan p;
  p.n = n;
  p.chunk = std::max<size_t>(1, chunk);
  p.first_group.push_back(0);
  for (size_t k = 0; k < p.n_chunks(); ++k) {
    std::vector<size_t> idx;
    for (size_t i = p.chunk_begin(k); i < p.chunk_end(k); ++i)
      if (ds[req[3 * i]].from_file) idx.push_back(i);
    auto file_of = [&](size_t i) { return ds[req[3 * i]].same_as; };
    std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {
      if (file_of(a) != file_of(b)) return file_of(a) < file_of(b);
      if (req[3 * a + 1] != req[3 * b + 1]) return req[3 * a + 1] < req[3 * b + 1];
      if (req[3 * a + 2] != req[3 * b + 2]) return req[3 * a + 2] < req[3 * b + 2];
      return a < b;
    });
    for (size_t i : idx) {
      if (p.groups.size() == p.first_group.back() || p.groups.back().ds != file_of(i) || p.groups.back().slot != req[3 * i + 1]) {
        ReadGroup g;
        g.ds = file_of(i);
        g.slot = req[3 * i + 1];
        g.begin = g.end = p.order.size();
        p.groups.push_back(g);
      }
      p.order.push_back(i);
      p.groups.back().end = p.order.size();
    }
    p.first_group.push_back(p.groups.size());
  }
  return p;
}

// ---- packed paths ----------------------------------------------------------------------------------------------------------------------
// request i's path: rows [off[i], off[i + 1]) of `paths`, as many as the block-proof depth of its dataset; off has n + 1 entries
inline std::vector<uint64_t> read_blocks_path_off(const std::vector<ReadDataset>& ds, const uint64_t* req, size_t n) {
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + ds[req[3 * i]].depth();
  return off;
}

// ---- the address tables ----------------------------------------------------------------------------------------------------------------
// the kept block root of one request: the row repair compares with (repair_dataset_row), as an absolute device address
inline uint64_t read_blocks_kept_addr(const ReadDataset& d, uint64_t slot, uint64_t block) {
  const uint64_t local = slot - d.first_slot;
  const uint64_t row = d.mode == 1 ? repair_row_full(d.root_off, d.root_size, d.n_blocks(), local, block) : repair_row_compact(d.root_off, d.root_size, local, block);
  return d.nodes + row * 32;
}
// one entry per request, then one per path row (entry n + path_off[i] + l: sibling l of request i, bottom first; 0 for the ZERO
// sibling): what one k_gather_addr launch fetches, and the first n entries are what k_repair_compare_addr compares with
inline std::vector<uint64_t> read_blocks_addr_table(const std::vector<ReadDataset>& ds, const uint64_t* req, size_t n, const std::vector<uint64_t>& path_off) {
  std::vector<uint64_t> t(n + (size_t)path_off[n], 0), rows;
  for (size_t i = 0; i < n; ++i) {
    const ReadDataset& d = ds[req[3 * i]];
    const uint64_t s = req[3 * i + 1], b = req[3 * i + 2];
    t[i] = read_blocks_kept_addr(d, s, b);
    const size_t depth = d.depth();
    rows.assign(depth, 0);
    block_proof_rows(d.offs, d.sizes, s - d.first_slot, b, depth, rows.data());
    for (size_t l = 0; l < depth; ++l) t[n + (size_t)path_off[i] + l] = rows[l] == BLOCK_PROOF_NO_ROW ? 0 : d.nodes + rows[l] * 32;
  }
  return t;
}

// ---- the reader ------------------------------------------------------------------------------------------------------------------------
// The file-sourced requests of chunk k, each block into row_of(i) (block_size bytes), the chunk's files spread over `threads` threads.
// false: *bad names the first file (in plan order) that could not be opened (*err 0) or whose read failed (*err its errno), as
// slot_file_error takes them; no row of the chunk may be used then.
template <typename RowOf>
inline bool read_blocks_read_chunk(const ReadPlan& p, size_t k, const std::vector<ReadDataset>& ds, const uint64_t* req, size_t block_size, RowOf row_of,
                                   int threads, std::string* bad, int* err) {
  const size_t g0 = p.first_group[k], ng = p.first_group[k + 1] - g0;
  std::vector<int> failed(ng, -1);                    // per group: -1 fine, else the errno (0: open)
  on_threads(threads, ng, [&](int, size_t j) {
    const ReadGroup& g = p.groups[g0 + j];
    failed[j] = slot_file_read_list(fill_slot_file_name(ds[g.ds].base, g.slot), g.end - g.begin, [&](size_t) { return block_size; },
                                    [&](size_t q) { return req[3 * p.order[g.begin + q] + 2] * (uint64_t)block_size; },
                                    [&](size_t q) { return row_of(p.order[g.begin + q]); });
    return true;
  });
  for (size_t j = 0; j < ng; ++j)
    if (failed[j] >= 0) {
      *bad = fill_slot_file_name(ds[p.groups[g0 + j].ds].base, p.groups[g0 + j].slot);
      *err = failed[j];
      return false;
    }
  return true;
}

}  // namespace cp2i
