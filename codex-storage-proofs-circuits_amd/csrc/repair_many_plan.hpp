// The host side of cp2_datasets_repair_blocks_many (csrc/repair_many.cpp): replacement blocks of many datasets judged in one pass and
// written back on many threads.  What a request means is defined by the calls that exist -- an empty path is cp2_dataset_repair_blocks'
// comparison with the kept block root, a whole path is cp2_dataset_repair_blocks_proved's walk to the dataset's own slot root -- so this
// header holds only what the many-dataset form adds: which calls are refused and with which words (arguments, then datasets, then the
// lowest offending request), how the requests are cut into chunks (repair_check_with's expression, through read_blocks_chunk), the
// descriptor k_repair_judge_many reads for every request, the matched requests grouped by slot FILE NAME (two handles over one base name
// share their files), and the writer that spreads those files over threads.  A listed dataset is read_blocks_plan.hpp's ReadDataset.  No
// HIP in here: tests/host_check/repair_many_check.cpp runs all of it on the CPU under AddressSanitizer + UBSan, the writer also under
// ThreadSanitizer, and tests/repair_many_models.py restates the arithmetic.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "read_blocks_plan.hpp"

namespace cp2i {

constexpr int REPAIR_MANY_CHECK_ONLY = 1;             // CP2_REPAIR_CHECK_ONLY (include/codex_p2.h; repair_many.cpp asserts the equality)

// which of the call's pointers are there
struct RepairManyArgs {
  bool ds = false, req = false, data = false, paths = false, path_off = false, status = false;
  size_t n_ds = 0, n = 0;
  int flags = 0;
};

// one descriptor of the device's request table: cp2k::RepairManyReq (kernels.hpp) restated, field by field
struct RepairManyDesc {
  uint64_t want;         // device address of the 32-byte row the request is judged against
  uint64_t blk;          // block of the slot: the walk's first index
  uint64_t n_blocks;     // blocks of a slot of its dataset: the walk's first layer size
  uint64_t path_at;      // first row of its path inside the chunk's staged paths
  uint32_t len;          // rows of its path: 0, or its dataset's depth
  uint32_t reserved;     // 0
};

// the slot file a request of dataset k goes to is named by the dataset listed first with that base name (file-sourced), or under that
// handle (fake source: no file, the key of the duplicate rule only)
inline std::vector<size_t> repair_many_file_of(const std::vector<ReadDataset>& ds) {
  std::vector<size_t> f(ds.size());
  std::unordered_map<std::string, size_t> first;      // base name -> the first file-sourced dataset over it: linear in the datasets
  first.reserve(ds.size());
  for (size_t k = 0; k < ds.size(); ++k) f[k] = ds[k].from_file ? first.emplace(ds[k].base, k).first->second : ds[k].same_as;
  return f;
}

// ---- validation: before any device or file work -------------------------------------------------------------------------------------------
// false with *err naming the rule and the dataset or request index: arguments first, then the lowest dataset, then the lowest request that
// breaks a rule -- for the same (slot file, block) twice that is the later of the pair.  req holds n x 3: index into ds, dataset slot,
// block of the slot; path_off n + 1 entries or none.
inline bool repair_many_validate(const RepairManyArgs& a, const std::vector<ReadDataset>& ds, const uint64_t* req, const uint64_t* path_off,
                                 std::string* err) {
  if (a.flags & ~REPAIR_MANY_CHECK_ONLY) {
    char b[16];
    std::snprintf(b, sizeof b, "%x", (unsigned)(a.flags & ~REPAIR_MANY_CHECK_ONLY));
    *err = std::string("repair many: unknown flag bits 0x") + b;
    return false;
  }
  if ((a.paths && !a.path_off) || (!a.paths && a.path_off)) {
    *err = a.paths ? "repair many: paths without path_off" : "repair many: path_off without paths";
    return false;
  }
  if (a.n == 0) return true;
  if (!a.ds || !a.req || !a.data || !a.status) {
    *err = "repair many: ds, req, data and status must not be NULL when n > 0";
    return false;
  }
  if (path_off && path_off[0] != 0) {
    *err = "repair many: path_off[0] is " + std::to_string(path_off[0]) + ", not 0";
    return false;
  }
  for (size_t k = 0; k < ds.size(); ++k) {
    const ReadDataset& d = ds[k];
    const std::string who = "repair many: dataset " + std::to_string(k) + ": ";
    if (d.null) { *err = who + "NULL dataset"; return false; }
    if (d.foreign) { *err = who + "it belongs to another context"; return false; }
    if (d.cell_size != ds[0].cell_size || d.block_size != ds[0].block_size) {
      *err = who + "cell_size " + std::to_string(d.cell_size) + ", block_size " + std::to_string(d.block_size) + " differ from dataset 0's " +
             std::to_string(ds[0].cell_size) + ", " + std::to_string(ds[0].block_size);
      return false;
    }
  }
  size_t bad = a.n;                                   // the lowest request that breaks a rule of its own
  for (size_t i = 0; i < a.n && bad == a.n; ++i) {
    const uint64_t k = req[3 * i], s = req[3 * i + 1], b = req[3 * i + 2];
    auto who = [i] { return "repair many: request " + std::to_string(i) + ": "; };   // (made only for a refusal)
    if (k >= a.n_ds) {
      *err = who() + "dataset index " + std::to_string(k) + " is not below n_ds = " + std::to_string(a.n_ds);
      bad = i;
      break;
    }
    const ReadDataset& d = ds[k];
    if (path_off && path_off[i + 1] < path_off[i]) {
      *err = who() + "path_off decreases from " + std::to_string(path_off[i]) + " to " + std::to_string(path_off[i + 1]);
      bad = i;
    } else if (path_off && path_off[i + 1] != path_off[i] && path_off[i + 1] - path_off[i] != d.depth()) {
      *err = who() + "a path of " + std::to_string(path_off[i + 1] - path_off[i]) + " row(s) is neither empty nor the depth " + std::to_string(d.depth()) +
             " of dataset " + std::to_string(k);
      bad = i;
    } else if ((!path_off || path_off[i + 1] == path_off[i]) && d.mode == 0) {
      *err = who() + "an empty path for dataset " + std::to_string(k) + ", which keeps only its slot roots, no block roots to check a block against: give the path";
      bad = i;
    } else if ((!path_off || path_off[i + 1] == path_off[i]) && (!d.whole || d.offs.size() != d.depth() + 1 || d.sizes.size() != d.depth() + 1)) {
      *err = who() + "an empty path for dataset " + std::to_string(k) + ", whose kept layers are not those of whole slot trees: give the path";
      bad = i;
    } else if (s < d.first_slot || s - d.first_slot >= d.n_local) {
      *err = who() + "slot " + std::to_string(s) + " is not inside the local range " + std::to_string(d.first_slot) + " + " + std::to_string(d.n_local) +
             " of dataset " + std::to_string(k);
      bad = i;
    } else if (b >= d.n_blocks()) {
      *err = who() + "block " + std::to_string(b) + " of slot " + std::to_string(s) + " is not below nBlocks = " + std::to_string(d.n_blocks()) + " of dataset " +
             std::to_string(k);
      bad = i;
    } else if (!d.from_file && !(a.flags & REPAIR_MANY_CHECK_ONLY)) {
      *err = who() + "dataset " + std::to_string(k) + " has the fake source and no slot files to write: only CP2_REPAIR_CHECK_ONLY is accepted";
      bad = i;
    }
  }
  // the same (slot file, block) twice among the requests below `bad`, which are all in range: the lowest later one of a pair, found in
  // one pass over a hash of the keys (the requests of thousands of datasets are checked in the time one dataset's are)
  const std::vector<size_t> file_of = repair_many_file_of(ds);
  auto key = [&](size_t i) { return std::make_tuple(file_of[req[3 * i]], req[3 * i + 1], req[3 * i + 2]); };
  struct KeyHash {
    size_t operator()(const std::tuple<size_t, uint64_t, uint64_t>& k) const {
      uint64_t h = std::get<0>(k) * 0x9E3779B97F4A7C15ULL;
      h = (h ^ (h >> 29) ^ std::get<1>(k)) * 0xBF58476D1CE4E5B9ULL;
      h = (h ^ (h >> 32) ^ std::get<2>(k)) * 0x94D049BB133111EBULL;
      return (size_t)(h ^ (h >> 31));
    }
  };
  std::unordered_map<std::tuple<size_t, uint64_t, uint64_t>, size_t, KeyHash> seen;
  seen.reserve(bad);
  size_t twice = bad, first = 0;
  for (size_t i = 0; i < bad; ++i) {
    const auto at = seen.emplace(key(i), i);
    if (!at.second) { twice = i; first = at.first->second; break; }
  }
  if (twice < bad) {
    *err = "repair many: request " + std::to_string(twice) + ": (slot " + std::to_string(req[3 * twice + 1]) + ", block " + std::to_string(req[3 * twice + 2]) +
           ") of dataset " + std::to_string(req[3 * twice]) + " is the block of request " + std::to_string(first) + " again";
    return false;
  }
  return bad == a.n;
}

// ---- the descriptor table -----------------------------------------------------------------------------------------------------------------
// One entry per request, uploaded once; chunk c covers requests [c * chunk, ...) and stages the packed path rows path_off[c0] ...
// path_off[c0 + m) at row 0 of the staging buffer, so path_at is relative to the first request of the request's own chunk.  want: an
// empty path -- the kept block root (read_blocks_kept_addr); a whole path -- row slot - first_slot of the dataset's own slot roots.
inline std::vector<RepairManyDesc> repair_many_table(const std::vector<ReadDataset>& ds, const uint64_t* req, const uint64_t* path_off, size_t n,
                                                     size_t chunk) {
  std::vector<RepairManyDesc> t(n);
  chunk = std::max<size_t>(1, chunk);
  for (size_t i = 0; i < n; ++i) {
    const ReadDataset& d = ds[req[3 * i]];
    const uint64_t s = req[3 * i + 1], b = req[3 * i + 2];
    const uint64_t len = path_off ? path_off[i + 1] - path_off[i] : 0;
    RepairManyDesc& q = t[i];
    q.want = len ? d.roots + (s - d.first_slot) * 32 : read_blocks_kept_addr(d, s, b);
    q.blk = b;
    q.n_blocks = d.n_blocks();
    q.path_at = path_off ? path_off[i] - path_off[i / chunk * chunk] : 0;
    q.len = (uint32_t)len;
    q.reserved = 0;
  }
  return t;
}
// the most path rows any chunk stages
inline uint64_t repair_many_most_path_rows(const uint64_t* path_off, size_t n, size_t chunk) {
  uint64_t most = 0;
  chunk = std::max<size_t>(1, chunk);
  for (size_t c0 = 0; path_off && c0 < n; c0 += chunk) most = std::max(most, path_off[std::min(n, c0 + chunk)] - path_off[c0]);
  return most;
}

// ---- the write groups ---------------------------------------------------------------------------------------------------------------------
// The matched requests (status[i] == `match`) grouped by slot file, files in ascending (dataset that names the file, slot) order, each
// file's requests in ascending block: the writer opens every file once, writes it front to back and syncs it once.
struct RepairManyFile {
  size_t ds = 0;                                      // repair_many_file_of of its requests' datasets
  uint64_t slot = 0;
  std::string name;
  std::vector<size_t> reqs;                           // request indices, ascending block
};
inline std::vector<RepairManyFile> repair_many_write_groups(const std::vector<ReadDataset>& ds, const uint64_t* req, const uint32_t* status, size_t n,
                                                            uint32_t match) {
  const std::vector<size_t> file_of = repair_many_file_of(ds);
  std::vector<size_t> order;
  for (size_t i = 0; i < n; ++i)
    if (status[i] == match && ds[req[3 * i]].from_file) order.push_back(i);
  auto key = [&](size_t i) { return std::make_tuple(file_of[req[3 * i]], req[3 * i + 1], req[3 * i + 2]); };
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return key(x) < key(y); });
  std::vector<RepairManyFile> g;
  for (size_t i : order) {
    const size_t f = file_of[req[3 * i]];
    if (g.empty() || g.back().ds != f || g.back().slot != req[3 * i + 1]) {
      g.emplace_back();
      g.back().ds = f;
      g.back().slot = req[3 * i + 1];
      g.back().name = fill_slot_file_name(ds[f].base, req[3 * i + 1]);
    }
    g.back().reqs.push_back(i);
  }
  return g;
}

// ---- the writer ---------------------------------------------------------------------------------------------------------------------------
// A function of (file name, rows): file j receives its rows -- block_size bytes each, at their byte offsets, in the order given -- through
// repair_write_file, one open, one fdatasync and one close a file, the files spread over `threads` threads in contiguous shares
// (on_threads: worker w takes files [count w / threads, count (w + 1) / threads)).  Every file is attempted on its own: what stopped file j
// (0: written and synced) and its stamps from before its first write and after its sync land in out[j], whatever became of its neighbours.
struct WriteRow {
  uint64_t off = 0;
  const uint8_t* p = nullptr;
};
struct WriteFile {
  std::string name;
  std::vector<WriteRow> rows;
};
struct WriteOutcome {
  int what = 0;                                       // repair_write_file's
  int worker = 0;
  uint64_t before[2] = {~0ULL, ~0ULL}, after[2] = {~0ULL, ~0ULL};
};
inline std::vector<WriteOutcome> write_files_threaded(const std::vector<WriteFile>& files, size_t block_size, int threads) {
  std::vector<WriteOutcome> out(files.size());
  on_threads(threads, files.size(), [&](int w, size_t j) {
    const WriteFile& f = files[j];
    WriteOutcome& o = out[j];
    o.worker = w;
    (void)repair_stat_stamp(f.name, o.before);
    o.what = repair_write_file(f.name, block_size, f.rows.size(), [&](size_t q) { return f.rows[q].off; }, [&](size_t q) { return f.rows[q].p; });
    if (!o.what) (void)repair_stat_stamp(f.name, o.after);
    return true;
  });
  return out;
}

// What the call makes of the outcomes.  The matched requests of a file that failed become `unwritten`; *n_written counts the blocks of the
// files written and synced; written[k] collects, for every listed dataset k, the stamps of the files written that hold a request naming
// ds[k]'s handle (what repair_restamp_caches takes for cache_paths[k]).  Returns the index of the failing file that comes first in
// (dataset, slot) order -- the groups' own order -- or files.size() when none failed.
inline size_t repair_many_settle(const std::vector<ReadDataset>& ds, const uint64_t* req, const std::vector<RepairManyFile>& files,
                                 const std::vector<WriteOutcome>& out, uint32_t unwritten, uint32_t* status, size_t* n_written,
                                 std::vector<std::vector<FileStamp>>* written) {
  size_t first_bad = files.size();
  written->assign(ds.size(), {});
  std::vector<std::vector<size_t>> listed(ds.size());  // the indices that list each handle
  for (size_t k = 0; k < ds.size(); ++k) listed[ds[k].same_as].push_back(k);
  for (size_t j = 0; j < files.size(); ++j) {
    if (out[j].what) {
      first_bad = std::min(first_bad, j);
      for (size_t i : files[j].reqs) status[i] = unwritten;
      continue;
    }
    *n_written += files[j].reqs.size();
    FileStamp st;
    st.slot = files[j].slot;
    for (int h = 0; h < 2; ++h) { st.before[h] = out[j].before[h]; st.after[h] = out[j].after[h]; }
    std::vector<size_t> handles;
    for (size_t i : files[j].reqs) handles.push_back(ds[req[3 * i]].same_as);
    std::sort(handles.begin(), handles.end());
    handles.erase(std::unique(handles.begin(), handles.end()), handles.end());
    for (size_t h : handles)
      for (size_t k : listed[h]) (*written)[k].push_back(st);
  }
  return first_bad;
}

}  // namespace cp2i
