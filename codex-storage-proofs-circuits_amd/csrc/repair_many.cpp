// cp2_datasets_repair_blocks_many behind the C ABI (include/codex_p2.h): replacement blocks of many datasets judged in one pass, then
// written back on the context's ingestion threads.
//
// After a scrub or a verified read-back has named the damaged blocks of many datasets, the replacements went in one dataset per call:
// a data-path set-up, launches that last a wave's lifetime whatever their size, a drain and serial file writes for a few blocks each.
// Nothing in the device work needs a chunk's blocks to belong to one dataset: k_hash_cells and the block-tree layers see block bytes
// only, and the last step is per lane.  So this call is ONE repair_check_with pass (repair.cpp) over all n candidates: begin uploads the
// descriptor table, stage the chunk's contiguous range of the packed paths, and the verdicts come from k_repair_judge_many, which walks
// each request's 0 or depth levels and compares with a row at an absolute address -- the kept block root (cp2_dataset_repair_blocks'
// rule) or the dataset's own slot root (cp2_dataset_repair_blocks_proved's).  What the plan decides -- refusals, chunks, descriptors, write
// groups by file name, the writer -- is repair_many_plan.hpp; the stamps and the restamp rule are repair's own (repair_stat_stamp,
// repair_write_file, repair_restamp_caches).  Unlike the single call the writer attempts every file: a file that fails leaves only its own
// requests unwritten.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "dataset_obj.hpp"
#include "repair.hpp"
#include "repair_many_plan.hpp"

using namespace cp2i;

static_assert(REPAIR_MANY_CHECK_ONLY == CP2_REPAIR_CHECK_ONLY, "the plan's flag is the boundary's");
static_assert(sizeof(RepairManyDesc) == sizeof(cp2k::RepairManyReq) && offsetof(RepairManyDesc, want) == offsetof(cp2k::RepairManyReq, want) &&
              offsetof(RepairManyDesc, blk) == offsetof(cp2k::RepairManyReq, blk) &&
              offsetof(RepairManyDesc, n_blocks) == offsetof(cp2k::RepairManyReq, n_blocks) &&
              offsetof(RepairManyDesc, path_at) == offsetof(cp2k::RepairManyReq, path_at) &&
              offsetof(RepairManyDesc, len) == offsetof(cp2k::RepairManyReq, len), "repair_many_plan.hpp restates the kernel's request descriptor");

namespace {

// read_blocks.cpp's description of a listed dataset, for every residency: a roots-only dataset has its slot roots and no kept layers
// (`first` maps a handle to the lowest index that lists it: linear in the datasets, where read_blocks.cpp scans)
ReadDataset describe(const cp2_ctx* ctx, cp2_dataset* const* ds, size_t k, std::unordered_map<const cp2_dataset*, size_t>* first) {
  ReadDataset d;
  const cp2_dataset* p = ds[k];
  d.same_as = k;
  if (!p) { d.null = true; return d; }
  d.same_as = first->emplace(p, k).first->second;
  d.foreign = p->ctx != ctx;
  d.cell_size = p->cfg.cell_size;
  d.block_size = p->cfg.block_size;
  d.n_cells = p->cfg.n_cells;
  d.first_slot = p->first_slot;
  d.n_local = p->n_local;
  d.mode = repair_dataset_mode(p);
  d.from_file = p->from_file;
  d.base = p->file_base;
  d.seed = p->cfg.seed;
  if (d.foreign) return d;
  d.roots = (uint64_t)reinterpret_cast<uintptr_t>(dataset_roots_dev(p));
  if (d.mode == 0) return d;
  d.nodes = (uint64_t)reinterpret_cast<uintptr_t>(repair_dataset_kept(p).nodes);
  if (const cp2_slot_trees* t = p->trees) {
    d.whole = t->units_per_slot == 1;
    d.root_off = t->boff.back();
    d.root_size = t->bsizes.back();
    d.offs.assign(t->toff.begin(), t->toff.end());
    d.sizes.assign(t->tsizes.begin(), t->tsizes.end());
  } else {
    d.whole = true;
    d.root_off = p->coff.empty() ? 0 : p->coff[0];
    d.root_size = p->csizes.empty() ? 0 : p->csizes[0];
    d.offs.assign(p->coff.begin(), p->coff.end());
    d.sizes.assign(p->csizes.begin(), p->csizes.end());
  }
  return d;
}

}  // namespace

extern "C" int cp2_datasets_repair_blocks_many(cp2_ctx* ctx, cp2_dataset* const* ds, size_t n_ds, const uint64_t* req, const uint8_t* data,
                                               const uint8_t* paths, const uint64_t* path_off, size_t n, int flags, const char* const* cache_paths,
                                               uint32_t* status, size_t* n_written) try {
  if (!ctx) return CP2_ERR_INVALID;
  RepairManyArgs a;
  a.ds = ds != nullptr; a.req = req != nullptr; a.data = data != nullptr; a.status = status != nullptr;
  a.paths = paths != nullptr; a.path_off = path_off != nullptr;
  a.n_ds = n_ds; a.n = n; a.flags = flags;
  std::vector<ReadDataset> sets;
  std::unordered_map<const cp2_dataset*, size_t> first;
  if (ds && n) {
    sets.reserve(n_ds);
    first.reserve(n_ds);
    for (size_t k = 0; k < n_ds; ++k) sets.push_back(describe(ctx, ds, k, &first));
  }
  std::string err;
  if (!repair_many_validate(a, sets, req, path_off, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n == 0) {
    if (n_written) *n_written = 0;
    return CP2_OK;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  const size_t cs = sets[0].cell_size, bs = sets[0].block_size;
  const size_t chunk = read_blocks_chunk(ctx->stage_bytes, bs, n);
  const std::vector<RepairManyDesc> table = repair_many_table(sets, req, path_off, n, chunk);
  const uint64_t most = repair_many_most_path_rows(path_off, n, chunk);

  // ---- the pass: repair's, once over all n rows of `data` ------------------------------------------------------------------------------------
  DevBuf d_tab, d_paths;                               // (go after the streams have drained: DevBuf::release)
  RepairJudge judge;
  judge.begin = [&](size_t) -> int {
    CP2_TRY(d_tab.scratch(ctx, n * sizeof(RepairManyDesc)));
    CP2_HIP(ctx, hipMemcpyAsync(d_tab.p, table.data(), n * sizeof(RepairManyDesc), hipMemcpyHostToDevice, ctx->stream));
    if (most) CP2_TRY(d_paths.scratch(ctx, (size_t)most * 32));
    return CP2_OK;
  };
  // the chunk's paths travel with the chunk (the previous chunk's walk, earlier on this stream, has read its own)
  judge.stage = [&](size_t c0, size_t m, hipStream_t st) -> int {
    const size_t rows = path_off ? (size_t)(path_off[c0 + m] - path_off[c0]) : 0;
    if (rows) CP2_HIP(ctx, hipMemcpyAsync(d_paths.p, paths + (size_t)path_off[c0] * 32, rows * 32, hipMemcpyHostToDevice, st));
    return CP2_OK;
  };
  judge.verdicts = [&](const uint8_t* fresh, size_t c0, size_t m, uint32_t* verdict, hipStream_t st) -> int {
    CP2_HIP(ctx, cp2k::launch_repair_judge_many(fresh, d_paths.p, static_cast<const cp2k::RepairManyReq*>(d_tab.p) + c0, m, verdict, st));
    return CP2_OK;
  };
  std::vector<uint32_t> st(n);
  CP2_TRY(repair_check_with(ctx, cs, bs, data, n, st.data(), judge));

  // ---- the writer: every matched block into its slot file, the files spread over the ingestion threads; then the stamps ----------------------
  size_t written_n = 0, restamped = 0, n_files = 0, with_paths = 0, matched = 0;
  for (size_t i = 0; i < n; ++i) {
    with_paths += table[i].len != 0;
    matched += st[i] == CP2_REPAIR_MATCH;
  }
  int r = CP2_OK;
  if (!(flags & CP2_REPAIR_CHECK_ONLY)) {
    const std::vector<RepairManyFile> groups = repair_many_write_groups(sets, req, st.data(), n, CP2_REPAIR_MATCH);
    std::vector<WriteFile> files(groups.size());
    for (size_t j = 0; j < groups.size(); ++j) {
      files[j].name = groups[j].name;
      for (size_t i : groups[j].reqs) files[j].rows.push_back({req[3 * i + 2] * (uint64_t)bs, data + i * bs});
    }
    n_files = files.size();
    const std::vector<WriteOutcome> out = write_files_threaded(files, bs, fill_threads(ctx));
    std::vector<std::vector<FileStamp>> written;
    const size_t bad = repair_many_settle(sets, req, groups, out, CP2_REPAIR_UNWRITTEN, st.data(), &written_n, &written);
    if (bad < groups.size()) {
      r = CP2_ERR_IO;
      err = "cannot write " + groups[bad].name + ": " + repair_write_reason(out[bad].what);
    }
    for (size_t k = 0; cache_paths && k < n_ds; ++k) {   // (after a failed file too: the other files are written and synced)
      if (!cache_paths[k] || written[k].empty()) continue;
      const cp2_dataset* p = ds[k];
      std::string rerr;
      const int rs = repair_restamp_caches({std::string(cache_paths[k]), std::string(cache_paths[k]) + ".kept"}, p->cfg, p->n_local, p->cfg.n_cells,
                                           p->first_slot, 1, p->file_base, written[k], &restamped, &rerr);
      if (r == CP2_OK && rs != CP2_OK) { r = rs; err = rerr; }
    }
  }
  std::copy(st.begin(), st.end(), status);
  if (n_written) *n_written = written_n;
  if (r != CP2_OK) ctx->err = err;
  if (std::getenv("CP2_TRACE")) {
    const double bytes = (double)n * (double)bs, seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "[cp2 trace] repair many: %zu dataset(s), %zu request(s), %zu chunk(s), %zu with paths, %zu matched, %zu written, %zu file(s), %.0f bytes, "
                 "%.3f s (%.2f GB/s), %zu stamp(s) restamped\n", n_ds, n, (n + chunk - 1) / chunk, with_paths, matched, written_n, n_files, bytes, seconds,
                 seconds > 0 ? bytes / seconds / 1e9 : 0.0, restamped);
  }
  return r;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
