// Listed blocks read back verified, with their proofs, behind the C ABI: cp2_datasets_read_blocks and cp2_dataset_read_blocks
// (include/codex_p2.h).
//
// A node that answers a peer, or spot-checks what it stores, names blocks of the slots it holds: (dataset, slot, block).  Each block is
// read from its slot file into the row of its request (the caller's `data`, or a pooled pinned chunk buffer when the call only checks),
// uploaded from there, hashed and reduced to its block root on repair's data path (repair_check_with, repair.cpp) and compared with the
// block root the dataset keeps for it by k_repair_compare_addr -- one absolute address per request, so the requests of many datasets
// share every launch.  The kept roots and the paths above them do not depend on what was read: one k_gather_addr and one download per
// call fetch them all.  What the plan decides -- refusals, read order, chunks, packed path offsets, the address tables -- is
// read_blocks_plan.hpp.  Chunk k + 1 is read on the context's ingestion threads while chunk k is uploaded and hashed: the pass itself is
// read_pass.hpp, which cp2_fills_resume_many runs with another judge.
//
// Where the time goes on the device: 1119 permutations per block in k_hash_cells and the block-tree layers, as in every other pass over
// block bytes.  The compare and the gather are what this file adds there, a few bytes per block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "dataset_obj.hpp"
#include "read_blocks_plan.hpp"
#include "read_pass.hpp"
#include "repair.hpp"

using namespace cp2i;

static_assert(READ_BLOCKS_CHECK_ONLY == CP2_READ_CHECK_ONLY, "the plan's flag is the boundary's");
static_assert(CP2_READ_OK == CP2_REPAIR_MATCH && CP2_READ_DAMAGED == CP2_REPAIR_MISMATCH, "repair_check_with's verdicts are the statuses");

namespace {

ReadDataset describe(const cp2_ctx* ctx, cp2_dataset* const* ds, size_t k) {
  ReadDataset d;
  const cp2_dataset* p = ds[k];
  d.same_as = k;
  if (!p) { d.null = true; return d; }
  for (size_t j = 0; j < k; ++j)
    if (ds[j] == p) { d.same_as = j; break; }
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
  if (d.mode == 0 || d.foreign) return d;
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

// the one implementation: outputs are written only when the whole call succeeded (data excepted: its rows are read into in place, and
// hold zeros wherever the call had written when it fails)
int read_blocks(cp2_ctx* ctx, cp2_dataset* const* ds, size_t n_ds, const uint64_t* req, size_t n, int flags, uint8_t* data, uint8_t* block_roots,
                uint8_t* paths, uint64_t* path_off, bool packed, uint32_t* status, size_t* n_ok) {
  ReadArgs a;
  a.ds = ds != nullptr; a.req = req != nullptr; a.data = data != nullptr; a.status = status != nullptr;
  a.paths = paths != nullptr;
  a.path_off = packed ? path_off != nullptr : a.paths;   // (the single form's layout needs no offsets)
  a.n_ds = n_ds; a.n = n; a.flags = flags;
  std::vector<ReadDataset> sets;
  if (ds && n)
    for (size_t k = 0; k < n_ds; ++k) sets.push_back(describe(ctx, ds, k));
  std::string err;
  if (!read_blocks_validate(a, sets, req, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n == 0) {
    if (n_ok) *n_ok = 0;
    return CP2_OK;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  const size_t cs = sets[0].cell_size, bs = sets[0].block_size;
  const size_t chunk = read_blocks_chunk(ctx->stage_bytes, bs, n);
  const ReadPlan plan = read_blocks_plan(sets, req, n, chunk);
  const std::vector<uint64_t> off = read_blocks_path_off(sets, req, n);
  const std::vector<uint64_t> addr = read_blocks_addr_table(sets, req, n, off);
  BlockSource src;
  src.n_chunks = plan.n_chunks();
  const int threads = fill_threads(ctx);
  src.read = [&](size_t k, const std::function<uint8_t*(size_t)>& row_of, std::string* e) {
    std::string bad;
    int eno = 0;
    if (read_blocks_read_chunk(plan, k, sets, req, bs, row_of, threads, &bad, &eno)) return true;
    *e = slot_file_error(bad, eno);
    return false;
  };
  bool any_fake = false;
  for (size_t i = 0; i < n; ++i) any_fake |= !sets[req[3 * i]].from_file;
  if (any_fake) {
    src.fake.resize(n);
    src.seeds.assign(n, 0);
    src.firsts.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
      const ReadDataset& d = sets[req[3 * i]];
      src.fake[i] = d.from_file ? 0 : 1;
      if (d.from_file) continue;
      src.seeds[i] = cp2_slot_seed(d.seed, req[3 * i + 1]);
      src.firsts[i] = req[3 * i + 2] * (bs / cs);
    }
  }
  std::vector<uint32_t> st(n);
  std::vector<uint8_t> gathered(addr.size() * 32);
  size_t touched = 0;
  const ReadJudge compare = [&](const uint8_t* fresh, const uint64_t* d_addr, size_t m, uint32_t* verdict, hipStream_t stream) {
    return cp2k::launch_repair_compare_addr(fresh, d_addr, m, verdict, stream);
  };
  const int r = read_pass(ctx, cs, bs, n, chunk, addr, src, compare, data, gathered.data(), st.data(), &touched);
  if (r != CP2_OK) {
    if (data) std::memset(data, 0, touched * bs);
    return r;
  }
  size_t ok = 0;
  for (size_t i = 0; i < n; ++i) {
    status[i] = st[i];
    if (st[i] == CP2_READ_OK) ++ok;
    else if (data) std::memset(data + i * bs, 0, bs);   // no byte that failed its check is left in an output
  }
  if (block_roots) std::memcpy(block_roots, gathered.data(), n * 32);
  if (paths) std::memcpy(paths, gathered.data() + n * 32, (size_t)off[n] * 32);
  if (packed && path_off) std::copy(off.begin(), off.end(), path_off);
  if (n_ok) *n_ok = ok;
  if (std::getenv("CP2_TRACE")) {
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), bytes = (double)n * (double)bs;
    std::fprintf(stderr, "[cp2 trace] read blocks: %zu dataset(s), %zu request(s), %zu chunk(s), %.0f bytes, %.3f s (%.2f GB/s), %zu damaged\n", n_ds, n,
                 plan.n_chunks(), bytes, s, s > 0 ? bytes / s / 1e9 : 0.0, n - ok);
  }
  return CP2_OK;
}

}  // namespace

extern "C" int cp2_datasets_read_blocks(cp2_ctx* ctx, cp2_dataset* const* ds, size_t n_ds, const uint64_t* req, size_t n, int flags, uint8_t* data,
                                        uint8_t* block_roots, uint8_t* paths, uint64_t* path_off, uint32_t* status, size_t* n_ok) try {
  if (!ctx) return CP2_ERR_INVALID;
  return read_blocks(ctx, ds, n_ds, req, n, flags, data, block_roots, paths, path_off, true, status, n_ok);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_dataset_read_blocks(cp2_dataset* ds, const uint64_t* slot_block, size_t n, int flags, uint8_t* data, uint8_t* block_roots,
                                       uint8_t* paths, uint32_t* status, size_t* n_ok) try {
  if (!ds) return CP2_ERR_INVALID;
  // the many-dataset pass with one dataset, on the dataset's own context; one depth, so the packed paths ARE cp2_dataset_block_proofs' layout
  std::vector<uint64_t> req;
  if (slot_block) {
    req.resize(3 * n);
    for (size_t i = 0; i < n; ++i) {
      req[3 * i] = 0;
      req[3 * i + 1] = slot_block[2 * i];
      req[3 * i + 2] = slot_block[2 * i + 1];
    }
  }
  cp2_dataset* const one[1] = {ds};
  return read_blocks(ds->ctx, one, 1, slot_block ? req.data() : nullptr, n, flags, data, block_roots, paths, nullptr, false, status, n_ok);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
