// Block multiproofs behind the C ABI (include/codex_p2.h): cp2_block_multiproof_rows, cp2_block_multiproof_layout,
// cp2_dataset_block_multiproofs and cp2_blocks_verify_multi, and the pass cp2_fill_add_multi (fill.cpp) shares with the last.
//
// The single proofs of block_proofs.cpp carry one whole path per block; two blocks of one slot share every node above the point where
// their paths meet, and that node is sent, uploaded and hashed once per block.  A multiproof of a set of blocks of one slot holds each
// node that cannot be computed from the set and from the other rows once (multiproof_plan.hpp: the layout), and checking hashes each
// inner node of the induced subtree once.  A dataset SERVES the rows with the gather block proofs use; a node that holds nothing but
// slot roots CHECKS groups of blocks against them: the candidates go down repair's data path (repair_check_with, repair.cpp), their block
// roots land in a work table beside the sent rows, and k_multiproof_layer builds every group's subtree level by level, one launch per
// level, one verdict per group.  A fill session that keeps nodes runs the same pass with groups that stop at the nodes it holds
// (cp2_fill_add_multi_anchored, fill.cpp; multiproof_anchor_plan.hpp): the kept inputs are gathered into the work table first and the
// verdicts come from every group's tops (k_multiproof_tops, k_multiproof_fold).  cp2_dataset_block_tree_rows serves the rows such a
// session asks for, by their place in the tree.
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
#include "multiproof_anchor_plan.hpp"
#include "multiproof_plan.hpp"
#include "repair.hpp"

using namespace cp2i;

static_assert(sizeof(MultiproofJob) == 16 && sizeof(cp2k::MultiproofJob) == 16 && MULTIPROOF_ZERO == cp2k::MULTIPROOF_ZERO,
              "the plan's jobs are uploaded as the kernel's");
static_assert(sizeof(cp2k::MultiproofTop) == 8, "the tops go up as (row, group) pairs of 32-bit words");

namespace {

size_t blocks_of(size_t cell_size, size_t block_size, size_t n_cells) { return n_cells / (block_size / cell_size); }

}  // namespace

// Groups of candidates judged against stated roots in device memory (want[g]: the absolute device address of group g's root): the n
// candidates go down repair's data path, unchanged; its `verdicts` step only copies each chunk's fresh block roots into rows [c0, c0 + m)
// of the work table (device to device, on the chunk's stream) and writes a provisional verdict, so a group that straddles two chunks needs
// nothing special.  The sent rows and the job tables go up once, before the first chunk.  After the pass k_multiproof_layer runs level by
// level, then `commit` (may be empty: what a fill keeps), then one download of the n_groups verdicts (and the n block roots) and one drain.
int cp2i::multiproof_check(cp2_ctx* ctx, size_t cell_size, size_t block_size, const MultiproofPlan& plan, const uint64_t* want, size_t n_groups,
                           const uint8_t* data, const uint8_t* nodes, const MultiproofCommit& commit, uint32_t* group_verdict, uint8_t* block_roots,
                           const MultiproofAnchors* anchors) {
  const size_t n = plan.n, n_rows = plan.n_rows;
  // with anchors the stated addresses are per top, and the tops' tables go up beside the jobs
  const size_t n_want = anchors ? anchors->n_tops : n_groups, n_kept = anchors ? anchors->n_kept : 0;
  DevBuf d_work, d_jobs, d_want, d_group_verdict, d_kept_addr, d_tops, d_top_off, d_top_verdict;   // (go after the streams have drained: DevBuf::release)
  RepairJudge judge;
  judge.begin = [&](size_t) -> int {
    CP2_TRY(d_work.scratch(ctx, plan.n_work * 32));
    CP2_TRY(d_jobs.scratch(ctx, plan.jobs.size() * sizeof(MultiproofJob)));
    CP2_TRY(d_want.scratch(ctx, n_want * 8));
    CP2_TRY(d_group_verdict.scratch(ctx, n_groups * 4));
    if (n_rows) CP2_HIP(ctx, hipMemcpyAsync(d_work.u8() + n * 32, nodes, n_rows * 32, hipMemcpyHostToDevice, ctx->stream));
    if (!plan.jobs.empty())                          // (a group whose tops are all block roots has none)
      CP2_HIP(ctx, hipMemcpyAsync(d_jobs.p, plan.jobs.data(), plan.jobs.size() * sizeof(MultiproofJob), hipMemcpyHostToDevice, ctx->stream));
    CP2_HIP(ctx, hipMemcpyAsync(d_want.p, anchors ? anchors->top_want : want, n_want * 8, hipMemcpyHostToDevice, ctx->stream));
    if (!anchors) return CP2_OK;
    CP2_TRY(d_tops.scratch(ctx, anchors->n_tops * sizeof(cp2k::MultiproofTop)));
    CP2_TRY(d_top_off.scratch(ctx, (n_groups + 1) * 8));
    CP2_TRY(d_top_verdict.scratch(ctx, anchors->n_tops * 4));
    CP2_HIP(ctx, hipMemcpyAsync(d_tops.p, anchors->top_row_group, anchors->n_tops * sizeof(cp2k::MultiproofTop), hipMemcpyHostToDevice, ctx->stream));
    CP2_HIP(ctx, hipMemcpyAsync(d_top_off.p, anchors->top_off, (n_groups + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n_kept) {                                    // the kept inputs, once: rows [n + n_rows, n + n_rows + n_kept) of the work table
      CP2_TRY(d_kept_addr.scratch(ctx, n_kept * 8));
      CP2_HIP(ctx, hipMemcpyAsync(d_kept_addr.p, anchors->kept_addr, n_kept * 8, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, cp2k::launch_gather_addr(static_cast<const uint64_t*>(d_kept_addr.p), n_kept, 32, d_work.u8() + (n + n_rows) * 32, ctx->stream));
    }
    return CP2_OK;
  };
  judge.verdicts = [&](const uint8_t* fresh, size_t c0, size_t m, uint32_t* verdict, hipStream_t st) -> int {
    CP2_HIP(ctx, hipMemcpyAsync(d_work.u8() + c0 * 32, fresh, m * 32, hipMemcpyDeviceToDevice, st));
    CP2_HIP(ctx, hipMemsetAsync(verdict, 0, m * 4, st));
    return CP2_OK;
  };
  std::vector<uint32_t> provisional(n);
  CP2_TRY(repair_check_with(ctx, cell_size, block_size, data, n, provisional.data(), judge));
  uint32_t* d_verdict = static_cast<uint32_t*>(d_group_verdict.p);
  CP2_HIP(ctx, cp2k::launch_multiproof_layers(d_work.p, plan.n_work, static_cast<const cp2k::MultiproofJob*>(d_jobs.p), plan.level_off.data(),
                                              plan.level_base.data(), plan.levels(), static_cast<const uint64_t*>(d_want.p), d_verdict, ctx->stream));
  if (anchors)
    CP2_HIP(ctx, cp2k::launch_multiproof_tops(d_work.p, plan.n_work, static_cast<const cp2k::MultiproofTop*>(d_tops.p),
                                              static_cast<const uint64_t*>(d_want.p), anchors->n_tops, anchors->top_off,
                                              static_cast<const uint64_t*>(d_top_off.p), n_groups, static_cast<uint32_t*>(d_top_verdict.p), d_verdict,
                                              ctx->stream));
  if (commit) CP2_TRY(commit(d_work.p, d_verdict, ctx->stream));
  CP2_HIP(ctx, hipMemcpyAsync(group_verdict, d_verdict, n_groups * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (block_roots) CP2_HIP(ctx, hipMemcpyAsync(block_roots, d_work.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "multiproof: the check failed on the device";
    return CP2_ERR_HIP;
  }
  return CP2_OK;
}

extern "C" size_t cp2_block_multiproof_rows(size_t cell_size, size_t block_size, size_t n_cells, const uint64_t* blocks, size_t k) try {
  if (trees_check_geometry(cell_size, block_size, n_cells, 1) != CP2_OK) return SIZE_MAX;
  const uint64_t n_blocks = blocks_of(cell_size, block_size, n_cells);
  if (!multiproof_list_ok(n_blocks, blocks, k)) return SIZE_MAX;
  return multiproof_layout(n_blocks, blocks, k, nullptr);
} catch (...) {
  return SIZE_MAX;   // nothing may unwind across the C ABI
}

extern "C" int cp2_block_multiproof_layout(size_t cell_size, size_t block_size, size_t n_cells, const uint64_t* blocks, size_t k,
                                           uint64_t* level_index) try {
  if (trees_check_geometry(cell_size, block_size, n_cells, 1) != CP2_OK) return CP2_ERR_INVALID;
  const uint64_t n_blocks = blocks_of(cell_size, block_size, n_cells);
  if (!multiproof_list_ok(n_blocks, blocks, k)) return CP2_ERR_INVALID;
  std::vector<uint64_t> li;
  multiproof_layout(n_blocks, blocks, k, &li);
  if (!li.empty() && !level_index) return CP2_ERR_INVALID;
  if (!li.empty()) std::memcpy(level_index, li.data(), li.size() * 8);
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_dataset_block_multiproofs(cp2_dataset* ds, const uint64_t* groups, size_t n_groups, const uint64_t* blocks, uint8_t* block_roots,
                                             uint8_t* nodes, size_t cap, size_t* n_rows) try {
  if (!ds) return CP2_ERR_INVALID;
  cp2_ctx* ctx = ds->ctx;
  const cp2_config& c = ds->cfg;
  size_t n = 0;
  if (!n_rows || (n_groups && !groups) || !multiproof_count(groups, n_groups, &n) || (n && !blocks)) {
    ctx->err = "block multiproofs: groups, blocks and n_rows must not be NULL when there are requests";
    return CP2_ERR_INVALID;
  }
  if (repair_dataset_mode(ds) == 0) {
    ctx->err = "block multiproofs: this dataset keeps only its slot roots, no block roots and no layers above them to take a proof from: build it with "
               "every node or the compact layers kept (cp2_set_keep_trees)";
    return CP2_ERR_INVALID;
  }
  const uint64_t n_blocks = blocks_of(c.cell_size, c.block_size, c.n_cells);
  std::string err;
  uint64_t rows_needed = 0;
  if (!multiproof_validate("block multiproofs", "slot", groups, n_groups, blocks, ds->first_slot, ds->n_local, n_blocks, false, 0, &rows_needed, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  *n_rows = (size_t)rows_needed;
  if (rows_needed > cap || (rows_needed && !nodes)) {
    ctx->err = "block multiproofs: the groups' layouts hold " + std::to_string(rows_needed) + " rows, nodes has room for " + std::to_string(nodes ? cap : 0);
    return CP2_ERR_INVALID;
  }
  if (n_groups == 0) return CP2_OK;
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const size_t depth = block_proof_depth(n_blocks), per = depth + 1;
  const std::vector<size_t>& offs = ds->trees ? ds->trees->toff : ds->coff;
  const std::vector<size_t>& sizes = ds->trees ? ds->trees->tsizes : ds->csizes;
  if (offs.size() != per || sizes.size() != per || (ds->trees && ds->trees->units_per_slot != 1)) {
    ctx->err = "block multiproofs: the kept layers of this dataset are not those of whole slot trees";
    return CP2_ERR_INVALID;
  }
  // the rows of the call: every group's sent rows in packed order, then (when asked for) the block root of every request
  const RepairKept k = repair_dataset_kept(ds);
  const uint64_t base = (uint64_t)reinterpret_cast<uintptr_t>(k.nodes);
  std::vector<uint64_t> addr, li;
  addr.reserve((size_t)rows_needed + (block_roots ? n : 0));
  size_t at = 0;
  for (size_t g = 0; g < n_groups; ++g) {
    const uint64_t local = groups[2 * g] - ds->first_slot;
    li.clear();
    multiproof_layout(n_blocks, blocks + at, (size_t)groups[2 * g + 1], &li);
    for (size_t r = 0; r < li.size() / 2; ++r) addr.push_back(offs[li[2 * r]] + local * sizes[li[2 * r]] + li[2 * r + 1]);
    at += (size_t)groups[2 * g + 1];
  }
  if (block_roots) {
    at = 0;
    for (size_t g = 0; g < n_groups; ++g)
      for (uint64_t j = 0; j < groups[2 * g + 1]; ++j, ++at) addr.push_back(repair_dataset_row(ds, groups[2 * g], blocks[at]));
  }
  for (uint64_t& r : addr) {
    if (r >= k.rows) {
      ctx->err = "block multiproofs: a row lies outside the kept nodes";
      return CP2_ERR_INVALID;
    }
    r = base + r * 32;
  }
  std::vector<uint8_t> out(addr.size() * 32);
  CP2_TRY(gather_rows_by_addr(ctx, addr, out.data()));
  if (rows_needed) std::memcpy(nodes, out.data(), (size_t)rows_needed * 32);
  if (block_roots) std::memcpy(block_roots, out.data() + (size_t)rows_needed * 32, n * 32);
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// Tree rows by their place (the rows a fill session's want list names: cp2_fill_multiproof_want, fill.cpp), from every node kept or the
// compact layers, with the row arithmetic block proofs use; one upload of the address list, one gather, one download.
extern "C" int cp2_dataset_block_tree_rows(cp2_dataset* ds, const uint64_t* places, size_t n, uint8_t* rows) try {
  if (!ds) return CP2_ERR_INVALID;
  cp2_ctx* ctx = ds->ctx;
  const cp2_config& c = ds->cfg;
  if (n && (!places || !rows)) {
    ctx->err = "block tree rows: places and rows must not be NULL when n > 0";
    return CP2_ERR_INVALID;
  }
  if (repair_dataset_mode(ds) == 0) {
    ctx->err = "block tree rows: this dataset keeps only its slot roots, no block roots and no layers above them to take a row from: build it with "
               "every node or the compact layers kept (cp2_set_keep_trees)";
    return CP2_ERR_INVALID;
  }
  const uint64_t n_blocks = blocks_of(c.cell_size, c.block_size, c.n_cells);
  const size_t per = block_proof_depth(n_blocks) + 1;
  const std::vector<size_t>& offs = ds->trees ? ds->trees->toff : ds->coff;
  const std::vector<size_t>& sizes = ds->trees ? ds->trees->tsizes : ds->csizes;
  if (offs.size() != per || sizes.size() != per || (ds->trees && ds->trees->units_per_slot != 1)) {
    ctx->err = "block tree rows: the kept layers of this dataset are not those of whole slot trees";
    return CP2_ERR_INVALID;
  }
  std::string err;
  if (!tree_places_validate("block tree rows", places, n, ds->first_slot, ds->n_local, sizes, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n == 0) return CP2_OK;
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const RepairKept k = repair_dataset_kept(ds);
  std::vector<uint64_t> addr(n);
  for (size_t i = 0; i < n; ++i) {
    const uint64_t l = places[3 * i + 1], r = offs[l] + (places[3 * i] - ds->first_slot) * sizes[l] + places[3 * i + 2];
    if (r >= k.rows) {
      ctx->err = "block tree rows: a row lies outside the kept nodes";
      return CP2_ERR_INVALID;
    }
    addr[i] = (uint64_t)reinterpret_cast<uintptr_t>(k.nodes) + r * 32;
  }
  std::vector<uint8_t> out(n * 32);
  CP2_TRY(gather_rows_by_addr(ctx, addr, out.data()));
  std::memcpy(rows, out.data(), n * 32);
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_blocks_verify_multi(cp2_ctx* ctx, size_t cell_size, size_t block_size, size_t n_cells, const uint8_t* slot_roots, size_t n_roots,
                                       const uint64_t* groups, size_t n_groups, const uint64_t* blocks, const uint8_t* data, const uint8_t* nodes,
                                       size_t n_rows, uint32_t* status, uint8_t* block_roots) try {
  if (!ctx) return CP2_ERR_INVALID;
  if (trees_check_geometry(cell_size, block_size, n_cells, 1) != CP2_OK) {
    ctx->err = "block verify multi: cell_size " + std::to_string(cell_size) + ", block_size " + std::to_string(block_size) + ", n_cells " +
               std::to_string(n_cells) + " is a geometry the tree builders refuse";
    return CP2_ERR_INVALID;
  }
  size_t n = 0;
  if ((n_groups && (!groups || !status)) || !multiproof_count(groups, n_groups, &n) || (n && (!slot_roots || !blocks || !data)) || (n_rows && !nodes)) {
    ctx->err = "block verify multi: slot_roots, groups, blocks, data and status must not be NULL when there are requests, nor nodes when n_rows > 0";
    return CP2_ERR_INVALID;
  }
  const uint64_t n_blocks = blocks_of(cell_size, block_size, n_cells);
  std::string err;
  if (!multiproof_validate("block verify multi", "root index", groups, n_groups, blocks, 0, n_roots, n_blocks, true, n_rows, nullptr, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n_groups == 0) return CP2_OK;
  std::vector<uint64_t> counts(n_groups), nb(n_groups, n_blocks);
  for (size_t g = 0; g < n_groups; ++g) counts[g] = groups[2 * g + 1];
  MultiproofPlan plan;
  if (!multiproof_plan(counts.data(), nb.data(), n_groups, blocks, &plan, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  DevBuf d_roots;                                    // the slot roots once per call
  CP2_TRY(d_roots.scratch(ctx, n_roots * 32));
  CP2_HIP(ctx, hipMemcpyAsync(d_roots.p, slot_roots, n_roots * 32, hipMemcpyHostToDevice, ctx->stream));
  std::vector<uint64_t> want(n_groups);
  for (size_t g = 0; g < n_groups; ++g) want[g] = (uint64_t)reinterpret_cast<uintptr_t>(d_roots.p) + groups[2 * g] * 32;
  std::vector<uint32_t> v(n_groups);
  std::vector<uint8_t> roots(block_roots ? n * 32 : 0);
  CP2_TRY(multiproof_check(ctx, cell_size, block_size, plan, want.data(), n_groups, data, nodes, nullptr, v.data(), block_roots ? roots.data() : nullptr));
  size_t matched = 0;
  for (size_t g = 0; g < n_groups; ++g) {
    status[g] = v[g] == 0 ? CP2_BLOCK_MATCH : CP2_BLOCK_MISMATCH;
    matched += v[g] == 0;
  }
  if (block_roots) std::memcpy(block_roots, roots.data(), n * 32);
  if (std::getenv("CP2_TRACE")) {
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), bytes = (double)n * (double)block_size;
    const size_t whole = n * block_proof_depth(n_blocks);
    std::fprintf(stderr, "[cp2 trace] block verify multi: %zu group(s), %zu request(s), %zu group(s) matched, %zu rows received against %zu, %zu "
                 "compressions against %zu, %.0f bytes, %.3f s (%.2f GB/s)\n", n_groups, n, matched, n_rows, whole, plan.computed(), whole, bytes, seconds,
                 seconds > 0 ? bytes / seconds / 1e9 : 0.0);
  }
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
