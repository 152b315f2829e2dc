// cp2_datasets_set_roots_many behind the C ABI (include/codex_p2.h): the dataset trees of n datasets of one context in ONE pass.
//
// cp2_dataset_set_roots builds one tree of n_slots leaves with one k_compress_layer launch per level, the upper levels a lone wave each,
// and drains the stream: a storage node that holds one slot each of thousands of datasets pays about a dozen dependent launches and a
// drain per dataset for a few thousand compressions.  Across datasets those trees are independent.  Here the trees of a CHUNK of requests
// lie tree-major in one device buffer -- tree r owns cp2_merkle_total(n_slots) consecutive rows, its layers bottom first, which is what
// cp2_dataset::dlayers holds, so every dataset's slice of the one download is contiguous -- and one k_compress_layer_ragged launch per
// level serves all of them through the tables of set_roots_plan.hpp.  Per chunk: one upload (the tables and the roots the caller gave,
// through pinned staging), one device-to-device copy per tree that puts its leaves in place (from the upload, or from the dataset's own
// built roots where the caller gave none), the comparison of every request's own rows with its built roots (k_gather_addr, then
// k_repair_compare_addr: both through address tables), the level launches, one download.  The results wait in host staging until every
// chunk has passed; only then does any dataset change.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dataset_obj.hpp"
#include "kernels.hpp"
#include "set_roots_plan.hpp"
#include "trees.hpp"

using namespace cp2i;

namespace {

struct Lap {
  bool on = false;
  double up = 0, levels = 0, down = 0, commit = 0;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  // what has passed since the last call goes to *to; with tracing on the stream is drained first, so that the device's share is in it
  int add(cp2_ctx* ctx, double* to, bool drain) {
    if (on && drain) CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const auto now = std::chrono::steady_clock::now();
    *to += std::chrono::duration<double>(now - t).count();
    t = now;
    return CP2_OK;
  }
};

size_t up32(size_t b) { return (b + 31) & ~(size_t)31; }

// requests [0, n) of one chunk: staged[i] receives every layer of request i's tree, own[i] (own may be NULL) whether its own rows match
int run_chunk(cp2_ctx* ctx, cp2_dataset* const* ds, const uint8_t* const* roots, size_t n, std::vector<uint8_t>* staged, uint8_t* own,
              size_t* n_levels, Lap& lap) {
  std::vector<uint64_t> n_slots(n);
  size_t cmp = 0, given = 0;                                  // rows compared; rows the caller gave
  for (size_t i = 0; i < n; ++i) {
    n_slots[i] = ds[i]->cfg.n_slots;
    if (roots && roots[i]) { cmp += ds[i]->n_local; given += n_slots[i]; }
  }
  const SetRootsPlan plan = set_roots_plan(n_slots.data(), n);
  if (!set_roots_plan_ok(plan, plan.rows)) {
    ctx->err = "set roots many: the plan of a chunk does not hold (a dataset of more than 2^40 slots?)";
    return CP2_ERR_INVALID;
  }
  *n_levels = std::max(*n_levels, plan.n_levels());
  const size_t P = plan.prefix.size();
  // the upload: [tree_tab 2 n][prefix P][given-row addresses cmp][built-root addresses cmp] (64-bit), [tree_of P] (32-bit), [given roots]
  const size_t o_tab = 0, o_prefix = o_tab + up32(2 * n * 8), o_fresh = o_prefix + up32(P * 8), o_kept = o_fresh + up32(cmp * 8),
               o_tree = o_kept + up32(cmp * 8), o_roots = o_tree + up32(P * 4), up_bytes = o_roots + given * 32;
  PinBuf h_up, h_down;                                        // before the device scratch: they outlive its drain on every way out
  DevBuf d_up, d_trees, d_cmp, d_verdict;
  CP2_TRY(h_up.alloc(ctx, up_bytes));
  CP2_TRY(h_down.alloc(ctx, plan.rows * 32 + cmp * 4));
  CP2_TRY(d_up.scratch(ctx, up_bytes));
  CP2_TRY(d_trees.scratch(ctx, plan.rows * 32));
  CP2_TRY(d_cmp.scratch(ctx, std::max<size_t>(cmp, 1) * 32));
  CP2_TRY(d_verdict.scratch(ctx, std::max<size_t>(cmp, 1) * 4));
  std::memcpy(h_up.u8() + o_tab, plan.tree_tab.data(), 2 * n * 8);
  std::memcpy(h_up.u8() + o_prefix, plan.prefix.data(), P * 8);
  std::memcpy(h_up.u8() + o_tree, plan.tree_of.data(), P * 4);
  uint64_t* fresh = reinterpret_cast<uint64_t*>(h_up.u8() + o_fresh);
  uint64_t* kept = reinterpret_cast<uint64_t*>(h_up.u8() + o_kept);
  std::vector<size_t> src_row(n, 0), cmp_at(n, 0);            // request i's rows inside the given roots; its first compared row
  for (size_t i = 0, c = 0, g = 0; i < n; ++i) {
    if (!(roots && roots[i])) continue;
    const uint64_t mine = (uint64_t)reinterpret_cast<uintptr_t>(d_trees.u8()) + (plan.tree_tab[2 * i] + ds[i]->first_slot) * 32;
    const uint64_t built = (uint64_t)reinterpret_cast<uintptr_t>(dataset_roots_dev(ds[i]));
    cmp_at[i] = c;
    for (uint64_t l = 0; l < ds[i]->n_local; ++l, ++c) { fresh[c] = mine + l * 32; kept[c] = built + l * 32; }
    src_row[i] = g;
    g += n_slots[i];
  }
  on_threads(fill_threads(ctx), n, [&](int, size_t i) {
    if (roots && roots[i]) std::memcpy(h_up.u8() + o_roots + src_row[i] * 32, roots[i], n_slots[i] * 32);
    return true;
  });
  CP2_HIP(ctx, hipMemcpyAsync(d_up.p, h_up.p, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  for (size_t i = 0; i < n; ++i) {
    const void* from = roots && roots[i] ? static_cast<const void*>(d_up.u8() + o_roots + src_row[i] * 32) : dataset_roots_dev(ds[i]);
    CP2_HIP(ctx, hipMemcpyAsync(d_trees.u8() + plan.tree_tab[2 * i] * 32, from, n_slots[i] * 32, hipMemcpyDeviceToDevice, ctx->stream));
  }
  if (cmp) {
    CP2_HIP(ctx, cp2k::launch_gather_addr(reinterpret_cast<const uint64_t*>(d_up.u8() + o_fresh), cmp, 32, d_cmp.p, ctx->stream));
    CP2_HIP(ctx, cp2k::launch_repair_compare_addr(d_cmp.p, reinterpret_cast<const uint64_t*>(d_up.u8() + o_kept), cmp,
                                                  static_cast<uint32_t*>(d_verdict.p), ctx->stream));
  }
  CP2_TRY(lap.add(ctx, &lap.up, true));
  CP2_HIP(ctx, cp2k::launch_compress_layers_ragged(d_trees.p, reinterpret_cast<const uint64_t*>(d_up.u8() + o_tab),
                                                   reinterpret_cast<const uint64_t*>(d_up.u8() + o_prefix),
                                                   reinterpret_cast<const uint32_t*>(d_up.u8() + o_tree), plan.level_off.data(),
                                                   plan.level_cnt.data(), plan.level_work.data(), plan.n_levels(), ctx->stream));
  CP2_TRY(lap.add(ctx, &lap.levels, true));
  CP2_HIP(ctx, hipMemcpyAsync(h_down.p, d_trees.p, plan.rows * 32, hipMemcpyDeviceToHost, ctx->stream));
  if (cmp) CP2_HIP(ctx, hipMemcpyAsync(h_down.u8() + plan.rows * 32, d_verdict.p, cmp * 4, hipMemcpyDeviceToHost, ctx->stream));
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  CP2_TRY(lap.add(ctx, &lap.down, false));
  std::atomic<bool> short_of_memory{false};
  on_threads(fill_threads(ctx), n, [&](int, size_t i) {
    try {
      const uint8_t* mine = h_down.u8() + plan.tree_tab[2 * i] * 32;
      staged[i].assign(mine, mine + set_roots_total(n_slots[i]) * 32);
    } catch (...) {
      short_of_memory = true;
    }
    return true;
  });
  if (short_of_memory) {
    ctx->err = "set roots many: no host memory for the trees";
    return CP2_ERR_ALLOC;
  }
  if (own) {
    const uint32_t* verdict = reinterpret_cast<const uint32_t*>(h_down.u8() + plan.rows * 32);
    for (size_t i = 0; i < n; ++i) {
      own[i] = 1;
      if (roots && roots[i])
        for (uint64_t l = 0; l < ds[i]->n_local; ++l)
          if (verdict[cmp_at[i] + l]) own[i] = 0;
    }
  }
  return lap.add(ctx, &lap.commit, false);
}

int refuse(cp2_ctx* ctx, size_t i, const std::string& why) {
  ctx->err = "request " + std::to_string(i) + ": " + why;
  return CP2_ERR_INVALID;
}

}  // namespace

// The pass behind the entry point and behind prepare() of proof_many.cpp: requests already validated (every dataset of this context, none
// twice, roots given or every slot local).  All or nothing: a dataset changes only after every chunk has come back.
int cp2i::set_roots_pass(cp2_ctx* ctx, cp2_dataset* const* ds, const uint8_t* const* all_roots, size_t n, uint8_t* own) {
  if (n == 0) return CP2_OK;
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  Lap lap;
  lap.on = std::getenv("CP2_TRACE") != nullptr;
  std::vector<uint64_t> n_slots(n);
  for (size_t i = 0; i < n; ++i) n_slots[i] = ds[i]->cfg.n_slots;
  const std::vector<SetRootsChunk> chunks = set_roots_chunks(n_slots.data(), n, ctx->stage_bytes / 2);
  std::vector<std::vector<uint8_t>> staged(n);
  std::vector<std::vector<size_t>> sizes(n);
  std::vector<uint8_t> mine(own ? n : 0);
  size_t n_levels = 0;
  uint64_t rows = 0;
  for (const SetRootsChunk& c : chunks) {
    CP2_TRY(run_chunk(ctx, ds + c.first, all_roots ? all_roots + c.first : nullptr, c.count, &staged[c.first], own ? &mine[c.first] : nullptr,
                      &n_levels, lap));
    rows += c.rows;
  }
  for (size_t i = 0; i < n; ++i) sizes[i] = layer_sizes_of(n_slots[i]);
  for (size_t i = 0; i < n; ++i) {                             // nothing below can fail
    ds[i]->dsizes.swap(sizes[i]);
    ds[i]->dlayers.swap(staged[i]);
    ds[i]->have_roots = true;
  }
  if (own) std::memcpy(own, mine.data(), n);
  (void)lap.add(ctx, &lap.commit, false);
  if (lap.on)
    std::fprintf(stderr, "[cp2 trace] set roots many: %zu request(s) in %zu chunk(s), %llu tree rows, %zu level(s); upload %.3f s, levels %.3f s, download %.3f s, commit %.3f s\n",
                 n, chunks.size(), (unsigned long long)rows, n_levels, lap.up, lap.levels, lap.down, lap.commit);
  return CP2_OK;
}

extern "C" int cp2_datasets_set_roots_many(cp2_ctx* ctx, cp2_dataset* const* ds, const uint8_t* const* all_roots, size_t n, uint8_t* own) try {
  if (!ctx) return CP2_ERR_INVALID;
  if (n && !ds) {
    ctx->err = "set roots many: ds is NULL";
    return CP2_ERR_INVALID;
  }
  for (size_t i = 0; i < n; ++i) {
    const cp2_dataset* d = ds[i];
    if (!d) return refuse(ctx, i, "NULL dataset");
    if (d->ctx != ctx) return refuse(ctx, i, "its dataset belongs to another context");
    if (!(all_roots && all_roots[i]) && !(d->first_slot == 0 && d->n_local == d->cfg.n_slots))
      return refuse(ctx, i, "NULL roots for a dataset whose slots are not all local (slots " + std::to_string(d->first_slot) + " + " +
                                std::to_string(d->n_local) + " of " + std::to_string(d->cfg.n_slots) + ")");
  }
  std::vector<std::pair<const cp2_dataset*, size_t>> seen(n);
  for (size_t i = 0; i < n; ++i) seen[i] = {ds[i], i};
  std::sort(seen.begin(), seen.end());
  for (size_t k = 1; k < n; ++k)
    if (seen[k].first == seen[k - 1].first)
      return refuse(ctx, seen[k].second, "the same dataset as request " + std::to_string(seen[k - 1].second));
  if (n == 0) return CP2_OK;
  CP2_REFUSE_STUCK(ctx);
  return set_roots_pass(ctx, ds, all_roots, n, own);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
