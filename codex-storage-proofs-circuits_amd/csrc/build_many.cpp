// cp2_datasets_build_many behind the C ABI (include/codex_p2.h): n datasets of one context built in ONE pass.
//
// A storage node holds one-slot datasets by the thousand; built one by one with cp2_dataset_build, every dataset pays a whole ingestion
// pipe (rings, events, a copy stream set up and torn down), a sliver of a hash launch and a drain of the device: 5.7 ms a dataset of 8
// MiB, 27 times what the same files cost as the slots of one dataset (profiles/scrub_many_rate.txt).  The read side of one pass over the
// slots of many datasets exists since cp2_datasets_scrub_many: trees_build_file_list builds a batch from a table of file names, and the
// batch loop (batch_loop.hpp; DESIGN.md, "The batch loop") drives it.  This is the scrub's mirror image on the write side.  Where the
// scrub COMPARES a batch's fresh layer with the kept layers through a table of addresses, the build WRITES the batch's layers through
// one: one k_scatter_rows_addr launch per kept layer, whatever number of datasets the batch's items belong to (dataset_keep_from_batch,
// proof_input.cpp, is one hipMemcpyAsync per layer into ONE dataset's layout: 4096 x 8 tiny copies here).
//
// The plan -- classes, items, batches, the row of every kept layer in a batch and in a request's buffer, the address tables -- is
// build_many_plan.hpp (host only).  What the datasets keep lives in ARENAS: device allocations shared by consecutive requests of the call
// (about ARENA_BYTES each, a larger request alone in its own), each dataset holding a reference and a borrowed view of its slice, so that
// the call makes a handful of allocations instead of one or three per dataset, and cp2_dataset_free works on any subset in any order: an
// arena goes with the last dataset that has a slice of it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "build_many_plan.hpp"
#include "dataset_obj.hpp"
#include "trees.hpp"

using namespace cp2i;

namespace {

constexpr size_t ARENA_BYTES = (size_t)64 << 20;   // what a dataset that outlives its neighbours can hold back beyond its own slice
constexpr size_t ARENA_ALIGN = 256;

struct Built {                                    // the datasets of one attempt: freed unless released
  std::vector<cp2_dataset*> ds;
  ~Built() { for (cp2_dataset* d : ds) cp2_dataset_free(d); }
};

// what request i keeps under `mode`, in bytes (the plan's rows; equal to trees_node_bytes / compact_bytes / 32 per root)
size_t kept_bytes(const BuildRequest& r, int mode) {
  return (size_t)(build_many_layers(r.cell_size, r.block_size, r.n_cells, mode).kept_rows * r.n_local * 32);
}

// Every file-sourced request's dataset object with its slice of an arena, laid out as cp2_dataset_build lays out what it keeps;
// base[i] = the device address of row 0 of request i's slice (0 for the fake-source requests, which are not made here).
int allocate(cp2_ctx* ctx, const cp2_config* cfgs, const std::vector<BuildRequest>& req, int mode, Built& built, std::vector<uint64_t>& base) {
  const size_t n = req.size();
  built.ds.assign(n, nullptr);
  base.assign(n, 0);
  for (size_t i0 = 0; i0 < n;) {
    // requests [i0, i1): one arena
    size_t i1 = i0, bytes = 0;
    std::vector<size_t> off;
    for (; i1 < n; ++i1) {
      const size_t b = req[i1].from_file ? (kept_bytes(req[i1], mode) + ARENA_ALIGN - 1) / ARENA_ALIGN * ARENA_ALIGN : 0;
      if (bytes && bytes + b > ARENA_BYTES) break;
      off.push_back(bytes);
      bytes += b;
    }
    if (bytes) {
      std::shared_ptr<DevBuf> arena = std::make_shared<DevBuf>();
      CP2_TRY(arena->alloc(ctx, bytes));
      for (size_t i = i0; i < i1; ++i) {
        if (!req[i].from_file) continue;
        cp2_dataset* d = dataset_new(ctx, &cfgs[i], req[i].first_slot, req[i].n_local);
        if (!d) return CP2_ERR_ALLOC;
        built.ds[i] = d;
        d->arena = arena;
        uint8_t* p = arena->u8() + off[i - i0];
        const size_t want = kept_bytes(req[i], mode);
        if (mode == 1) {
          d->trees = trees_new(ctx, (size_t)req[i].n_local, req[i].cell_size, req[i].block_size, (size_t)req[i].n_cells);
          if (!d->trees) return CP2_ERR_ALLOC;
          d->trees->src = CellSrc::File;              // sampled cells come from the request's own slot files, as in a dataset cp2_dataset_build made
          d->trees->file_base = d->file_base;
          d->trees->first_slot = req[i].first_slot;
          DevBuf view;
          view.borrow(p, want);
          CP2_TRY(trees_layout(d->trees, &view));
          if (d->trees->nodes.p != p || d->trees->nodes.bytes != want) { ctx->err = "build many: the plan and trees_layout disagree about a request's nodes"; return CP2_ERR_INVALID; }
        } else {
          if (dataset_kept_layout(d, mode) != want) { ctx->err = "build many: the plan and the kept layout disagree about a request's bytes"; return CP2_ERR_INVALID; }
          (mode == 2 ? d->compact : d->local_roots).borrow(p, want);
        }
        base[i] = (uint64_t)reinterpret_cast<uintptr_t>(p);
      }
    }
    i0 = i1;
  }
  return CP2_OK;
}

// One class through the batch loop: two pinned and two device address tables of kept layers x batch entries, table b rewritten for
// batch k + 2 only after batch k's event, like node buffer b; in the builder's SlotsDone hook -- on the stream the batch's layer passes
// ran on -- the table's upload, then one k_scatter_rows_addr launch per kept layer.  No HIP call per dataset anywhere in here.
int build_class(cp2_ctx* ctx, const BuildClass& k, int mode, const std::vector<BuildRequest>& req, const std::vector<std::string>& names,
                const std::vector<uint64_t>& base) {
  const BuildLayers L = build_many_layers(k.cell_size, k.block_size, k.n_cells, mode);
  const size_t n_items = k.n_items(), batch = k.batch, nl = L.n();
  if (n_items == 0) return CP2_OK;
  const int n_bufs = n_items > batch ? 2 : 1;
  DevBuf d_addr[2];                             // (declared before the device: they go after its scratch has drained the streams)
  PinBuf h_addr[2];
  for (int b = 0; b < n_bufs; ++b) {
    CP2_TRY(d_addr[b].scratch(ctx, nl * batch * 8));
    CP2_TRY(h_addr[b].alloc(ctx, nl * batch * 8));
  }
  const ItemSource src{true, std::string(), 0, k.cell_size, k.block_size, (size_t)k.n_cells, 1, names.data(), names.size()};
  // the builder calls this once, with every slot of the batch, on the stream its layer passes ran on (group 0: one pass at the end)
  const auto keep = [&](const BatchStep& s, cp2_slot_trees* t, size_t a, size_t z, hipStream_t ls) -> int {
    const size_t b = (size_t)s.b, n = s.n;
    if (a != 0 || z != n || t->n_slots != n) { ctx->err = "build many: a batch's layers were built in parts"; return CP2_ERR_INVALID; }
    const size_t below = mode == 1 ? t->bsizes.size() - 1 : 0;             // kept layers below the block roots
    if (nl != (mode == 0 ? 1 : below + t->tsizes.size())) { ctx->err = "build many: the plan and the batch disagree about the kept layers"; return CP2_ERR_INVALID; }
    CP2_HIP(ctx, hipMemcpyAsync(d_addr[b].p, h_addr[b].p, nl * n * 8, hipMemcpyHostToDevice, ls));
    for (size_t layer = 0; layer < nl; ++layer) {
      const size_t src_row = (size_t)build_many_src_row(L, layer, n);
      // the plan's row against the batch's own layout: a write through a wrong row is a fault, not a wrong answer
      const size_t big = mode == 0 ? t->tsizes.size() - 1 : layer - below;
      const size_t have = layer < below ? t->boff[layer] : t->toff[big];
      const size_t rows = layer < below ? t->nblocks * t->bsizes[layer] : t->tsizes[big];
      if (src_row != have || rows != L.rows[layer] || (src_row + n * rows) * 32 > t->nodes.bytes) {
        ctx->err = "build many: the plan and the batch disagree about a layer";
        return CP2_ERR_INVALID;
      }
      CP2_HIP(ctx, cp2k::launch_scatter_rows_addr(t->nodes.u8() + src_row * 32, rows, static_cast<const uint64_t*>(d_addr[b].p) + layer * n, rows, n, ls));
    }
    return CP2_OK;
  };
  BatchDevice dev;
  CP2_TRY(dev.init(ctx));
  return batch_loop(dev, "build many", ctx->err, n_items, batch,
      [&](const BatchStep& s) -> int {   // (table b's last upload landed with batch k - 2)
        if (build_many_addr_table(k, L, req, base.data(), s.s0, s.n, static_cast<uint64_t*>(h_addr[s.b].p))) return CP2_OK;
        ctx->err = "build many: a kept row outside its request's buffer";
        return CP2_ERR_INVALID;
      },
      [&](const BatchStep& s, hipStream_t* tail) -> int {
        return dev.build(src, s.s0, s.n, 0, [&](cp2_slot_trees* t, size_t a, size_t z, hipStream_t ls) { return keep(s, t, a, z, ls); }, s.b, tail);
      },
      [](const BatchStep&, hipStream_t) -> int { return CP2_OK; }, [](const BatchStep&) {});
}

// one attempt in `mode`: every dataset of the call in built.ds, or an error (the caller frees what the attempt made)
int build_in_mode(cp2_ctx* ctx, const cp2_config* cfgs, const std::vector<BuildRequest>& req, const BuildPlan& plan, int mode, Built& built) {
  std::vector<uint64_t> base;
  const auto t0 = std::chrono::steady_clock::now();
  CP2_TRY(allocate(ctx, cfgs, req, mode, built, base));
  if (std::getenv("CP2_TRACE"))                  // the host-side split: the objects and their allocations against the pass that follows
    std::fprintf(stderr, "[cp2 trace] build many: %zu dataset object(s) and their shared allocations made in %.4f s, before the pass\n",
                 req.size() - plan.fake.size(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  for (const BuildClass& k : plan.classes) {
    std::vector<std::string> names(k.n_items());
    for (size_t j = 0; j < names.size(); ++j) names[j] = slot_file_name(built.ds[k.request[j]]->file_base, req[k.request[j]].first_slot + k.local[j]);
    CP2_TRY(build_class(ctx, k, mode, req, names, base));
  }
  for (size_t i : plan.fake)                    // regenerated data has no files to list: the single-dataset path, inside the same call
    CP2_TRY(dataset_build_in_mode(ctx, &cfgs[i], req[i].first_slot, req[i].n_local, mode, &built.ds[i]));
  return CP2_OK;
}

// The mode of the whole call: the caller's word (cp2_set_keep_trees / CODEX_P2_KEEP_TREES) for every request, else the most that fits
// under dataset_tree_mode's arithmetic over the call's totals: the sum of what the requests keep, one staging, one pair of batches in
// flight (the largest class's) and the headroom.  -1: CODEX_P2_KEEP_TREES is malformed.
int call_mode(cp2_ctx* ctx, const std::vector<BuildRequest>& req, const BuildPlan& plan, bool* automatic) {
  const int named = dataset_named_mode(ctx, automatic);
  if (named != -2) return named;
  typedef unsigned __int128 u128;
  u128 data = 0, nodes_all = 0, compact_all = 0, in_flight = 0;
  for (const BuildRequest& r : req) {
    data += (u128)r.n_local * r.n_cells * r.cell_size;
    nodes_all += (u128)kept_bytes(r, 1);
    compact_all += (u128)kept_bytes(r, 2);
    if (!r.from_file)
      in_flight = std::max<u128>(in_flight, 2 * (u128)trees_node_bytes(trees_batch_items(ctx, r.cell_size, r.block_size, r.n_cells, r.n_local), r.cell_size, r.block_size, r.n_cells));
  }
  for (const BuildClass& k : plan.classes)
    in_flight = std::max<u128>(in_flight, 2 * (u128)trees_node_bytes(k.batch, k.cell_size, k.block_size, (size_t)k.n_cells));
  return dataset_mode_that_fits(ctx, data, nodes_all, compact_all, in_flight);
}

}  // namespace

extern "C" int cp2_datasets_build_many(cp2_ctx* ctx, const cp2_config* cfgs, const uint64_t* ranges, size_t n, cp2_dataset** out) try {
  if (out)
    for (size_t i = 0; i < n; ++i) out[i] = nullptr;
  if (!ctx) return CP2_ERR_INVALID;
  if (!out || (n && (!cfgs || !ranges))) {
    ctx->err = !out ? "build many: out is NULL" : (!cfgs ? "build many: cfgs is NULL" : "build many: ranges is NULL");
    return CP2_ERR_INVALID;
  }
  std::vector<BuildRequest> req(n);
  for (size_t i = 0; i < n; ++i) {
    const cp2_config& c = cfgs[i];
    const uint64_t first = ranges[2 * i], n_local = ranges[2 * i + 1];
    if (dataset_check(&c, first, n_local) != CP2_OK || trees_check_geometry(c.cell_size, c.block_size, c.n_cells, n_local) != CP2_OK) {
      const std::string why = build_many_refusal(c.n_slots, first, n_local, c.max_depth, c.max_log2_nslots, c.cell_size, c.block_size, c.n_cells,
                                                 c.file_base != nullptr, SLOT_FILE_MAX_CELL);
      ctx->err = "request " + std::to_string(i) + ": " + (why.empty() ? std::string("cp2_dataset_build refuses its configuration or its slots") : why);
      return CP2_ERR_INVALID;
    }
    req[i].cell_size = c.cell_size; req[i].block_size = c.block_size; req[i].n_cells = c.n_cells;
    req[i].first_slot = first; req[i].n_local = n_local; req[i].from_file = c.file_base != nullptr;
  }
  if (n == 0) return CP2_OK;
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  const BuildPlan plan = build_many_plan(req, ctx->stage_bytes);
  bool automatic = false;
  int mode = call_mode(ctx, req, plan, &automatic);
  if (mode < 0) return CP2_ERR_INVALID;
  for (;;) {
    Built built;
    const int st = build_in_mode(ctx, cfgs, req, plan, mode, built);
    if (st == CP2_OK) {
      std::copy(built.ds.begin(), built.ds.end(), out);
      built.ds.clear();
      break;
    }
    for (cp2_dataset*& d : built.ds) { cp2_dataset_free(d); d = nullptr; }   // (frees what the failed attempt holds before anything else is tried)
    if (st != CP2_ERR_ALLOC || !automatic || !step_down(ctx, &mode, "build many")) return st;
  }
  if (std::getenv("CP2_TRACE")) {
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double bytes = 0;
    for (const BuildRequest& r : req)
      if (r.from_file) bytes += (double)r.n_local * (double)r.n_cells * (double)r.cell_size;
    std::fprintf(stderr, "[cp2 trace] build many: %zu request(s), %zu of them fake-source (built one by one); %zu class(es) of slot files, %zu item(s) in %zu batch(es), %.0f bytes read, %.3f s (%.2f GB/s), mode %d\n",
                 n, plan.fake.size(), plan.classes.size(), plan.n_items, plan.n_batches, bytes, s, s > 0 ? bytes / s / 1e9 : 0.0, mode);
  }
  return CP2_OK;
} catch (const std::bad_alloc&) {
  if (out)
    for (size_t i = 0; i < n; ++i) out[i] = nullptr;
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  if (out)
    for (size_t i = 0; i < n; ++i) out[i] = nullptr;
  return CP2_ERR_INVALID;
}
