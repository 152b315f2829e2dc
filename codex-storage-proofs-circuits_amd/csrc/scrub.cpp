// Scrub behind the C ABI: cp2_dataset_scrub and cp2_datasets_scrub_many (include/codex_p2.h); cp2_multi_dataset_scrub (multi_gpu.cpp) runs
// scrub_items per shard.
//
// A storage node keeps a slot's trees -- every node, the compact layers or the roots -- and proves every period from the touched blocks
// alone; nothing on that path reads the rest of the slot.  A scrub re-reads the selected slots from the dataset's source and hashes them
// exactly as the compact / roots-only builds do (dataset_build_transient, proof_input.cpp): batches of about half a staging chunk of nodes
// in a BuildScratch, two node buffers used alternately, nothing synchronised per batch.  Where the build copies out what it keeps, the
// scrub compares instead: the builder's SlotsDone hook -- on the stream the batch's layer passes ran on -- launches k_scrub_compare over the
// fresh layer and the kept one (the fresh layer never leaves the device) and downloads one count per 4096 rows into pinned memory.  When
// batch k's node buffer is handed to batch k + 2 the host reads batch k's counts and downloads bitmap words only for tiles with a
// mismatch; batches are decoded in order, so the report comes out sorted by (item, row) with no sort anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "dataset_obj.hpp"
#include "trees.hpp"

using namespace cp2i;

namespace {

// The batch loop, shared by scrub_items (one dataset) and cp2_datasets_scrub_many (the slots of many datasets as one run of items).
// Two things differ between them, and nothing else:
//   the ITEM source   item i is unit item0 + i of `src` (slot files "<base><k>.dat" or the fake source), or -- a name table -- the whole
//                     file (*names)[i];
//   the KEPT source   the kept layer of item i starts at base + i * stride * 32, or -- an address table -- at the device address
//                     addr[i].  A batch's slice of the table goes into one of two pinned host tables, is uploaded to one of two device
//                     tables on the stream the compare runs on, just before it, and is read by k_scrub_compare_many; table b is
//                     rewritten for batch k + 2 only after batch k's `landed` event, like node buffer b: a table outlives its copy.
// Mismatches come out as (item0 + i, row) pairs in order, at most `cap`; *n_bad counts all.  item_counts (may be null; n_items entries,
// zeroed by the caller) receives the mismatches of every item, complete whatever `cap` is: every tile with a mismatch is decoded then.
struct ScrubItemSource {
  const ScrubSrc* src = nullptr;
  uint64_t item0 = 0;
  const std::vector<std::string>* names = nullptr;
};
struct ScrubKeptSource {
  const uint8_t* base = nullptr;
  size_t stride = 0;
  const uint64_t* addr = nullptr;
};

int scrub_loop(cp2_ctx* ctx, const ScrubItemSource& items, const ScrubKeptSource& keptsrc, uint64_t n_items, int level, size_t cap,
               std::vector<uint64_t>& bad, uint64_t* n_bad, uint64_t* item_counts, size_t* n_batches = nullptr) {
  const ScrubSrc& src = *items.src;
  const uint64_t item0 = items.item0;
  const uint8_t* kept = keptsrc.base;
  const uint64_t* addr = keptsrc.addr;
  const size_t kstride = addr ? 0 : keptsrc.stride;
  *n_bad = 0;
  if (n_items == 0) return CP2_OK;
  if ((!kept && !addr) || src.cell_size == 0 || src.block_size < src.cell_size) return CP2_ERR_INVALID;
  if (items.names && (!src.from_file || items.names->size() != n_items)) return CP2_ERR_INVALID;
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const size_t nblocks = src.n_cells / (src.block_size / src.cell_size);
  const size_t rows = level == CP2_SCRUB_CELL ? src.n_cells : (level == CP2_SCRUB_BLOCK ? nblocks : 1);
  if (rows == 0 || (!addr && kstride < rows)) return CP2_ERR_INVALID;
  // batches as the compact build cuts them (transient_batch_slots, proof_input.cpp): half a staging chunk of nodes, at least one item
  const size_t per_item = std::max<size_t>(1, trees_node_bytes(1, src.cell_size, src.block_size, src.n_cells));
  const size_t batch = std::max<size_t>(1, std::min<size_t>(n_items, (ctx->stage_bytes / 2) / per_item));
  const size_t groups = cp2k::scrub_groups(batch * rows);
  const int n_bufs = n_items > batch ? 2 : 1;
  DevBuf d_bits[2], d_counts[2];               // (declared before the scratch: they go after it has drained the streams)
  DevBuf d_addr[2];
  PinBuf h_counts[2], h_addr[2];
  for (int b = 0; b < n_bufs; ++b) {
    CP2_TRY(d_bits[b].scratch(ctx, groups * cp2k::SCRUB_TILE / 8));
    CP2_TRY(d_counts[b].scratch(ctx, groups * 4));
    CP2_TRY(h_counts[b].alloc(ctx, groups * 4));
    if (addr) {
      CP2_TRY(d_addr[b].scratch(ctx, batch * 8));
      CP2_TRY(h_addr[b].alloc(ctx, batch * 8));
    }
  }
  struct Pending { bool live = false; uint64_t s0 = 0; size_t n = 0; } pending[2];
  std::vector<uint64_t> words(cp2k::SCRUB_TILE / 64);
  uint64_t total = 0;
  // batch in buffer b has landed (its event completed): its counts are in h_counts[b], its bitmap in d_bits[b]
  auto collect = [&](int b) -> int {
    Pending& p = pending[b];
    if (!p.live) return CP2_OK;
    p.live = false;
    const size_t ng = cp2k::scrub_groups(p.n * rows);
    const uint32_t* c = static_cast<const uint32_t*>(h_counts[b].p);
    for (size_t w = 0; w < ng; ++w) {
      if (!c[w]) continue;
      total += c[w];
      if (bad.size() / 2 >= cap && !item_counts) continue;      // the report is full: only counting from here on
      CP2_HIP(ctx, hipMemcpy(words.data(), d_bits[b].u8() + w * (cp2k::SCRUB_TILE / 8), cp2k::SCRUB_TILE / 8, hipMemcpyDeviceToHost));
      for (size_t k = 0; k < words.size() && (bad.size() / 2 < cap || item_counts); ++k)
        for (uint64_t m = words[k]; m && (bad.size() / 2 < cap || item_counts); m &= m - 1) {
          const uint64_t g = w * cp2k::SCRUB_TILE + k * 64 + (uint64_t)__builtin_ctzll(m);
          if (g >= p.n * rows) break;             // (never: the kernel leaves the words past the last row zero)
          if (item_counts) ++item_counts[p.s0 + g / rows];
          if (bad.size() / 2 >= cap) continue;
          bad.push_back(item0 + p.s0 + g / rows);
          bad.push_back(g % rows);
        }
    }
    return CP2_OK;
  };
  int st = CP2_OK;
  {
    BuildScratch scratch;                       // drains the context's streams before its buffers go, whatever path leaves this scope
    hipEvent_t landed[2] = {nullptr, nullptr};
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 2; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } ev_guard{landed};
    for (int i = 0; i < 2; ++i) CP2_HIP(ctx, hipEventCreateWithFlags(&landed[i], hipEventDisableTiming));
    size_t k = 0;
    for (uint64_t s0 = 0; st == CP2_OK && s0 < n_items; s0 += batch, ++k) {
      const size_t n = (size_t)std::min<uint64_t>(batch, n_items - s0);
      const int b = (int)(k & 1);
      if (k >= 2) {
        if (hipEventSynchronize(landed[b]) != hipSuccess) { (void)hipGetLastError(); ctx->err = "scrub: a batch failed on the device"; st = CP2_ERR_HIP; break; }
        st = collect(b);
        if (st != CP2_OK) break;
      }
      const uint8_t* kept_b = addr ? nullptr : kept + s0 * kstride * 32;
      if (addr) std::copy(addr + s0, addr + s0 + n, static_cast<uint64_t*>(h_addr[b].p));   // (table b's last copy landed with batch k - 2)
      // the builder calls this once, with every slot of the batch, on the stream its layer passes ran on (group 0: one pass at the end)
      SlotsDone compare = [&, b, n, kept_b](cp2_slot_trees* t, size_t a, size_t z, hipStream_t ls) -> int {
        if (a != 0 || z != n) { ctx->err = "scrub: a batch's layers were built in parts"; return CP2_ERR_INVALID; }
        const size_t off = level == CP2_SCRUB_CELL ? t->boff[0] : (level == CP2_SCRUB_BLOCK ? t->toff[0] : t->toff.back());
        const size_t fstride = level == CP2_SCRUB_CELL ? t->n_cells : (level == CP2_SCRUB_BLOCK ? t->tsizes[0] : 1);
        if (addr) {
          CP2_HIP(ctx, hipMemcpyAsync(d_addr[b].p, h_addr[b].p, n * 8, hipMemcpyHostToDevice, ls));
          CP2_HIP(ctx, cp2k::launch_scrub_compare_many(t->nodes.u8() + off * 32, fstride, static_cast<const uint64_t*>(d_addr[b].p), rows, n,
                                                       static_cast<uint64_t*>(d_bits[b].p), static_cast<uint32_t*>(d_counts[b].p), ls));
        } else {
          CP2_HIP(ctx, cp2k::launch_scrub_compare(t->nodes.u8() + off * 32, fstride, kept_b, kstride, rows, n, static_cast<uint64_t*>(d_bits[b].p),
                                                  static_cast<uint32_t*>(d_counts[b].p), ls));
        }
        CP2_HIP(ctx, hipMemcpyAsync(h_counts[b].p, d_counts[b].p, cp2k::scrub_groups(n * rows) * 4, hipMemcpyDeviceToHost, ls));
        return CP2_OK;
      };
      cp2_slot_trees* t = nullptr;
      st = items.names  ? trees_build_file_list(ctx, items.names->data() + s0, n, src.cell_size, src.block_size, src.n_cells, 0, compare, &t, true,
                                                &scratch, b)
           : src.from_file ? trees_build_files(ctx, src.file_base, item0 + s0, n, src.cell_size, src.block_size, src.n_cells, 0, compare, &t,
                                             src.units_per_slot, true, &scratch, b)
                         : trees_build_fake(ctx, src.seed, item0 + s0, n, src.cell_size, src.block_size, src.n_cells, 0, compare, &t,
                                            src.units_per_slot, true, &scratch, b);
      hipStream_t tail = scratch.tail_stream ? scratch.tail_stream : ctx->stream;
      if (st == CP2_OK && hipEventRecord(landed[b], tail) != hipSuccess) { ctx->err = "hipEventRecord failed"; st = CP2_ERR_HIP; }
      cp2_slot_trees_free(t);                   // (the batch's nodes are the scratch's: nothing is waited for here)
      if (st == CP2_OK) { pending[b].live = true; pending[b].s0 = s0; pending[b].n = n; }
    }
    if (st == CP2_OK) {                         // everything landed (a failed launch or copy shows up here)
      if (hipStreamSynchronize(ctx->stream) != hipSuccess || (ctx->aux_stream && hipStreamSynchronize(ctx->aux_stream) != hipSuccess) ||
          (ctx->aux2_stream && hipStreamSynchronize(ctx->aux2_stream) != hipSuccess)) {
        (void)hipGetLastError();
        ctx->err = "scrub: a batch failed on the device";
        st = CP2_ERR_HIP;
      }
    }
    if (st == CP2_OK) st = collect((int)(k & 1));          // the older of the two batches still pending first
    if (st == CP2_OK) st = collect((int)((k + 1) & 1));
  }
  if (st != CP2_OK) return st;
  *n_bad = total;
  if (n_batches) *n_batches = (size_t)((n_items + batch - 1) / batch);
  return CP2_OK;
}

// the kept layer of `level` of local slot `local` of a dataset: the dataset's layer-major `trees`, its `compact` layers (coff / csizes)
// or its roots; *kstride = rows from one slot's layer to the next
const uint8_t* kept_layer(const cp2_dataset* ds, int level, uint64_t local, size_t* kstride) {
  if (level == CP2_SCRUB_CELL) {
    *kstride = ds->trees->n_cells;
    return ds->trees->nodes.u8() + (ds->trees->boff[0] + local * ds->trees->n_cells) * 32;
  }
  if (level == CP2_SCRUB_BLOCK && ds->trees) {
    *kstride = ds->trees->tsizes[0];
    return ds->trees->nodes.u8() + (ds->trees->toff[0] + local * ds->trees->tsizes[0]) * 32;
  }
  if (level == CP2_SCRUB_BLOCK) {
    *kstride = ds->csizes[0];
    return ds->compact.u8() + (ds->coff[0] + local * ds->csizes[0]) * 32;
  }
  *kstride = 1;
  return static_cast<const uint8_t*>(dataset_roots_dev(ds)) + local * 32;
}

}  // namespace

int cp2i::scrub_items(cp2_ctx* ctx, const ScrubSrc& src, uint64_t item0, uint64_t n_items, int level, const uint8_t* kept, size_t kstride,
                      size_t cap, std::vector<uint64_t>& bad, uint64_t* n_bad) {
  *n_bad = 0;
  if (n_items == 0) return CP2_OK;
  if (!kept) return CP2_ERR_INVALID;
  ScrubItemSource items;
  items.src = &src;
  items.item0 = item0;
  ScrubKeptSource ks;
  ks.base = kept;
  ks.stride = kstride;
  return scrub_loop(ctx, items, ks, n_items, level, cap, bad, n_bad, nullptr);
}

ScrubSrc cp2i::scrub_src_of(const cp2_slot_trees* t, uint64_t units_per_slot) {
  return {t->src == CellSrc::File, t->file_base, t->dataset_seed, t->cell_size, t->block_size, t->n_cells, units_per_slot};
}
ScrubSrc cp2i::scrub_src_of(const cp2_dataset* ds) {
  return {ds->from_file, ds->file_base, ds->cfg.seed, ds->cfg.cell_size, ds->cfg.block_size, ds->cfg.n_cells, 1};
}

int cp2i::dataset_scrub_level(const cp2_dataset* ds) {
  return ds->trees ? CP2_SCRUB_CELL : (ds->tree_mode == 2 ? CP2_SCRUB_BLOCK : CP2_SCRUB_SLOT);
}

int cp2i::dataset_scrub(cp2_dataset* ds, uint64_t first_slot, uint64_t n, int level, size_t cap, std::vector<uint64_t>& bad, uint64_t* n_bad) {
  *n_bad = 0;
  if (level > dataset_scrub_level(ds) || first_slot < ds->first_slot || first_slot - ds->first_slot > ds->n_local ||
      n > ds->n_local - (first_slot - ds->first_slot))
    return CP2_ERR_INVALID;
  const uint64_t local = first_slot - ds->first_slot;
  size_t kstride = 1;
  const uint8_t* kept = kept_layer(ds, level, local, &kstride);   // of the first slot scrubbed
  return scrub_items(ds->ctx, scrub_src_of(ds), first_slot, n, level, kept, kstride, cap, bad, n_bad);
}

extern "C" int cp2_dataset_scrub(cp2_dataset* ds, uint64_t first_slot, uint64_t n_slots, uint64_t* bad, size_t cap, size_t* n_bad,
                                 int* granularity) try {
  if (!ds || !n_bad || (cap && !bad)) return CP2_ERR_INVALID;
  cp2_ctx* ctx = ds->ctx;
  if (n_slots == 0) {
    first_slot = ds->first_slot;
    n_slots = ds->n_local;
  }
  if (first_slot < ds->first_slot || first_slot - ds->first_slot >= ds->n_local || n_slots > ds->n_local - (first_slot - ds->first_slot)) {
    ctx->err = "scrub: slots " + std::to_string(first_slot) + " + " + std::to_string(n_slots) + " are not inside the local range " +
               std::to_string(ds->first_slot) + " + " + std::to_string(ds->n_local);
    return CP2_ERR_INVALID;
  }
  CP2_REFUSE_STUCK(ctx);
  const auto t0 = std::chrono::steady_clock::now();
  const int level = dataset_scrub_level(ds);
  std::vector<uint64_t> got;
  uint64_t count = 0;
  CP2_TRY(dataset_scrub(ds, first_slot, n_slots, level, cap, got, &count));
  std::copy(got.begin(), got.end(), bad);      // (got holds min(cap, count) pairs)
  *n_bad = (size_t)count;
  if (granularity) *granularity = level;
  if (std::getenv("CP2_TRACE")) {
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const double bytes = (double)n_slots * (double)ds->cfg.n_cells * (double)ds->cfg.cell_size;
    std::fprintf(stderr, "[cp2 trace] scrub: slots %llu..%llu (%llu), %.0f bytes, %.3f s (%.2f GB/s), %llu mismatch(es) at %s level\n",
                 (unsigned long long)first_slot, (unsigned long long)(first_slot + n_slots - 1), (unsigned long long)n_slots, bytes, s,
                 s > 0 ? bytes / s / 1e9 : 0.0, (unsigned long long)count, level == CP2_SCRUB_CELL ? "cell" : (level == CP2_SCRUB_BLOCK ? "block" : "slot"));
  }
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// ---- cp2_datasets_scrub_many: every local slot of n datasets in one pass (include/codex_p2.h) --------------------------------------
// The requests are grouped into CLASSES of equal (cell size, block size, cells per slot, level, source kind); a class's items are its
// (request, local slot) pairs in request order, so what scrub_loop reports for a class -- (item, row) in order -- is already sorted by
// (request, slot, index).  A file-sourced class runs through scrub_loop with a name table (one file per item) and an address table (the
// kept layer of each item, wherever its dataset keeps it); fake-source requests are regenerated one by one through dataset_scrub.
namespace {

struct ManyClass {
  ScrubSrc src;
  int level = 0;
  std::vector<size_t> request;            // per item
  std::vector<uint64_t> slot;             // per item: the dataset's slot number
  std::vector<std::string> names;         // per item: its slot file
  std::vector<uint64_t> addr;             // per item: device address of row 0 of its kept layer
};

struct Triple {
  uint64_t request, slot, index;
  bool operator<(const Triple& o) const {
    return request != o.request ? request < o.request : (slot != o.slot ? slot < o.slot : index < o.index);
  }
};

int scrub_many(cp2_ctx* ctx, cp2_dataset* const* ds, size_t n, size_t cap, std::vector<Triple>& out, uint64_t* total,
               std::vector<uint64_t>& counts, std::vector<int>& levels, size_t* n_classes, size_t* n_items, size_t* n_batches, size_t* n_fake, double* bytes) {
  std::vector<ManyClass> classes;
  std::vector<size_t> fake;
  for (size_t i = 0; i < n; ++i) {
    const cp2_dataset* d = ds[i];
    const cp2_config& c = d->cfg;
    levels[i] = dataset_scrub_level(d);
    if (!d->from_file) { fake.push_back(i); continue; }
    *n_items += (size_t)d->n_local;           // (what the trace line accounts for: the slot files read)
    *bytes += (double)d->n_local * (double)c.n_cells * (double)c.cell_size;
    ManyClass* k = nullptr;
    for (auto& q : classes)
      if (q.src.cell_size == c.cell_size && q.src.block_size == c.block_size && q.src.n_cells == c.n_cells && q.level == levels[i]) { k = &q; break; }
    if (!k) {
      classes.emplace_back();
      k = &classes.back();
      k->src.from_file = true;
      k->src.cell_size = c.cell_size;
      k->src.block_size = c.block_size;
      k->src.n_cells = c.n_cells;
      k->level = levels[i];
    }
    for (uint64_t local = 0; local < d->n_local; ++local) {
      size_t kstride = 0;
      k->request.push_back(i);
      k->slot.push_back(d->first_slot + local);
      k->names.push_back(slot_file_name(d->file_base, d->first_slot + local));
      k->addr.push_back((uint64_t)reinterpret_cast<uintptr_t>(kept_layer(d, levels[i], local, &kstride)));
    }
  }
  *n_classes = classes.size();
  *n_fake = fake.size();
  std::vector<uint64_t> got;
  for (const ManyClass& k : classes) {
    if (k.names.empty()) continue;
    ScrubItemSource items;
    items.src = &k.src;
    items.names = &k.names;
    ScrubKeptSource ks;
    ks.addr = k.addr.data();
    std::vector<uint64_t> per_item(k.names.size(), 0);
    uint64_t count = 0;
    got.clear();
    size_t batches = 0;
    CP2_TRY(scrub_loop(ctx, items, ks, k.names.size(), k.level, cap, got, &count, per_item.data(), &batches));
    *n_batches += batches;
    *total += count;
    for (size_t j = 0; j < per_item.size(); ++j) counts[k.request[j]] += per_item[j];
    for (size_t j = 0; j + 1 < got.size(); j += 2) out.push_back({(uint64_t)k.request[got[j]], k.slot[got[j]], got[j + 1]});
  }
  for (size_t i : fake) {
    uint64_t count = 0;
    got.clear();
    CP2_TRY(dataset_scrub(ds[i], ds[i]->first_slot, ds[i]->n_local, levels[i], cap, got, &count));
    *total += count;
    counts[i] += count;
    for (size_t j = 0; j + 1 < got.size(); j += 2) out.push_back({(uint64_t)i, got[j], got[j + 1]});
  }
  // every class kept its lowest `cap`: the lowest `cap` of all are among them
  std::sort(out.begin(), out.end());
  if (out.size() > cap) out.resize(cap);
  return CP2_OK;
}

}  // namespace

extern "C" int cp2_datasets_scrub_many(cp2_ctx* ctx, cp2_dataset* const* ds, size_t n, uint64_t* bad, size_t cap, size_t* n_bad,
                                       uint64_t* counts, int* granularity) try {
  if (!ctx) return CP2_ERR_INVALID;
  if (!n_bad || (n && !ds) || (cap && !bad)) {
    ctx->err = !n_bad ? "scrub many: n_bad is NULL" : (cap && !bad ? "scrub many: cap > 0 with bad NULL" : "scrub many: ds is NULL");
    return CP2_ERR_INVALID;
  }
  for (size_t i = 0; i < n; ++i) {
    if (!ds[i]) { ctx->err = "request " + std::to_string(i) + ": NULL dataset"; return CP2_ERR_INVALID; }
    if (ds[i]->ctx != ctx) { ctx->err = "request " + std::to_string(i) + ": its dataset belongs to another context"; return CP2_ERR_INVALID; }
  }
  if (n == 0) { *n_bad = 0; return CP2_OK; }
  CP2_REFUSE_STUCK(ctx);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<Triple> out;
  std::vector<uint64_t> per_request(n, 0);
  std::vector<int> levels(n, 0);
  uint64_t total = 0;
  size_t n_classes = 0, n_items = 0, n_batches = 0, n_fake = 0;
  double bytes = 0;
  CP2_TRY(scrub_many(ctx, ds, n, cap, out, &total, per_request, levels, &n_classes, &n_items, &n_batches, &n_fake, &bytes));
  for (size_t j = 0; j < out.size(); ++j) { bad[3 * j] = out[j].request; bad[3 * j + 1] = out[j].slot; bad[3 * j + 2] = out[j].index; }
  *n_bad = (size_t)total;
  if (counts) std::copy(per_request.begin(), per_request.end(), counts);
  if (granularity) std::copy(levels.begin(), levels.end(), granularity);
  if (std::getenv("CP2_TRACE")) {
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "[cp2 trace] scrub many: %zu request(s), %zu of them fake-source (regenerated one by one, not counted in what follows); %zu class(es) of slot files, %zu item(s) in %zu batch(es), %.0f bytes read, %.3f s (%.2f GB/s), %llu mismatch(es)\n",
                 n, n_fake, n_classes, n_items, n_batches, bytes, s, s > 0 ? bytes / s / 1e9 : 0.0, (unsigned long long)total);
  }
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
