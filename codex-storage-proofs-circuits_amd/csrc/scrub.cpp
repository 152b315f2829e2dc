// Scrub behind the C ABI: cp2_dataset_scrub and cp2_datasets_scrub_many (include/codex_p2.h); cp2_multi_dataset_scrub (multi_gpu.cpp) runs
// scrub_items per shard.
//
// A storage node keeps a slot's trees -- every node, the compact layers or the roots -- and proves every period from the touched blocks
// alone; nothing on that path reads the rest of the slot.  A scrub re-reads the selected slots from the dataset's source and hashes them
// exactly as the compact / roots-only builds do, batch by batch through the batch loop (batch_loop.hpp; DESIGN.md, "The batch loop").
// Where the build copies out what it keeps, the scrub compares instead: the builder's SlotsDone hook -- on the stream the batch's layer
// passes ran on -- launches k_scrub_compare over the fresh layer and the kept one (the fresh layer never leaves the device) and downloads
// one count per 4096 rows into pinned memory.  When batch k's node buffer is handed to batch k + 2 the host reads batch k's counts and
// downloads bitmap words only for tiles with a mismatch; batches are decoded in order, so the report comes out sorted by (item, row)
// with no sort anywhere.
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

// One run of items through the batch loop, shared by scrub_items (one dataset) and cp2_datasets_scrub_many (the slots of many datasets
// as one run of items).  Two things differ between them, and nothing else:
//   the ITEM source   item i is unit item0 + i of `src` (slot files "<base><k>.dat" or the fake source), or -- `src` has a name table,
//                     item0 is 0 -- the whole file names[i];
//   the KEPT source   the kept layer of item i starts at base + i * stride * 32, or -- an address table -- at the device address
//                     addr[i].  A batch's slice of the table goes into one of two pinned host tables, is uploaded to one of two device
//                     tables on the stream the compare runs on, just before it, and is read by k_scrub_compare_many; table b is
//                     rewritten for batch k + 2 only after batch k's event, like node buffer b: a table outlives its copy.
// Mismatches come out as (item0 + i, row) pairs in order, at most `cap`; *n_bad counts all.  item_counts (may be null; n_items entries,
// zeroed by the caller) receives the mismatches of every item, complete whatever `cap` is: every tile with a mismatch is decoded then.
struct ScrubKeptSource {
  const uint8_t* base = nullptr;
  size_t stride = 0;
  const uint64_t* addr = nullptr;
};

int scrub_loop(cp2_ctx* ctx, const ItemSource& src, uint64_t item0, const ScrubKeptSource& keptsrc, uint64_t n_items, int level, size_t cap,
               std::vector<uint64_t>& bad, uint64_t* n_bad, uint64_t* item_counts, size_t* n_batches = nullptr) {
  const uint8_t* kept = keptsrc.base;
  const uint64_t* addr = keptsrc.addr;
  const size_t kstride = addr ? 0 : keptsrc.stride;
  *n_bad = 0;
  if (n_items == 0) return CP2_OK;
  if ((!kept && !addr) || src.cell_size == 0 || src.block_size < src.cell_size) return CP2_ERR_INVALID;
  if (src.names && (!src.from_file || src.n_names != n_items || item0 != 0)) return CP2_ERR_INVALID;
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const size_t nblocks = src.n_cells / (src.block_size / src.cell_size);
  const size_t rows = level == CP2_SCRUB_CELL ? src.n_cells : (level == CP2_SCRUB_BLOCK ? nblocks : 1);
  if (rows == 0 || (!addr && kstride < rows)) return CP2_ERR_INVALID;
  const size_t batch = trees_batch_items(ctx, src.cell_size, src.block_size, src.n_cells, n_items);   // as the compact build cuts them
  const size_t groups = cp2k::scrub_groups(batch * rows);
  const int n_bufs = n_items > batch ? 2 : 1;
  DevBuf d_bits[2], d_counts[2];               // (declared before the device: they go after its scratch has drained the streams)
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
  // the builder calls this once, with every slot of the batch, on the stream its layer passes ran on (group 0: one pass at the end)
  const auto compare = [&](const BatchStep& s, cp2_slot_trees* t, size_t a, size_t z, hipStream_t ls) -> int {
    const size_t b = (size_t)s.b, n = s.n;
    if (a != 0 || z != n) { ctx->err = "scrub: a batch's layers were built in parts"; return CP2_ERR_INVALID; }
    const size_t off = level == CP2_SCRUB_CELL ? t->boff[0] : (level == CP2_SCRUB_BLOCK ? t->toff[0] : t->toff.back());
    const size_t fstride = level == CP2_SCRUB_CELL ? t->n_cells : (level == CP2_SCRUB_BLOCK ? t->tsizes[0] : 1);
    if (addr) {
      CP2_HIP(ctx, hipMemcpyAsync(d_addr[b].p, h_addr[b].p, n * 8, hipMemcpyHostToDevice, ls));
      CP2_HIP(ctx, cp2k::launch_scrub_compare_many(t->nodes.u8() + off * 32, fstride, static_cast<const uint64_t*>(d_addr[b].p), rows, n,
                                                   static_cast<uint64_t*>(d_bits[b].p), static_cast<uint32_t*>(d_counts[b].p), ls));
    } else {
      CP2_HIP(ctx, cp2k::launch_scrub_compare(t->nodes.u8() + off * 32, fstride, kept + s.s0 * kstride * 32, kstride, rows, n,
                                              static_cast<uint64_t*>(d_bits[b].p), static_cast<uint32_t*>(d_counts[b].p), ls));
    }
    CP2_HIP(ctx, hipMemcpyAsync(h_counts[b].p, d_counts[b].p, cp2k::scrub_groups(n * rows) * 4, hipMemcpyDeviceToHost, ls));
    return CP2_OK;
  };
  size_t k = 0;
  {
    BatchDevice dev;
    CP2_TRY(dev.init(ctx));
    CP2_TRY(batch_loop(dev, "scrub", ctx->err, n_items, batch,
        [&](const BatchStep& s) -> int {   // batch k - 2 has landed: its report, then table b is free for this batch's slice
          CP2_TRY(collect(s.b));
          if (addr) std::copy(addr + s.s0, addr + s.s0 + s.n, static_cast<uint64_t*>(h_addr[s.b].p));
          return CP2_OK;
        },
        [&](const BatchStep& s, hipStream_t* tail) -> int {
          return dev.build(src, item0 + s.s0, s.n, 0, [&](cp2_slot_trees* t, size_t a, size_t z, hipStream_t ls) { return compare(s, t, a, z, ls); }, s.b, tail);
        },
        [&](const BatchStep& s, hipStream_t) -> int { pending[s.b] = {true, s.s0, s.n}; return CP2_OK; },
        [](const BatchStep&) {}, &k));
    CP2_TRY(collect((int)(k & 1)));             // the older of the two batches still pending first
    CP2_TRY(collect((int)((k + 1) & 1)));
  }
  *n_bad = total;
  if (n_batches) *n_batches = k;
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

int cp2i::scrub_items(cp2_ctx* ctx, const ItemSource& src, uint64_t item0, uint64_t n_items, int level, const uint8_t* kept, size_t kstride,
                      size_t cap, std::vector<uint64_t>& bad, uint64_t* n_bad) {
  *n_bad = 0;
  if (n_items == 0) return CP2_OK;
  if (!kept) return CP2_ERR_INVALID;
  return scrub_loop(ctx, src, item0, {kept, kstride, nullptr}, n_items, level, cap, bad, n_bad, nullptr);
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
  return scrub_items(ds->ctx, item_source_of(ds), first_slot, n, level, kept, kstride, cap, bad, n_bad);
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
  ItemSource src;                         // (its name table: `names` below, set when the class runs)
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
    ItemSource src = k.src;
    src.names = k.names.data();
    src.n_names = k.names.size();
    std::vector<uint64_t> per_item(k.names.size(), 0);
    uint64_t count = 0;
    got.clear();
    size_t batches = 0;
    CP2_TRY(scrub_loop(ctx, src, 0, {nullptr, 0, k.addr.data()}, k.names.size(), k.level, cap, got, &count, per_item.data(), &batches));
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
