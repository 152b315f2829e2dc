// Datasets and proof inputs behind the C ABI (include/codex_p2.h).
//
// Mirrors reference/nim/proof_input/src/gen_input/bn254.nim:35-79 (generateProofInput), sample/bn254.nim:16-27
// (cellIndices), merkle.nim:21-42,86-100 (merkleProof, mergeMerkleProofs), types.nim:27-37 (padMerkleProof) and
// json/bn254.nim:19-78 + json/shared.nim:17-25 (exportProofInput).  Sampling, path lookup, gathers and cell
// regeneration run on the device; what stays on the host is byte packing and text formatting.
//
// Two ways through: (1) build the dataset, then generate proof inputs for any entropy (objects with accessors);
// (2) cp2_dataset_build_streamed: the entropy is known up front, so the sampling / gather / download / JSON body of
// every finished slot overlaps the hashing of the later slots, and only the lines that need ALL slot roots
// (dataSetRoot, slotProof: gen_input/bn254.nim:49-51,72) are added at the end by cp2_dataset_export_streamed.
//
// What these routes share with proof_many.cpp and multi_gpu.cpp is not in here.  proof_export.hpp (host only, checked on the CPU):
// the refusals that mirror the reference's asserts (proof_shape_refusal), slotProof, the name of an input.json, the malloc'ed text,
// the strided formatting fan-out under cp2_proof_inputs_write_json_batch and cp2_dataset_export_streamed, and the two-stage
// generate / format pipeline (export_in_chunks) that cp2_dataset_export_proof_inputs is one call of.  fill_pipeline.hpp: the one
// reader of listed pieces of a slot file (slot_file_read_list) that every sampled-cell read on the host goes through.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "body_store.hpp"
#include "dataset_obj.hpp"
#include "json_text.hpp"
#include "proof_input_obj.hpp"
#include "trees.hpp"

using namespace cp2i;
using namespace cp2text;

// ---------------------------------------------------------------------------------------------
// dataset
// ---------------------------------------------------------------------------------------------
// struct cp2_dataset and canonical_felt: dataset_obj.hpp (shared with proof_many.cpp)

int dataset_check(const cp2_config* cfg, uint64_t first_slot, uint64_t n_local) {
  if (n_local == 0 || first_slot > cfg->n_slots || n_local > cfg->n_slots - first_slot) return CP2_ERR_INVALID;   // (no wrap-around)
  if (cfg->max_depth < 0 || cfg->max_log2_nslots < 0) return CP2_ERR_INVALID;
  if (cfg->file_base && cfg->cell_size > SLOT_FILE_MAX_CELL) return CP2_ERR_INVALID;   // slot.nim:60-61
  return CP2_OK;
}

cp2_dataset* dataset_new(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local) {
  cp2_dataset* ds = new (std::nothrow) cp2_dataset();
  if (!ds) return nullptr;
  ds->ctx = ctx;
  ds->cfg = *cfg;
  ds->from_file = cfg->file_base != nullptr;
  if (ds->from_file) ds->file_base = cfg->file_base;
  ds->cfg.file_base = nullptr;
  ds->first_slot = first_slot;
  ds->n_local = n_local;
  return ds;
}

ItemSource cp2i::item_source_of(const cp2_dataset* ds) {
  return {ds->from_file, ds->file_base, ds->cfg.seed, ds->cfg.cell_size, ds->cfg.block_size, ds->cfg.n_cells, 1};
}

static int dataset_build_trees(cp2_dataset* ds, size_t group, const SlotsDone& done) {
  return build_items(ds->ctx, item_source_of(ds), ds->first_slot, ds->n_local, group, done, &ds->trees);
}

// the device buffer holding the roots of the local slots (n_local x 32 bytes)
const void* dataset_roots_dev(const cp2_dataset* ds) {
  if (ds->trees) return cp2_slot_trees_roots_dev(ds->trees);
  if (ds->tree_mode == 2) return ds->compact.u8() + ds->coff.back() * 32;   // the last layer: one root per local slot
  return ds->local_roots.p;
}

// the trees of `n` local slots starting at local index `s0`, in pooled scratch (roots-only datasets: batches of the build, and
// the one slot a proof input is made for)
static int dataset_transient_trees(const cp2_dataset* ds, size_t s0, size_t n, cp2_slot_trees** out) {
  return build_items(ds->ctx, item_source_of(ds), ds->first_slot + s0, n, 0, nullptr, out, true);
}

// bytes of the compact part (block roots and up) of n_slots slot trees
size_t compact_bytes(const cp2_config& c, size_t n_slots) {
  size_t per_slot = 0;
  for (size_t m : layer_sizes_of(c.n_cells / (c.block_size / c.cell_size))) per_slot += m;
  return n_slots * per_slot * 32;
}

// What of its trees does this dataset keep?  1 every node, 2 the compact part, 0 the roots.  The caller's word (cp2_set_keep_trees /
// CODEX_P2_KEEP_TREES), else the most that fits: a buffer must leave room for the builders' staging (two 2 GiB chunks), the batch in
// flight and some slack in what the device has free right now -- a SNAPSHOT (device_free_bytes: hipMemGetInfo, capped by
// CODEX_P2_MEM_LIMIT_MB), or the allowance a cp2_multi handed this context (its share of what the device had free before the shards started).  *automatic says whether the mode was
// chosen here (then dataset_build may step down when the allocation fails after all) or named by the caller (never changed).
#define CP2_TRY_MODE(call) do { if ((call) != CP2_OK) return 1; } while (0)   /* the device does not answer: plan as if everything fits */

// Slots per batch of a transient (compact / roots-only) build: every batch loop's rule (batch_items, batch_loop.hpp)
static size_t transient_batch_slots(const cp2_ctx* ctx, const cp2_config& c, uint64_t n_local) {
  return trees_batch_items(ctx, c.cell_size, c.block_size, c.n_cells, n_local);
}

int dataset_named_mode(cp2_ctx* ctx, bool* automatic) {
  if (automatic) *automatic = false;
  int mode = ctx->keep_trees;
  if (mode < 0 && !env_keep_trees(&mode)) {
    ctx->err = "CODEX_P2_KEEP_TREES must be \"auto\", \"1\", \"2\" or \"0\"";
    return -1;
  }
  if (mode >= 0) return mode;
  if (automatic) *automatic = true;
  return -2;
}

// The automatic choice over totals: `data` bytes of slot data, `nodes_all` bytes when every node is kept, `compact_all` when the compact
// layers are, `in_flight` the node buffers of two transient batches.  One dataset (dataset_tree_mode) or the sum over the datasets of one
// cp2_datasets_build_many call (build_many.cpp), which share one staging and one pair of batches.
int dataset_mode_that_fits(cp2_ctx* ctx, unsigned __int128 data, unsigned __int128 nodes_all, unsigned __int128 compact_all,
                           unsigned __int128 in_flight) {
  if (const char* t = std::getenv("CODEX_P2_TEST_OPTIMISTIC"))   // test-only: start at "every node" without looking, so that the step-down chain is what finds the mode that fits
    if (*t == '1') return 1;
  size_t free_b = ctx->mem_allowance;
  if (!free_b) CP2_TRY_MODE(device_free_bytes(&free_b));
  // What a build holds at its peak: what it keeps + the builders' staging (two chunks of at most `stage_bytes`, never more than the
  // data itself) + for the transient modes the node buffers of two batches in flight + headroom (sampling scratch, the dataset tree)
  typedef unsigned __int128 u128;
  const u128 staging = 2 * std::min<u128>(data, ctx->stage_bytes), headroom = std::min<u128>(data, (u128)1 << 30);
  const u128 room = (u128)free_b * 9 / 10;
  if (nodes_all + staging + headroom <= room) return 1;
  if (compact_all + in_flight + staging + headroom <= room) return 2;
  return 0;
}

static int dataset_tree_mode(cp2_ctx* ctx, const cp2_config& c, uint64_t n_local, bool* automatic = nullptr) {
  const int named = dataset_named_mode(ctx, automatic);
  if (named != -2) return named;
  typedef unsigned __int128 u128;
  const u128 data = (u128)n_local * c.n_cells * c.cell_size;
  const u128 nodes_all = (u128)trees_node_bytes(1, c.cell_size, c.block_size, c.n_cells) * n_local;
  const u128 in_flight = 2 * (u128)trees_node_bytes(transient_batch_slots(ctx, c, n_local), c.cell_size, c.block_size, c.n_cells);
  return dataset_mode_that_fits(ctx, data, nodes_all, (u128)compact_bytes(c, 1) * n_local, in_flight);
}

// compact / roots-only datasets: room for what stays of the local slots (dataset_kept_layout: the mode, the layout and its bytes)
size_t dataset_kept_layout(cp2_dataset* ds, int mode) {
  ds->tree_mode = mode;
  if (mode == 0) return ds->n_local * 32;
  const cp2_config& c = ds->cfg;
  ds->csizes = layer_sizes_of(c.n_cells / (c.block_size / c.cell_size));
  ds->coff.clear();
  size_t off = 0;
  for (size_t m : ds->csizes) { ds->coff.push_back(off); off += ds->n_local * m; }
  return off * 32;
}

static int dataset_alloc_kept(cp2_dataset* ds, int mode) {
  const size_t bytes = dataset_kept_layout(ds, mode);
  return mode == 0 ? ds->local_roots.alloc(ds->ctx, bytes) : ds->compact.alloc(ds->ctx, bytes);
}

// ... and what stays of a finished batch `t` (local slots [base, base + t->n_slots)): its roots, or its layers from the block roots up.
// Enqueued on `st` (default: the context's stream); the caller waits before the batch's nodes are used for anything else.
static int dataset_keep_from_batch(cp2_dataset* ds, const cp2_slot_trees* t, size_t base, hipStream_t st = nullptr) {
  cp2_ctx* ctx = ds->ctx;
  if (!st) st = ctx->stream;
  if (ds->tree_mode == 0) {
    CP2_HIP(ctx, hipMemcpyAsync(ds->local_roots.u8() + base * 32, cp2_slot_trees_roots_dev(t), t->n_slots * 32, hipMemcpyDeviceToDevice, st));
    return CP2_OK;
  }
  for (size_t k = 0; k < t->tsizes.size(); ++k)   // layer k of the batch's slots is contiguous, and so is its place in the dataset's layout
    CP2_HIP(ctx, hipMemcpyAsync(ds->compact.u8() + (ds->coff[k] + base * ds->csizes[k]) * 32, t->nodes.u8() + t->toff[k] * 32,
                                t->n_slots * t->tsizes[k] * 32, hipMemcpyDeviceToDevice, st));
  return CP2_OK;
}

// compact / roots-only build: batches of transient_batch_slots slots, every batch a normal builder call; what the mode keeps is copied
// out, the rest is overwritten by the batch after next.  The batches PIPELINE, from either source, through the batch loop
// (batch_loop.hpp; DESIGN.md, "The batch loop").  A batch ends with its tree-layer passes -- 22 launches for 2^22-cell slots, the top
// 16 of them one lone permutation latency each -- and the copy-out of what is kept, all on the context's THIRD stream; the next batch's
// generation and hashing go on alternating between the first two meanwhile, so the device does not drain between batches and the tail
// of a batch's last hash launch has the next batch's first one beside it.
static int dataset_build_transient(cp2_dataset* ds, int mode, bool allocated = false) {
  cp2_ctx* ctx = ds->ctx;
  const size_t batch = transient_batch_slots(ctx, ds->cfg, ds->n_local);
  if (!allocated) CP2_TRY(dataset_alloc_kept(ds, mode));
  const std::string what = mode == 2 ? "compact build" : "roots-only build";
  const ItemSource src = item_source_of(ds);
  StageTimer trace;
  {
    BatchDevice dev;
    CP2_TRY(dev.init(ctx));
    CP2_TRY(batch_loop(dev, what.c_str(), ctx->err, (size_t)ds->n_local, batch, [](const BatchStep&) -> int { return CP2_OK; },
        [&](const BatchStep& s, hipStream_t* tail) -> int { return dev.build(src, ds->first_slot + s.s0, s.n, 0, nullptr, s.b, tail); },
        [&](const BatchStep& s, hipStream_t tail) -> int { return dataset_keep_from_batch(ds, dev.batch, s.s0, tail); },   // behind the batch's layer passes
        [&](const BatchStep& s) {
          if (trace.on) std::fprintf(stderr, "[cp2 trace] %s: %zu of %llu slots enqueued\n", what.c_str(), s.s0 + s.n, (unsigned long long)ds->n_local);
        }));
  }
  trace.lap(mode == 2 ? "compact build (block layers dropped)" : "roots-only build (trees dropped)");
  return CP2_OK;
}

// One mode down after an allocation failure of an automatically chosen mode: everything of the failed attempt is gone by now (the
// dataset object, its trees), the context's cached scratch goes too, and the trace / the error text say what happened.
bool step_down(cp2_ctx* ctx, int* mode, const char* what) {
  if (*mode == 0) return false;
  const int next = *mode == 1 ? 2 : 0;
  (void)cp2_trim(ctx);
  const std::string why = ctx->err;
  if (std::getenv("CP2_TRACE"))
    std::fprintf(stderr, "[cp2 trace] %s: keeping %s did not fit after all (%s): retrying with %s\n", what, *mode == 1 ? "every node" : "the compact layers",
                 why.c_str(), next == 2 ? "the compact layers" : "the roots only");
  ctx->err.clear();
  *mode = next;
  return true;
}

// one attempt in a given mode: *out, or nothing of the attempt left
int dataset_build_in_mode(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, int mode, cp2_dataset** out) {
  *out = nullptr;
  std::unique_ptr<cp2_dataset> ds(dataset_new(ctx, cfg, first_slot, n_local));
  if (!ds) return CP2_ERR_ALLOC;
  CP2_TRY(mode == 1 ? dataset_build_trees(ds.get(), 0, nullptr) : dataset_build_transient(ds.get(), mode));
  *out = ds.release();
  return CP2_OK;
}

static int dataset_build(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, bool always_keep_trees, cp2_dataset** out) {
  if (!ctx || !cfg || !out) return CP2_ERR_INVALID;
  *out = nullptr;
  CP2_REFUSE_STUCK(ctx);
  CP2_TRY(dataset_check(cfg, first_slot, n_local));
  CP2_TRY(trees_check_geometry(cfg->cell_size, cfg->block_size, cfg->n_cells, n_local));
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  bool automatic = false;
  int mode = always_keep_trees ? 1 : dataset_tree_mode(ctx, *cfg, n_local, &automatic);
  if (mode < 0) return CP2_ERR_INVALID;
  for (;;) {
    const int st = dataset_build_in_mode(ctx, cfg, first_slot, n_local, mode, out);   // (a failed attempt holds nothing by now)
    if (st == CP2_OK) return CP2_OK;
    if (st != CP2_ERR_ALLOC || !automatic || !step_down(ctx, &mode, "dataset build")) return st;
  }
}

extern "C" int cp2_dataset_build(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local,
                                 cp2_dataset** out) try {
  return dataset_build(ctx, cfg, first_slot, n_local, false, out);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// Same as cp2_dataset_build, but what the dataset keeps of its slot trees is read from the cache when a file there is intact and
// matches the configuration AND (SlotFile source) the slot files' sizes and mtimes; built and written otherwise.
//
// Three representations can be cached -- every node ("CP2TREE3"), the compact layers or the roots ("CP2KEPT1", the mode in the
// header) -- and which one a run WANTS depends on what the device has free at that moment (dataset_tree_mode), which another
// tenant of the device can change from one run to the next.  So that such a change never costs a rebuild (hours at config 5's
// nominal size) or evicts a good cache:
//   * loading accepts ANY cached representation that is valid, describes this data and fits: the one wanted first, then the
//     smaller ones (a run that wanted every node but finds the compact layers keeps the dataset compact; CP2_TRACE says so);
//   * saving never overwrites a tree cache ("CP2TREE3") with the smaller kept form: that goes to "<cache_path>.kept" beside it,
//     and loading looks there too.
// To pin the representation, pin the mode: cp2_set_keep_trees / CODEX_P2_KEEP_TREES.
namespace {

// the kept form of `mode` (2 compact, 0 roots) from `path`: CP2_OK with *out set, CP2_ERR_IO when the file is not that, other errors as they come
int load_kept_dataset(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, int mode, const char* path, cp2_dataset** out) {
  if (!file_has_magic(path, "CP2KEPT1")) return CP2_ERR_IO;
  std::unique_ptr<cp2_dataset> ds(dataset_new(ctx, cfg, first_slot, n_local));
  if (!ds) return CP2_ERR_ALLOC;
  CP2_TRY(dataset_alloc_kept(ds.get(), mode));
  void* buf = mode == 2 ? ds->compact.p : ds->local_roots.p;
  const size_t bytes = mode == 2 ? compact_bytes(*cfg, n_local) : (size_t)n_local * 32;
  CP2_TRY(kept_load(ctx, path, kept_meta(*cfg, first_slot, n_local, ds->from_file, ds->file_base, mode), buf, bytes));
  *out = ds.release();
  return CP2_OK;
}

int save_kept_dataset(cp2_dataset* ds, const char* cache_path) {
  const cp2_config& c = ds->cfg;
  const void* buf = ds->tree_mode == 2 ? ds->compact.p : ds->local_roots.p;
  const size_t bytes = ds->tree_mode == 2 ? compact_bytes(c, ds->n_local) : (size_t)ds->n_local * 32;
  return kept_save(ds->ctx, kept_cache_path(cache_path).c_str(), kept_meta(c, ds->first_slot, ds->n_local, ds->from_file, ds->file_base, ds->tree_mode),
                   buf, bytes);
}

}  // namespace

extern "C" int cp2_dataset_build_cached(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local,
                                        const char* cache_path, cp2_dataset** out) try {
  if (!ctx || !cfg || !out || !cache_path) return CP2_ERR_INVALID;
  *out = nullptr;
  CP2_REFUSE_STUCK(ctx);
  CP2_TRY(dataset_check(cfg, first_slot, n_local));
  CP2_TRY(trees_check_geometry(cfg->cell_size, cfg->block_size, cfg->n_cells, n_local));
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  bool automatic = false;
  int mode = dataset_tree_mode(ctx, *cfg, n_local, &automatic);
  if (mode < 0) return CP2_ERR_INVALID;
  const std::string beside = std::string(cache_path) + ".kept";
  StageTimer trace;
  // ---- load: the representation wanted, else (automatic choice only) any smaller one that is there
  if (mode == 1) {
    cp2_slot_trees* t = nullptr;
    const int lst = cp2_slot_trees_load(ctx, cache_path, &t);
    if (lst == CP2_OK) {
      const bool from_file = cfg->file_base != nullptr;
      bool match = t->n_slots == n_local && t->cell_size == cfg->cell_size && t->block_size == cfg->block_size &&
                   t->n_cells == cfg->n_cells && t->first_slot == first_slot && t->units_per_slot == 1 &&
                   (from_file ? (t->src == CellSrc::File && t->file_base == cfg->file_base)
                              : (t->src == CellSrc::Fake && t->dataset_seed == cfg->seed));
      if (match) {
        cp2_dataset* ds = dataset_new(ctx, cfg, first_slot, n_local);
        if (!ds) { cp2_slot_trees_free(t); return CP2_ERR_ALLOC; }
        ds->trees = t;
        *out = ds;
        return CP2_OK;
      }
      cp2_slot_trees_free(t);
    } else if (lst == CP2_ERR_ALLOC && automatic) {
      (void)step_down(ctx, &mode, "cached build (loading the tree cache)");   // the nodes do not fit after all: what is smaller may
    }
  }
  auto size_rank = [](int md) { return md == 1 ? 2 : (md == 2 ? 1 : 0); };   // every node > compact > roots only
  for (int m2 : {2, 0}) {
    if (size_rank(m2) > size_rank(mode) || (m2 != mode && !automatic)) continue;   // never a representation larger than what fits; a named mode is taken literally
    for (const char* path : {cache_path, beside.c_str()}) {
      cp2_dataset* ds = nullptr;
      const int lst = load_kept_dataset(ctx, cfg, first_slot, n_local, m2, path, &ds);
      if (lst == CP2_OK) {
        if (trace.on && m2 != mode) std::fprintf(stderr, "[cp2 trace] the cache holds %s (this run would have kept %s): taken as it is\n",
                                                 m2 == 2 ? "the compact layers" : "the slot roots", mode == 1 ? "every node" : "the compact layers");
        trace.lap(m2 == 2 ? "compact layers loaded from the cache" : "slot roots loaded from the cache");
        *out = ds;
        return CP2_OK;
      }
      if (lst != CP2_ERR_IO && lst != CP2_ERR_ALLOC) return lst;
    }
  }
  // ---- build (stepping down when an automatic choice does not fit after all) and write what the dataset keeps
  CP2_TRY(dataset_build(ctx, cfg, first_slot, n_local, mode == 1 && !automatic, out));
  cp2_dataset* ds = *out;
  int st = ds->trees ? cp2_slot_trees_save(ds->trees, cache_path) : save_kept_dataset(ds, cache_path);
  if (st != CP2_OK) { cp2_dataset_free(ds); *out = nullptr; return st; }
  trace.lap("built and written to the cache");
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" void cp2_dataset_free(cp2_dataset* ds) { delete ds; }

extern "C" int cp2_dataset_local_roots(cp2_dataset* ds, uint8_t* out) try {
  if (!ds || !out) return CP2_ERR_INVALID;
  if (ds->trees) return cp2_slot_trees_roots(ds->trees, out);
  cp2_ctx* ctx = ds->ctx;
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  CP2_HIP(ctx, hipMemcpyAsync(out, dataset_roots_dev(ds), ds->n_local * 32, hipMemcpyDeviceToHost, ctx->stream));
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// The dataset tree over the slot roots (gen_input/bn254.nim:49-50; odd layers use keys 2 / 3) from a DEVICE buffer holding
// all n_slots roots: the layers are built in device scratch and downloaded once (slotProof and the JSON heads are made on the
// host).  The buffer may live on another device or be the tree's own root layer; it is read on the context's stream.
static int dataset_tree_from_dev(cp2_dataset* ds, const void* d_all_roots) {
  cp2_ctx* ctx = ds->ctx;
  const size_t n = ds->cfg.n_slots;
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  ds->dsizes = layer_sizes_of(n);
  const size_t total = cp2_merkle_total(n);
  ds->dlayers.assign(total * 32, 0);
  StageTimer trace;
  DevBuf d;
  CP2_TRY(d.scratch(ctx, total * 32));
  CP2_TRY(merkle_trees_dev(ctx, d_all_roots, n, 1, d.p, false));
  CP2_HIP(ctx, hipMemcpyAsync(ds->dlayers.data(), d.p, total * 32, hipMemcpyDeviceToHost, ctx->stream));
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  trace.lap("dataset tree");
  ds->have_roots = true;
  return CP2_OK;
}

extern "C" int cp2_dataset_set_roots(cp2_dataset* ds, const uint8_t* all_roots) try {
  if (!ds) return CP2_ERR_INVALID;
  cp2_ctx* ctx = ds->ctx;
  const size_t n = ds->cfg.n_slots;
  if (!all_roots) {   // single GPU: the local roots are all of them and are already on the device
    if (ds->first_slot != 0 || ds->n_local != n) return CP2_ERR_INVALID;   // roots of other ranks' slots are missing
    return dataset_tree_from_dev(ds, dataset_roots_dev(ds));
  }
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  DevBuf d;
  CP2_TRY(d.scratch(ctx, n * 32));
  CP2_HIP(ctx, hipMemcpyAsync(d.p, all_roots, n * 32, hipMemcpyHostToDevice, ctx->stream));
  return dataset_tree_from_dev(ds, d.p);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// The same from a device buffer (what a device-to-device gather leaves behind: RCCL all-gather output, a torch tensor):
// no host copy of the roots is made on the way in.
extern "C" int cp2_dataset_set_roots_dev(cp2_dataset* ds, const void* d_all_roots) try {
  if (!ds || !d_all_roots) return CP2_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(d_all_roots) & 15) return CP2_ERR_ALIGN;
  return dataset_tree_from_dev(ds, d_all_roots);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

int cp2i::dataset_own_roots_in_place(cp2_dataset* ds, bool* ok) {
  *ok = false;
  if (!ds->have_roots) return CP2_ERR_INVALID;
  std::vector<uint8_t> own(ds->n_local * 32);
  CP2_TRY(cp2_dataset_local_roots(ds, own.data()));
  *ok = std::memcmp(own.data(), &ds->dlayers[ds->first_slot * 32], own.size()) == 0;   // layer 0 of the dataset tree = all slot roots
  return CP2_OK;
}

extern "C" const void* cp2_dataset_local_roots_dev(const cp2_dataset* ds) { return ds ? dataset_roots_dev(ds) : nullptr; }
extern "C" int cp2_dataset_keeps_trees(const cp2_dataset* ds) { return !ds ? 0 : (ds->trees ? 1 : ds->tree_mode); }

extern "C" int cp2_dataset_copy_local_roots_dev(cp2_dataset* ds, void* d_out) try {
  if (!ds || !d_out) return CP2_ERR_INVALID;
  cp2_ctx* ctx = ds->ctx;
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  CP2_HIP(ctx, hipMemcpyAsync(d_out, dataset_roots_dev(ds), ds->n_local * 32, hipMemcpyDeviceToDevice, ctx->stream));
  return CP2_OK;
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_dataset_range(const cp2_dataset* ds, uint64_t* first_slot, uint64_t* n_local) {
  if (!ds) return CP2_ERR_INVALID;
  if (first_slot) *first_slot = ds->first_slot;
  if (n_local) *n_local = ds->n_local;
  return CP2_OK;
}

extern "C" cp2_ctx* cp2_dataset_ctx(const cp2_dataset* ds) { return ds ? ds->ctx : nullptr; }

extern "C" int cp2_dataset_root(cp2_dataset* ds, uint8_t out[32]) try {
  if (!ds || !out) return CP2_ERR_INVALID;
  if (!ds->have_roots) CP2_TRY(cp2_dataset_set_roots(ds, nullptr));
  std::memcpy(out, &ds->dlayers[ds->dlayers.size() - 32], 32);
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// ---------------------------------------------------------------------------------------------
// sampling + gathers on the device, results in pinned host memory
// ---------------------------------------------------------------------------------------------
namespace {

// device scratch of one sampling pass over up to `cap` (slot, counter) pairs
struct SampleDev {
  DevBuf entropy, slots, idx, gcell, rows, paths, leaves, cells;
  size_t cap = 0;
  int init(cp2_ctx* ctx, size_t cap_items, size_t ns, size_t md, size_t cs, bool need_cells) {
    cap = cap_items * ns;
    CP2_TRY(entropy.scratch(ctx, 32));
    CP2_TRY(slots.scratch(ctx, std::max<size_t>(cap_items, 1) * 8));
    CP2_TRY(idx.scratch(ctx, std::max<size_t>(cap, 1) * 8));
    CP2_TRY(gcell.scratch(ctx, std::max<size_t>(cap, 1) * 8));
    CP2_TRY(rows.scratch(ctx, std::max<size_t>(cap * md, 1) * 8));
    CP2_TRY(paths.scratch(ctx, std::max<size_t>(cap * md, 1) * 32));
    CP2_TRY(leaves.scratch(ctx, std::max<size_t>(cap, 1) * 32));
    if (need_cells) CP2_TRY(cells.scratch(ctx, std::max<size_t>(cap * cs, 1)));
    return CP2_OK;
  }
};

// pinned host landing zone of one pass
struct SampleHost {
  PinBuf idx, paths, leaves, cells;
  hipStream_t stream = nullptr;   // downloads into these buffers are enqueued here: drained before the blocks go back to the pool
  ~SampleHost() { if (stream) (void)hipStreamSynchronize(stream); }
  int init(cp2_ctx* ctx, size_t cap_items, size_t ns, size_t md, size_t cs, bool need_cells) {
    const size_t cap = cap_items * ns;
    CP2_TRY(idx.alloc(ctx, std::max<size_t>(cap, 1) * 8));
    CP2_TRY(paths.alloc(ctx, std::max<size_t>(cap * md, 1) * 32));
    CP2_TRY(leaves.alloc(ctx, std::max<size_t>(cap, 1) * 32));
    if (need_cells) CP2_TRY(cells.alloc(ctx, std::max<size_t>(cap * cs, 1)));
    return CP2_OK;
  }
};

// Enqueue on `st`: cellIndices for n_items slots (explicit batch-local list `h_slots`, or the range starting at slot0),
// path rows, the path gather, the regeneration / gather of the sampled cells (device-resident sources), and the
// downloads into `host`.  Nothing is synchronised.  d.entropy must already hold the entropy.
int enqueue_sampling(cp2_slot_trees* t, const cp2k::TreeGeom& g, SampleDev& d, SampleHost& host, const uint64_t* h_slots, uint64_t slot0,
                     size_t n_items, size_t ns, size_t md, bool fetch_cells, hipStream_t st) {
  cp2_ctx* ctx = t->ctx;
  const size_t total = n_items * ns, cs = t->cell_size;
  if (total == 0) return CP2_OK;
  host.stream = st;
  const uint64_t* d_slots = nullptr;
  if (h_slots) {
    CP2_HIP(ctx, hipMemcpyAsync(d.slots.p, h_slots, n_items * 8, hipMemcpyHostToDevice, st));
    d_slots = static_cast<const uint64_t*>(d.slots.p);
  }
  uint64_t* idx = static_cast<uint64_t*>(d.idx.p);
  uint64_t* gcell = static_cast<uint64_t*>(d.gcell.p);
  uint64_t* rows = static_cast<uint64_t*>(d.rows.p);
  CP2_HIP(ctx, cp2k::launch_sample_paths(g, t->nodes.p, d.entropy.p, d_slots, slot0, n_items, (uint32_t)ns, (uint32_t)md, idx, gcell, rows, st));
  CP2_HIP(ctx, cp2k::launch_gather_rows(t->nodes.p, rows, total * md, 32, d.paths.p, st));
  CP2_HIP(ctx, hipMemcpyAsync(host.idx.p, idx, total * 8, hipMemcpyDeviceToHost, st));
  CP2_HIP(ctx, hipMemcpyAsync(host.paths.p, d.paths.p, total * md * 32, hipMemcpyDeviceToHost, st));
  // the sampled cells' own hashes (leafValue of the merged proof, merkle.nim:86-100): layer 0 rows are slot * n_cells + cell
  CP2_HIP(ctx, cp2k::launch_gather_rows(t->nodes.p, gcell, total, 32, d.leaves.p, st));
  CP2_HIP(ctx, hipMemcpyAsync(host.leaves.p, d.leaves.p, total * 32, hipMemcpyDeviceToHost, st));
  if (!fetch_cells) return CP2_OK;   // host-side sources: the caller reads the sampled cells itself
  if (t->src != CellSrc::Fake) return CP2_ERR_INVALID;   // a dataset's trees are Fake or File (dataset_build_trees, the match test of cached trees)
  CP2_HIP(ctx, cp2k::launch_gen_fake_cells(cp2_slot_seed(t->dataset_seed, t->units_per_slot > 1 ? 0 : t->first_slot), t->n_cells, 0, gcell, total, cs,
                                           d.cells.p, st, t->units_per_slot, t->first_slot));
  CP2_HIP(ctx, hipMemcpyAsync(host.cells.p, d.cells.p, total * cs, hipMemcpyDeviceToHost, st));
  return CP2_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// proof input
// ---------------------------------------------------------------------------------------------
// BatchStore and struct cp2_proof_input: proof_input_obj.hpp (shared with verify.cpp)

// The sampled cells of `n` slots of slot-file trees (slotLoadCellData, slot.nim:57-68): cells idx[r * ns .. + ns) of local slot
// local[r] into out, in that order.  A batch of proof inputs samples hundreds of thousands of cells (4096 slots x 100): the slots are
// spread over the context's fill threads, each taking a contiguous share and every slot's file read as one list.  The failure reported
// is that of the lowest slot in the list.  (A dataset's trees hold whole slots -- units_per_slot 1 -- of the Fake or the File source:
// dataset_build_trees, dataset_transient_trees and the match test of cached trees make no other.)
static int host_cells_of_slots(cp2_slot_trees* t, const uint64_t* local, const uint64_t* idx, size_t n, size_t ns, uint8_t* out) {
  cp2_ctx* ctx = t->ctx;
  const size_t cs = t->cell_size;
  if (t->src != CellSrc::File || t->units_per_slot != 1) return CP2_ERR_INVALID;
  const int threads = (int)std::min<size_t>((size_t)fill_threads(ctx), std::max<size_t>(1, n * ns / 256));
  std::vector<std::string> failed(threads);   // per worker: slot_file_error of the file it could not open or read
  on_threads(threads, n, [&](int w, size_t r) {
    const std::string fname = slot_file_name(t->file_base, t->first_slot + local[r]);
    const int e = slot_file_read_list(fname, ns, [&](size_t) { return cs; }, [&](size_t c) { return idx[r * ns + c] * cs; },
                                      [&](size_t c) { return out + (r * ns + c) * cs; });
    if (e >= 0) failed[w] = slot_file_error(fname, e);
    return e < 0;
  });
  for (const std::string& f : failed)
    if (!f.empty()) { ctx->err = f; return CP2_ERR_IO; }
  return CP2_OK;
}

// generateProofInput (gen_input/bn254.nim:35-79) for `n` slots of the dataset at once.  Every node kept: one sampling launch, one
// path gather, one cell fetch for all of them, here.  Compact: the n slots are n requests to the pass of proof_many.cpp
// (cp2i::prove_requests: the top of every path from the stored layers, the bottom from the touched blocks, rebuilt and checked
// against their stored roots), in chunks whose touched blocks fit the staging chunk (CODEX_P2_STAGE_MB).  Roots only: slot by slot.
extern "C" int cp2_proof_inputs_generate_batch(cp2_dataset* ds, const uint64_t* slot_idx, size_t n, const uint8_t entropy_in[32],
                                               cp2_proof_input** out) try {
  if (!ds || !entropy_in || (n && (!slot_idx || !out))) return CP2_ERR_INVALID;
  uint8_t entropy[32];
  canonical_felt(entropy_in, entropy);
  for (size_t i = 0; i < n; ++i) out[i] = nullptr;
  if (n == 0) return CP2_OK;
  const cp2_config& cfg = ds->cfg;
  cp2_ctx* ctx = ds->ctx;
  for (size_t i = 0; i < n; ++i)
    if (slot_idx[i] < ds->first_slot || slot_idx[i] >= ds->first_slot + ds->n_local) return CP2_ERR_INVALID;
  const std::string refusal = proof_shape_refusal(cfg, config_slot_tree_depth(cfg), config_dataset_tree_depth(cfg));
  if (!refusal.empty()) { ctx->err = refusal; return CP2_ERR_INVALID; }
  if (!ds->trees && ds->tree_mode == 2) {                               // compact dataset: stored upper layers + the touched blocks
    if (!ds->have_roots) CP2_TRY(cp2_dataset_set_roots(ds, nullptr));
    std::vector<cp2_dataset*> same(n, ds);
    std::vector<uint8_t> entropies(n * 32);
    for (size_t i = 0; i < n; ++i) std::memcpy(&entropies[i * 32], entropy, 32);
    return prove_requests(ctx, same.data(), slot_idx, entropies.data(), n, 0, false, out);
  }
  if (!ds->trees && n > 1) {                                            // roots-only dataset: one slot, one rebuilt tree, at a time
    for (size_t i = 0; i < n; ++i) {
      int st = cp2_proof_inputs_generate_batch(ds, slot_idx + i, 1, entropy_in, out + i);
      if (st != CP2_OK) {
        for (size_t j = 0; j < i; ++j) { delete out[j]; out[j] = nullptr; }
        return st;
      }
    }
    return CP2_OK;
  }
  // the trees the paths come from: the dataset's own, or (roots-only) the tree of this one slot, rebuilt in pooled scratch
  cp2_slot_trees* t = ds->trees;
  struct Transient { cp2_slot_trees* t = nullptr; ~Transient() { cp2_slot_trees_free(t); } } transient;
  if (!t) {
    CP2_HIP(ctx, hipSetDevice(ctx->device));
    CP2_TRY(dataset_transient_trees(ds, (size_t)(slot_idx[0] - ds->first_slot), 1, &transient.t));
    t = transient.t;
    // slotRoot, slotProof and dataSetRoot come from the STORED roots; indices, paths and cells from the tree just rebuilt: the two must
    // be the same slot.  A slot file that changed since the build (or since the cache was written) is an I/O error, like the compact
    // mode's block check, never an input.json over mixed data.
    uint8_t rebuilt[32], stored[32];
    CP2_TRY(cp2_slot_trees_roots(t, rebuilt));
    CP2_HIP(ctx, hipMemcpyAsync(stored, static_cast<const uint8_t*>(dataset_roots_dev(ds)) + (slot_idx[0] - ds->first_slot) * 32, 32, hipMemcpyDeviceToHost, ctx->stream));
    CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (std::memcmp(rebuilt, stored, 32) != 0) {
      ctx->err = "slot " + std::to_string(slot_idx[0]) + " does not hash to its stored root (slot data changed since the build?)";
      return CP2_ERR_IO;
    }
  }
  const uint64_t local_base = ds->trees ? ds->first_slot : slot_idx[0];  // index inside `t` = slot index - local_base
  if (!ds->have_roots) CP2_TRY(cp2_dataset_set_roots(ds, nullptr));
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const size_t ns = cfg.n_samples, md = (size_t)cfg.max_depth, cs = cfg.cell_size, total = n * ns;

  StageTimer trace;
  auto store = std::make_shared<BatchStore>();
  const bool dev_cells = t->src == CellSrc::Fake;   // regenerated on the device; slot files are read on the host
  if (total) {
    cp2k::TreeGeom g;
    trees_geom(t, &g);
    std::vector<uint64_t> local(n);
    for (size_t i = 0; i < n; ++i) local[i] = slot_idx[i] - local_base;
    SampleDev dev;
    SampleHost host;
    CP2_TRY(dev.init(ctx, n, ns, md, cs, dev_cells));
    CP2_TRY(host.init(ctx, n, ns, md, cs, dev_cells));
    CP2_HIP(ctx, hipMemcpyAsync(dev.entropy.p, entropy, 32, hipMemcpyHostToDevice, ctx->stream));
    CP2_TRY(enqueue_sampling(t, g, dev, host, local.data(), 0, n, ns, md, dev_cells, ctx->stream));
    CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    trace.lap("sampling + gathers + downloads");
    store->idx.swap(host.idx);
    store->paths.swap(host.paths);
    store->leaves.swap(host.leaves);
    if (dev_cells) {
      store->cells.swap(host.cells);
    } else {
      store->cells_heap.resize(total * cs);
      CP2_TRY(host_cells_of_slots(t, local.data(), static_cast<const uint64_t*>(store->idx.p), n, ns, store->cells_heap.data()));
      trace.lap("cells read on the host");
    }
  }
  const uint8_t* cells = dev_cells ? store->cells.u8() : store->cells_heap.data();
  // ---- split
  std::vector<ProofItem> items(n);
  for (size_t i = 0; i < n; ++i) items[i] = {ds, slot_idx[i], entropy, out + i};
  CP2_TRY(proof_inputs_from_store(items.data(), n, store, cells));
  trace.lap("split into proof inputs");
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_proof_input_generate(cp2_dataset* ds, uint64_t slot_idx, const uint8_t entropy[32], cp2_proof_input** out) try {
  if (!out) return CP2_ERR_INVALID;
  return cp2_proof_inputs_generate_batch(ds, &slot_idx, 1, entropy, out);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" void cp2_proof_input_free(cp2_proof_input* p) { delete p; }

extern "C" int cp2_proof_input_roots(const cp2_proof_input* p, uint8_t dataset_root[32], uint8_t slot_root[32], uint8_t entropy[32]) try {
  if (!p) return CP2_ERR_INVALID;
  if (dataset_root) std::memcpy(dataset_root, p->dataset_root, 32);
  if (slot_root) std::memcpy(slot_root, p->slot_root, 32);
  if (entropy) std::memcpy(entropy, p->entropy, 32);
  return CP2_OK;
} catch (...) {
  return CP2_ERR_INVALID;
}
extern "C" size_t cp2_proof_input_nsamples(const cp2_proof_input* p) { return p ? p->n_samples : 0; }
extern "C" const uint64_t* cp2_proof_input_cell_indices(const cp2_proof_input* p) { return p ? p->indices : nullptr; }
extern "C" const uint8_t* cp2_proof_input_cell_data(const cp2_proof_input* p) { return p ? p->cell_data : nullptr; }
extern "C" const uint8_t* cp2_proof_input_merkle_paths(const cp2_proof_input* p) { return p ? p->paths : nullptr; }
extern "C" const uint8_t* cp2_proof_input_slot_proof(const cp2_proof_input* p) { return p ? p->slot_proof.data() : nullptr; }
extern "C" const uint8_t* cp2_proof_input_leaf_hashes(const cp2_proof_input* p) { return p ? p->leaves : nullptr; }

// A proof input assembled from caller arrays (what the Nim shim's exportProofInputBN254 holds: a SlotProofInput[Hash]
// value, types.nim:52-60), so that the byte-exact writer below can be used on it.  Everything is copied.
extern "C" int cp2_proof_input_create(const cp2_config* cfg, uint64_t slot_idx, const uint8_t dataset_root[32], const uint8_t entropy[32],
                                      const uint8_t slot_root[32], const uint8_t* slot_proof, size_t n_samples, const uint64_t* cell_indices,
                                      const uint8_t* cell_data, const uint8_t* merkle_paths, const uint8_t* leaf_hashes,
                                      cp2_proof_input** out) try {
  if (!cfg || !dataset_root || !entropy || !slot_root || !out) return CP2_ERR_INVALID;
  if (cfg->max_depth < 0 || cfg->max_log2_nslots < 0 || (cfg->max_log2_nslots && !slot_proof)) return CP2_ERR_INVALID;
  if (n_samples && (!cell_data || !merkle_paths)) return CP2_ERR_INVALID;
  *out = nullptr;
  std::unique_ptr<cp2_proof_input> p(new cp2_proof_input());
  p->cfg = *cfg;
  p->cfg.file_base = nullptr;
  p->cfg.n_samples = n_samples;
  p->slot_idx = slot_idx;
  std::memcpy(p->dataset_root, dataset_root, 32);
  canonical_felt(entropy, p->entropy);   // a field element in the reference (types/bn254.nim:21): stored and printed as its residue, like the generate paths
  std::memcpy(p->slot_root, slot_root, 32);
  p->slot_proof.assign(slot_proof, slot_proof + (size_t)cfg->max_log2_nslots * 32);
  p->n_samples = n_samples;
  auto store = std::make_shared<BatchStore>();
  const size_t md = (size_t)cfg->max_depth, cs = cfg->cell_size;
  const size_t o_idx = 0, o_cells = o_idx + n_samples * 8, o_paths = o_cells + n_samples * cs, o_leaves = o_paths + n_samples * md * 32;
  store->heap.assign(o_leaves + n_samples * 32 + 8, 0);
  uint8_t* h = store->heap.data();
  if (n_samples) {
    if (cell_indices) std::memcpy(h + o_idx, cell_indices, n_samples * 8);
    std::memcpy(h + o_cells, cell_data, n_samples * cs);
    std::memcpy(h + o_paths, merkle_paths, n_samples * md * 32);
    if (leaf_hashes) std::memcpy(h + o_leaves, leaf_hashes, n_samples * 32);
  }
  p->store = store;
  p->indices = reinterpret_cast<const uint64_t*>(h + o_idx);   // the vector's storage is 16-byte aligned
  p->cell_data = h + o_cells;
  p->paths = h + o_paths;
  p->leaves = leaf_hashes ? h + o_leaves : nullptr;
  *out = p.release();
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// ---- JSON: the byte-exact formatter lives in json_text.hpp (cp2text::text_head / text_body) -----------------------------
namespace {

int write_parts(const char* path, const std::string& a, const std::string& b) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return CP2_ERR_IO;
  size_t w = std::fwrite(a.data(), 1, a.size(), f) + (b.empty() ? 0 : std::fwrite(b.data(), 1, b.size(), f));
  int rc = std::fclose(f);
  return (w == a.size() + b.size() && rc == 0) ? CP2_OK : CP2_ERR_IO;
}

// head, then the stored body of local slot s (resident or spilled)
int write_head_and_body(const char* path, const std::string& head, const BodyStore& bodies, size_t s) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return CP2_ERR_IO;
  int st = std::fwrite(head.data(), 1, head.size(), f) == head.size() ? CP2_OK : CP2_ERR_IO;
  if (st == CP2_OK) st = bodies.write_to(s, f);
  if (std::fclose(f) != 0 && st == CP2_OK) st = CP2_ERR_IO;
  return st;
}

}  // namespace

static void proof_input_text(const cp2_proof_input* p, std::string& s) {
  s.clear();
  s.reserve(body_bound(p->cfg, p->n_samples) + head_bound(p->cfg));
  text_head(s, p->cfg, p->slot_idx, p->dataset_root, p->entropy, p->slot_root, p->slot_proof.data());
  if (p->cell_felts) text_body_felts(s, p->cfg, p->n_samples, p->cell_felts, p->paths);   // a parsed text: printed as read
  else text_body(s, p->cfg, p->n_samples, p->cell_data, p->paths);
}

extern "C" int cp2_proof_input_json(const cp2_proof_input* p, char** text, size_t* len) try {
  if (!p || !text) return CP2_ERR_INVALID;
  std::string s;
  proof_input_text(p, s);
  return text_to_malloc(s, text, len);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// Serialise (and optionally write) many proof inputs on `threads` host threads.  paths == NULL or
// paths[i] == NULL: serialise only.  total_bytes (may be NULL) receives the summed text length.
extern "C" int cp2_proof_inputs_write_json_batch(const cp2_proof_input* const* ps, size_t n, const char* const* paths,
                                                 int threads, uint64_t* total_bytes) try {
  if (n && !ps) return CP2_ERR_INVALID;
  for (size_t i = 0; i < n; ++i)
    if (!ps[i]) return CP2_ERR_INVALID;
  std::vector<std::string> text(std::min<size_t>((size_t)std::max(threads, 1), std::max<size_t>(n, 1)));   // one per formatting thread, reused from input to input
  return format_strided(n, threads, [&](int t, size_t i, uint64_t* bytes) {
    proof_input_text(ps[i], text[t]);
    *bytes += text[t].size();
    return paths && paths[i] ? write_parts(paths[i], text[t], std::string()) : CP2_OK;
  }, total_bytes);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// Proof inputs for many slots of a built dataset, generated and serialised as a two-stage pipeline (export_in_chunks,
// proof_export.hpp): while the host threads turn batch k into JSON text (and write it when dir != NULL: "<dir>/input_<slot>.json"),
// the GPU already samples and gathers batch k+1.
extern "C" int cp2_dataset_export_proof_inputs(cp2_dataset* ds, const uint64_t* slot_idx, size_t n, const uint8_t entropy[32],
                                               const char* dir, int threads, size_t batch, uint64_t* total_bytes) try {
  if (!ds || !entropy || (n && !slot_idx)) return CP2_ERR_INVALID;
  std::vector<std::string> names(dir ? n : 0);
  for (size_t i = 0; i < names.size(); ++i) names[i] = input_json_name(dir, slot_idx[i]);
  return export_in_chunks(n, batch, threads, [&](size_t b0, size_t m, cp2_proof_input** out) {
    return cp2_proof_inputs_generate_batch(ds, slot_idx + b0, m, entropy, out);
  }, [&](size_t i) { return dir ? names[i].c_str() : nullptr; }, total_bytes);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// ---------------------------------------------------------------------------------------------
// streamed build: proof-input bodies of finished slots while later slots are still hashing
// ---------------------------------------------------------------------------------------------
namespace {

struct StreamRing {
  // Fake data (depth 4): pass k being enqueued, k - 1 waiting for its group's hashing (two chunks are in flight), k - 2 landing, k - 3
  // being formatted.  Slot files (depth 8): the building thread is also what FILLS the ingestion ring, so it must never sleep on a
  // pass that has not landed yet; it hands out the passes it finds landed (a query per turn) and blocks only when this ring is full --
  // on a pass enqueued eight turns earlier, while the device runs at most four turns behind the host.  (Without sampled cells -- the
  // formatting workers read those from the slot files -- a landing buffer is a third of the fake path's.)
  static constexpr int MAX_DEPTH = 8;
  int depth = 4;
  SampleHost host[MAX_DEPTH];
  Event landed[MAX_DEPTH];                         // (after host[], which drain their stream themselves: the events go first, as they always have)
  size_t s0[MAX_DEPTH] = {}, s1[MAX_DEPTH] = {};   // slot range parked in host[r]
  // body tasks still reading host[r]: the build thread sleeps on the condition variable until a ring slot is free
  void begin(int r, size_t n) { std::lock_guard<std::mutex> lk(mu); pending[r] = n; }
  void task_done(int r) {
    std::lock_guard<std::mutex> lk(mu);
    if (--pending[r] == 0) cv.notify_all();
  }
  void wait_free(int r) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return pending[r] == 0; });
  }

 private:
  std::mutex mu;
  std::condition_variable cv;
  size_t pending[MAX_DEPTH] = {};
};

}  // namespace

// the streamed build keeping its trees as `tree_mode` says (1 every node, 2 compact, 0 roots only)
static int build_streamed_in_mode(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local,
                                  const uint8_t entropy_in[32], int threads, size_t group_slots, int tree_mode, cp2_dataset** out) {
  if (!ctx || !cfg || !out || !entropy_in) return CP2_ERR_INVALID;
  uint8_t entropy[32];
  canonical_felt(entropy_in, entropy);
  *out = nullptr;
  CP2_TRY(dataset_check(cfg, first_slot, n_local));
  CP2_TRY(trees_check_geometry(cfg->cell_size, cfg->block_size, cfg->n_cells, n_local));
  // (the dataset tree is not asked about here: the heads, slotProof among them, are made by cp2_dataset_export_streamed, which refuses then)
  const std::string refusal = proof_shape_refusal(*cfg, config_slot_tree_depth(*cfg), 0);
  if (!refusal.empty()) { ctx->err = refusal; return CP2_ERR_INVALID; }
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  if (threads < 1) threads = 1;
  const size_t ns = cfg->n_samples, md = (size_t)cfg->max_depth, cs = cfg->cell_size;
  // group: slots per layer pass / sampling pass.  Default: what fills the fake builder's staging chunk (2 GiB), at least 1.
  if (group_slots == 0) group_slots = std::max<size_t>(1, ctx->stage_bytes / std::max<size_t>(1, cfg->n_cells * cs));
  group_slots = std::min<size_t>(group_slots, n_local);

  std::unique_ptr<cp2_dataset> ds(dataset_new(ctx, cfg, first_slot, n_local));
  if (!ds) return CP2_ERR_ALLOC;
  ds->bodies.init(ctx, n_local);
  std::memcpy(ds->prep_entropy, entropy, 32);
  const bool from_file = ds->from_file;
  const cp2_config cfgv = ds->cfg;
  const std::string file_base = ds->file_base;

  hipStream_t aux = nullptr;                                   // the sampling / download stream (the context's third)
  CP2_TRY(aux_stream(ctx, &aux, 2));
  SampleDev dev;
  StreamRing ring;
  CP2_TRY(dev.init(ctx, group_slots, ns, md, cs, !from_file));
  ring.depth = from_file ? StreamRing::MAX_DEPTH : 4;
  for (int r = 0; r < ring.depth; ++r) {
    CP2_TRY(ring.host[r].init(ctx, group_slots, ns, md, cs, !from_file));
    CP2_TRY(ring.landed[r].create(ctx));
  }
  CP2_HIP(ctx, hipMemcpyAsync(dev.entropy.p, entropy, 32, hipMemcpyHostToDevice, aux));
  Event trees_ready;
  CP2_TRY(trees_ready.create(ctx));

  std::atomic<int> task_status{CP2_OK};
  std::mutex io_mu;
  std::string io_error;         // first slot file a formatting worker could not open or read
  cp2_dataset* dsp = ds.get();
  size_t n_groups = 0;          // sampling passes enqueued so far
  size_t consumed = 0;          // passes whose body tasks have been handed to the workers
  cp2k::TreeGeom geom;
  bool have_geom = false;
  size_t slot_base = 0;         // roots-only build: dataset-local index of the first slot of the batch being built
  StageTimer trace;
  {
    Workers pool(threads, 10);  // declared last: joins before anything above is destroyed.  Niced: the bodies are needed at the end, the device is fed now

    // hand the body tasks of pass `k` to the workers once its downloads have landed
    auto consume = [&](size_t k) -> int {
      const int r = (int)(k % (size_t)ring.depth);
      CP2_HIP(ctx, hipEventSynchronize(ring.landed[r]));
      const size_t a = ring.s0[r], b = ring.s1[r];
      ring.begin(r, b - a);
      for (size_t s = a; s < b; ++s) {
        pool.submit([&, s, a, r] {
          try {
            const uint8_t* paths = ring.host[r].paths.u8() + (s - a) * ns * md * 32;
            const uint64_t* idx = static_cast<const uint64_t*>(ring.host[r].idx.p) + (s - a) * ns;
            static thread_local std::string body;   // worst-case sized once per worker; the store keeps an exact-size copy
            body.clear();
            body.reserve(body_reserve(cfgv, ns));
            bool have = true;
            if (from_file) {      // sampled cells straight from the slot file (slot.nim:57-68)
              std::vector<uint8_t> cells(ns * cs);
              const std::string fname = slot_file_name(file_base, first_slot + s);
              const int err = slot_file_read_list(fname, ns, [&](size_t) { return cs; }, [&](size_t c) { return idx[c] * cs; },
                                                  [&](size_t c) { return &cells[c * cs]; });
              if (err >= 0) {   // reported like the classic path ("cannot open / cannot read <file>"); no body for this slot
                task_status.store(CP2_ERR_IO);
                std::lock_guard<std::mutex> lk(io_mu);
                if (io_error.empty()) io_error = slot_file_error(fname, err);
                have = false;
              } else {
                text_body(body, cfgv, ns, cells.data(), paths);
              }
            } else {
              text_body(body, cfgv, ns, ring.host[r].cells.u8() + (s - a) * ns * cs, paths);
            }
            if (have && dsp->bodies.put(s, body) != CP2_OK) task_status.store(CP2_ERR_IO);   // the store names the path (bodies.error)
          } catch (...) {
            task_status.store(CP2_ERR_ALLOC);
          }
          ring.task_done(r);
        });
      }
      return CP2_OK;
    };

    // the builders call this each time the trees of slots [a, b) are complete on the context's stream
    double hook_wait_ms = 0, hook_enqueue_ms = 0, hook_handout_ms = 0;   // CP2_TRACE: where the hook's time goes (it runs on the building thread)
    auto clock_ms = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    SlotsDone on_done = [&](cp2_slot_trees* t, size_t a, size_t b, hipStream_t tree_stream) -> int {
      if (!have_geom) { trees_geom(t, &geom); have_geom = true; }
      for (size_t g0 = a; g0 < b; g0 += group_slots) {
        const size_t g1 = std::min(b, g0 + group_slots);
        const size_t k = n_groups;
        const int r = (int)(k % (size_t)ring.depth);
        const double h0 = trace.on ? clock_ms() : 0;
        // ring slot r was last used by pass k - DEPTH: its tasks must have been handed out and finished
        while (consumed + (size_t)ring.depth <= k) { CP2_TRY(consume(consumed)); ++consumed; }
        ring.wait_free(r);
        const double h1 = trace.on ? clock_ms() : 0;
        CP2_HIP(ctx, hipEventRecord(trees_ready, tree_stream));   // the group's layer passes end on one of the two hashing streams
        CP2_HIP(ctx, hipStreamWaitEvent(aux, trees_ready, 0));
        CP2_TRY(enqueue_sampling(t, geom, dev, ring.host[r], nullptr, g0, g1 - g0, ns, md, !from_file, aux));
        CP2_HIP(ctx, hipEventRecord(ring.landed[r], aux));
        ring.s0[r] = slot_base + g0;                           // dataset-local slot indices (bodies, file names); g0 counts inside `t`
        ring.s1[r] = slot_base + g1;
        ++n_groups;
        const double h2 = trace.on ? clock_ms() : 0;
        // Two chunks are hashed at a time (one per hashing stream), so the pass before this one still waits for its group's
        // hashing: waiting for it here would keep the builder from enqueueing the next chunk until then.  The pass before THAT
        // has landed or is about to: hand it out.
        if (!from_file) {
          while (consumed + (stream_serial() ? 1 : 2) < n_groups) { CP2_TRY(consume(consumed)); ++consumed; }
        } else {
          // slot files: this thread fills the ingestion ring between the builder's turns and must not sleep on the device here
          // (StreamRing): only what has landed already is handed out
          while (consumed < n_groups) {
            const hipError_t q = hipEventQuery(ring.landed[consumed % (size_t)ring.depth]);
            if (q == hipErrorNotReady) { (void)hipGetLastError(); break; }
            CP2_HIP(ctx, q);
            CP2_TRY(consume(consumed));
            ++consumed;
          }
        }
        if (trace.on) { const double h3 = clock_ms(); hook_wait_ms += h1 - h0; hook_enqueue_ms += h2 - h1; hook_handout_ms += h3 - h2; }
      }
      return CP2_OK;
    };

    int st = CP2_OK;
    if (tree_mode == 1) {
      st = dataset_build_trees(dsp, group_slots, on_done);
      trace.lap("trees (sampling overlapped)");
      if (trace.on) std::fprintf(stderr, "[cp2 trace] the sampling hook over %zu passes: %.1f ms waiting for a free landing buffer, %.1f ms enqueueing, %.1f ms handing landed passes to the formatting threads\n", n_groups, hook_wait_ms, hook_enqueue_ms, hook_handout_ms);
      while (st == CP2_OK && consumed < n_groups) { st = consume(consumed); ++consumed; }
      pool.wait_idle();
      (void)hipStreamSynchronize(aux);
      trace.lap("last bodies");
    } else {
      // Compact / roots only (the nodes of all local slots do not fit the device, or the caller said so): the same pipeline over
      // batches of slots -- about 1 GiB of nodes: 4 slots of 8 GiB, a whole number of groups -- whose nodes are dropped once the
      // batch's bodies are made and what the mode keeps is copied out; roots (or compact layers) and bodies stay.
      size_t batch = transient_batch_slots(ctx, cfgv, n_local);
      batch = std::max(group_slots, batch / group_slots * group_slots);
      st = dataset_alloc_kept(dsp, tree_mode);
      {
        // The batches PIPELINE, fake data and slot files alike, through the batch loop (batch_loop.hpp).  A batch's tail -- the layer passes
        // of its last group, that group's sampling, gathers and downloads, the copy-out of what is kept: all on the third stream -- runs
        // while the next batch's generation and hashing already occupy the two hashing streams.  Node buffer b goes to batch k + 2 once
        // batch k's copy-out and last sampling have completed: the tail waits for `sampled` before the loop records its event on it.
        BatchDevice batches;
        Event sampled[2];                                        // (after the device, like its own events: gone before its scratch drains)
        const ItemSource src = item_source_of(dsp);
        const std::string what = std::string("streamed ") + (tree_mode == 2 ? "compact" : "roots-only") + " build";
        if (st == CP2_OK) st = batches.init(ctx);
        for (int i = 0; i < 2 && st == CP2_OK; ++i) st = sampled[i].create(ctx);
        if (st == CP2_OK)
          st = batch_loop(batches, "streamed build", ctx->err, (size_t)n_local, batch,
              [&](const BatchStep& s) -> int { slot_base = s.s0; have_geom = false; return CP2_OK; },   // node offsets are those of THIS batch's layout
              [&](const BatchStep& s, hipStream_t* tail) -> int { return batches.build(src, first_slot + s.s0, s.n, group_slots, on_done, s.b, tail); },
              [&](const BatchStep& s, hipStream_t tail) -> int {
                CP2_TRY(dataset_keep_from_batch(dsp, batches.batch, s.s0, tail));   // follows the batch's last layer pass on that stream
                if (hipEventRecord(sampled[s.b], aux) != hipSuccess || hipStreamWaitEvent(tail, sampled[s.b], 0) != hipSuccess) {
                  ctx->err = "streamed build: event bookkeeping failed";
                  return CP2_ERR_HIP;
                }
                // the last batch: the passes still parked go to the workers now, so that their formatting overlaps the loop's drain
                while (s.last && consumed < n_groups) { CP2_TRY(consume(consumed)); ++consumed; }
                return CP2_OK;
              },
              [&](const BatchStep& s) {
                if (trace.on) std::fprintf(stderr, "[cp2 trace] %s: %zu of %llu slots enqueued\n", what.c_str(), s.s0 + s.n, (unsigned long long)n_local);
              });
        pool.wait_idle();
      }
      trace.lap("trees + bodies, batch by batch (trees dropped)");
    }
    if (st != CP2_OK) return st;
  }
  if (task_status.load() != CP2_OK) {
    if (!io_error.empty()) ctx->err = io_error;
    else if (!ds->bodies.error.empty()) ctx->err = ds->bodies.error;
    return task_status.load();
  }
  ds->prepared = true;
  *out = ds.release();
  return CP2_OK;
}

extern "C" int cp2_dataset_build_streamed(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local,
                                          const uint8_t entropy_in[32], int threads, size_t group_slots, cp2_dataset** out) try {
  if (!ctx || !cfg || !out || !entropy_in) return CP2_ERR_INVALID;
  *out = nullptr;
  CP2_REFUSE_STUCK(ctx);
  CP2_TRY(dataset_check(cfg, first_slot, n_local));
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  bool automatic = false;
  int mode = dataset_tree_mode(ctx, *cfg, n_local, &automatic);
  if (mode < 0) return CP2_ERR_INVALID;
  for (;;) {   // the same step-down chain as cp2_dataset_build: an automatic choice that does not fit after all is retried one mode down
    const int st = build_streamed_in_mode(ctx, cfg, first_slot, n_local, entropy_in, threads, group_slots, mode, out);
    if (st != CP2_ERR_ALLOC || !automatic || !step_down(ctx, &mode, "streamed build")) return st;
  }
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// Finish the proof inputs a streamed build prepared: the dataset tree must be set (cp2_dataset_set_roots; implied when
// all slots are local).  Heads (dataSetRoot .. slotProof) are formatted and joined with the stored bodies on `threads`
// host threads; dir != NULL writes "<dir>/input_<slot>.json" for every local slot.  Text identical to cp2_proof_input_json.
extern "C" int cp2_dataset_export_streamed(cp2_dataset* ds, const char* dir, int threads, uint64_t* total_bytes) try {
  if (!ds || !ds->prepared) return CP2_ERR_INVALID;
  if (!ds->have_roots) CP2_TRY(cp2_dataset_set_roots(ds, nullptr));
  if (ds->dsizes.size() - 1 > (size_t)ds->cfg.max_log2_nslots) return CP2_ERR_INVALID;   // padMerkleProof assert
  struct Scratch { std::string head; std::vector<uint8_t> proof; };
  const size_t n = ds->n_local;
  std::vector<Scratch> scratch(std::min<size_t>((size_t)std::max(threads, 1), n));   // one per formatting thread, reused from slot to slot
  return format_strided(n, threads, [&](int t, size_t s, uint64_t* bytes) {
    std::string& head = scratch[t].head;
    const uint64_t slot = ds->first_slot + s;
    head.clear();
    fill_slot_proof(ds, slot, scratch[t].proof);
    text_head(head, ds->cfg, slot, &ds->dlayers[ds->dlayers.size() - 32], ds->prep_entropy, &ds->dlayers[slot * 32], scratch[t].proof.data());
    *bytes += head.size() + ds->bodies.size[s];
    return dir ? write_head_and_body(input_json_name(dir, slot).c_str(), head, ds->bodies, s) : CP2_OK;
  }, total_bytes);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// the full text of one prepared slot (head + body) into a malloc'ed buffer (cp2_free_buffer)
extern "C" int cp2_dataset_streamed_json(cp2_dataset* ds, uint64_t slot_idx, char** text, size_t* len) try {
  if (!ds || !ds->prepared || !text) return CP2_ERR_INVALID;
  if (slot_idx < ds->first_slot || slot_idx >= ds->first_slot + ds->n_local) return CP2_ERR_INVALID;
  if (!ds->have_roots) CP2_TRY(cp2_dataset_set_roots(ds, nullptr));
  if (ds->dsizes.size() - 1 > (size_t)ds->cfg.max_log2_nslots) return CP2_ERR_INVALID;
  std::string head;
  std::vector<uint8_t> proof;
  fill_slot_proof(ds, slot_idx, proof);
  text_head(head, ds->cfg, slot_idx, &ds->dlayers[ds->dlayers.size() - 32], ds->prep_entropy, &ds->dlayers[slot_idx * 32], proof.data());
  CP2_TRY(ds->bodies.append(slot_idx - ds->first_slot, head));
  return text_to_malloc(head, text, len);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" void cp2_free_buffer(void* p) { std::free(p); }

extern "C" int cp2_proof_input_write_json(const cp2_proof_input* p, const char* path) try {
  if (!p || !path) return CP2_ERR_INVALID;
  StageTimer trace;
  std::string s;
  proof_input_text(p, s);
  const int st = write_parts(path, s, std::string());
  trace.lap("input.json formatted + written");
  return st;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_write_circom_main(const cp2_config* cfg, const char* path) try {
  if (!cfg || !path || cfg->cell_size == 0) return CP2_ERR_INVALID;
  if (cfg->block_size % cfg->cell_size) return CP2_ERR_INVALID;
  uint64_t cpb = cfg->block_size / cfg->cell_size;
  if (!is_pow2(cpb)) return CP2_ERR_INVALID;                     // exactLog2 assert, misc.nim:25-28
  int depth = 0;
  while ((1ULL << depth) < cpb) ++depth;
  FILE* f = std::fopen(path, "wb");
  if (!f) return CP2_ERR_IO;
  std::fprintf(f, "pragma circom 2.0.0;\n");
  std::fprintf(f, "include \"sample_cells.circom\";\n");
  std::fprintf(f, "// SampleAndProven( maxDepth, maxLog2NSlots, blockTreeDepth, nFieldElemsPerCell, nSamples )\n");
  std::fprintf(f, "component main {public [entropy,dataSetRoot,slotIndex]} = SampleAndProve(%d, %d, %d, %llu, %llu);\n",
               cfg->max_depth, cfg->max_log2_nslots, depth, (unsigned long long)((cfg->cell_size + 30) / 31),
               (unsigned long long)cfg->n_samples);
  return std::fclose(f) == 0 ? CP2_OK : CP2_ERR_IO;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
