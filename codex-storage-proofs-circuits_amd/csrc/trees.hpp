// Slot-tree batch shared by slot_trees.cpp, cache_file.cpp and proof_input.cpp (not installed).
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "batch_loop.hpp"
#include "internal.hpp"
#include "kernels.hpp"
#include "fill_pipeline.hpp"   // the slot-file read rule: read_file_cell, slot_file_error
#include "cache_file.hpp"      // CellSrc; the cache files' heads, stamps and tmp-file writer (host side)

struct cp2_slot_trees {
  cp2_ctx* ctx = nullptr;
  size_t n_slots = 0, cell_size = 0, block_size = 0, n_cells = 0, cpb = 0, nblocks = 0;
  std::vector<size_t> bsizes, tsizes;   // per-tree layer sizes: block tree (cpb leaves), big tree (nblocks leaves)
  std::vector<size_t> boff, toff;       // element offsets of each layer in `nodes` (layer-major)
  cp2i::DevBuf nodes;
  // where sampled cells come from
  CellSrc src = CellSrc::Fake;
  uint64_t dataset_seed = 0, first_slot = 0;
  // Slots cut into units (several devices sharing ONE slot, multi_gpu.cpp): this batch then holds `n_slots` UNITS of `n_cells`
  // cells each, unit i being unit first_slot + i of the dataset, unit u = cells [(u % units_per_slot) * n_cells, +n_cells) of
  // slot u / units_per_slot.  1: a unit is a whole slot (everything outside multi_gpu.cpp).
  uint64_t units_per_slot = 1;
  bool pooled_nodes = false;            // node buffer from the context's scratch pool (transient batches: roots-only datasets)
  const uint8_t* d_cells = nullptr;     // not owned
  const uint8_t* h_cells = nullptr;     // not owned
  std::string file_base;
};

// An empty batch object of this geometry, and its layout: layer sizes and offsets for its n_slots, then the node buffer -- allocated
// (pooled when pooled_nodes is set), or, with borrow_from, a view of that buffer (grown from the context's scratch pool when too small).
// The builders (slot_trees.cpp) start with these; build_many.cpp makes the every-node trees of its datasets with them.
cp2_slot_trees* trees_new(cp2_ctx* ctx, size_t n_slots, size_t cell_size, size_t block_size, size_t n_cells);
int trees_layout(cp2_slot_trees* t, cp2i::DevBuf* borrow_from = nullptr);

namespace cp2i {

constexpr uint64_t NO_ROW = ~0ULL;

// Called by the builders each time the trees of slots [s0, s1) (indices inside the batch) are complete ON STREAM `st`
// (everything enqueued, nothing synchronised): the streamed proof-input path hangs its sampling / gather / download
// of those slots on that stream (the context's third) while later slots are still hashing on the other two.
using SlotsDone = std::function<int(cp2_slot_trees* t, size_t s0, size_t s1, hipStream_t st)>;

// Scratch that outlives one builder call, so that consecutive batches of a transient (compact / roots-only) build PIPELINE instead of
// draining the device between them: two staging buffers for generated cells and two node buffers used alternately.  With it
// trees_build_fake returns with its work ENQUEUED (nothing synchronised, the batch's nodes a borrowed view of nodes[node_slot]):
// the next batch's generation and hashing start on the context's two hashing streams while this batch's layer passes and
// copy-outs still run on the third.  The owner (BatchDevice below, driven by batch_loop.hpp) waits for whatever reads nodes[b] before it
// hands slot b to another batch, and drains the context's streams before the scratch goes (its destructor does).
struct BuildScratch {
  cp2_ctx* ctx = nullptr;
  DevBuf stage[2], nodes[2];
  hipStream_t tail_stream = nullptr;   // set by the builder: the stream the last batch's layer passes were enqueued on
  std::shared_ptr<void> file_pipe;     // slot files: the ingestion pipe (pinned ring, device ring, copy stream) the batches share; declared
                                       // last, so it drains and goes before the buffers above
  ~BuildScratch();
};

int trees_check_geometry(size_t cell_size, size_t block_size, size_t n_cells, size_t n_slots);
// slots cut into units_per_slot > 1 units of cells_per_unit cells: a power of two of units, each a power of two >= 2 of whole blocks
bool unit_geometry_ok(uint64_t units_per_slot, size_t cell_size, size_t block_size, size_t cells_per_unit);
// fake-data or slot-file trees; `group` = how many finished slots to batch per layer pass / callback (0: all at the end)
// units_per_slot > 1: first_slot / n_slots / n_cells count UNITS and the cells of one unit (cp2_slot_trees above)
// pooled_nodes: the node buffer comes from (and goes back to) the context's scratch pool instead of hipMalloc / hipFree
// scratch != nullptr: pipelined (BuildScratch above); the returned batch borrows scratch->nodes[node_slot] (both builders)
int trees_build_fake(cp2_ctx* ctx, uint64_t dataset_seed, uint64_t first_slot, size_t n_slots, size_t cell_size, size_t block_size,
                     size_t n_cells, size_t group, const SlotsDone& done, cp2_slot_trees** out, uint64_t units_per_slot = 1,
                     bool pooled_nodes = false, BuildScratch* scratch = nullptr, int node_slot = 0);
int trees_build_files(cp2_ctx* ctx, const std::string& base, uint64_t first_slot, size_t n_slots, size_t cell_size,
                      size_t block_size, size_t n_cells, size_t group, const SlotsDone& done, cp2_slot_trees** out,
                      uint64_t units_per_slot = 1, bool pooled_nodes = false, BuildScratch* scratch = nullptr, int node_slot = 0);
// The same over a NAME TABLE: unit i of the batch is the whole file names[i] (units_per_slot 1), whatever it is called -- the slots of
// many datasets in one batch (scrub.cpp).  One body with trees_build_files, which is the base + first-item case of it.  O_DIRECT is
// honoured as there and the slot.nim:60-61 cell-size cap applies; the MAPPED mode keys its mappings by dataset unit, which a listed
// batch does not have: it is not used, every turn goes through the ring.  The batch's file_base is empty and its first_slot 0.
// The table is names[0 .. n_names): the caller keeps it alive for the call (every fill is joined before the builder returns), so a batch
// of a longer table is a pointer into it, nothing is copied.
int trees_build_file_list(cp2_ctx* ctx, const std::string* names, size_t n_names, size_t cell_size, size_t block_size, size_t n_cells,
                          size_t group, const SlotsDone& done, cp2_slot_trees** out, bool pooled_nodes = false,
                          BuildScratch* scratch = nullptr, int node_slot = 0);
// Where a run of items comes from: item i is unit i of the fake source (`seed`) or of the slot files "<file_base><k>.dat", the units
// counted as cp2_slot_trees says (units_per_slot, n_cells per item) -- or, with a name table, the whole file names[i] (from_file,
// units_per_slot 1; the table is the caller's and outlives every call).  build_items builds items [s0, s0 + n) of it: THE call of the
// three builders above outside slot_trees.cpp, their arguments as described there.
struct ItemSource {
  bool from_file = false;
  std::string file_base;
  uint64_t seed = 0;                   // dataset seed (fake source)
  size_t cell_size = 0, block_size = 0, n_cells = 0;   // n_cells: per item
  uint64_t units_per_slot = 1;
  const std::string* names = nullptr;  // the name table, n_names entries (null: none)
  size_t n_names = 0;
};
ItemSource item_source_of(const cp2_slot_trees* t, uint64_t units_per_slot);   // the units of `t`
ItemSource item_source_of(const cp2_dataset* ds);                              // the slots of `ds`
int build_items(cp2_ctx* ctx, const ItemSource& src, uint64_t s0, size_t n, size_t group, const SlotsDone& done, cp2_slot_trees** out,
                bool pooled_nodes = false, BuildScratch* scratch = nullptr, int node_slot = 0);

// The device of the batch loop (batch_loop.hpp): the scratch, the two events "whatever reads node buffer b has completed", the drain of
// the context's streams.  A failed wait or drain clears the runtime's sticky error: the loop reports it, it must not resurface from a
// later hipGetLastError().  The events are declared after the scratch and so go first; the scratch then drains the streams before its
// buffers go, whatever path leaves the owner's scope.  What the owner keeps beside it for the batches in flight (tables, counts) is
// declared BEFORE the device and so goes after that drain.
struct BatchDevice {
  using Tail = hipStream_t;
  cp2_ctx* ctx = nullptr;
  BuildScratch scratch;
  Event landed[2];
  cp2_slot_trees* batch = nullptr;     // the batch of the current step, its nodes a view of scratch.nodes[b]: freeing it waits for nothing
  ~BatchDevice() { release(); }
  int init(cp2_ctx* c) { ctx = c; CP2_TRY(landed[0].create(c)); return landed[1].create(c); }
  int wait(int b) { return cleared(hipEventSynchronize(landed[b]) == hipSuccess); }
  int record(int b, hipStream_t tail) {
    if (hipEventRecord(landed[b], tail) == hipSuccess) return CP2_OK;
    ctx->err = "hipEventRecord failed";
    return CP2_ERR_HIP;
  }
  int drain() {                        // everything landed (a failed launch or copy shows up here)
    return cleared(hipStreamSynchronize(ctx->stream) == hipSuccess && (!ctx->aux_stream || hipStreamSynchronize(ctx->aux_stream) == hipSuccess) &&
                   (!ctx->aux2_stream || hipStreamSynchronize(ctx->aux2_stream) == hipSuccess));
  }
  void release() { cp2_slot_trees_free(batch); batch = nullptr; }
  // items [s0, s0 + n) of `src` into node buffer b, enqueued; *tail = the stream the batch's layer passes ended on (the context's third)
  int build(const ItemSource& src, uint64_t s0, size_t n, size_t group, const SlotsDone& done, int b, hipStream_t* tail) {
    const int st = build_items(ctx, src, s0, n, group, done, &batch, true, &scratch, b);
    *tail = scratch.tail_stream ? scratch.tail_stream : ctx->stream;
    return st;
  }
  static int cleared(bool ok) { if (!ok) (void)hipGetLastError(); return ok ? CP2_OK : CP2_ERR_HIP; }
};

// bytes of the node buffer of a batch of n_slots slots of this geometry (all layers, 32 bytes per node)
size_t trees_node_bytes(size_t n_slots, size_t cell_size, size_t block_size, size_t n_cells);
// items per batch of the batch loop for this geometry (batch_items, batch_loop.hpp, over the context's staging chunk)
inline size_t trees_batch_items(const cp2_ctx* ctx, size_t cell_size, size_t block_size, size_t n_cells, uint64_t n_items) {
  return batch_items(ctx->stage_bytes, trees_node_bytes(1, cell_size, block_size, n_cells), n_items);
}
void trees_geom(const cp2_slot_trees* t, cp2k::TreeGeom* g);
// node-row indices of the merged path of `cell` in slot `slot` (host twin of k_sample_paths' row arithmetic)
void path_rows(const cp2_slot_trees* t, size_t slot, uint64_t cell, size_t max_depth, uint64_t* rows);
// merged paths (padded to max_depth, + leaf hashes) of n (slot-in-batch, cell) pairs of a batch in one gather
int trees_paths_multi(cp2_slot_trees* t, const uint64_t* slot_idx, const uint64_t* cell_idx, size_t n, size_t max_depth, uint8_t* out, uint8_t* leaf_hashes);
std::string slot_file_name(const std::string& base, uint64_t slot);
bool is_pow2(uint64_t x);

// Persisted form of what a compact / roots-only dataset keeps (cache_file.cpp, beside the tree cache; its head: kept_meta, cache_file.hpp).
// kept_load fills the device buffer and returns CP2_OK only when the file is intact and describes exactly `want` (and, for the SlotFile
// source, slot files of unchanged size and mtime); anything else is CP2_ERR_IO and means "rebuild".
int kept_save(cp2_ctx* ctx, const char* path, CacheHead meta, const void* d_buf, size_t bytes);
int kept_load(cp2_ctx* ctx, const char* path, const CacheHead& want, void* d_buf, size_t bytes);

// After cp2_dataset_set_roots*: do rows [first_slot, first_slot + n_local) of the dataset tree's bottom layer hold THIS dataset's own
// slot roots?  One small download.  The multi-device exchange is verified with it (multi_gpu.cpp).
int dataset_own_roots_in_place(cp2_dataset* ds, bool* ok);

// Scrub (scrub.cpp): items (whole slots, or units of a slot cut by units_per_slot) rebuilt batch by batch (batch_loop.hpp) from their
// source, and the fresh layer of `level` (CP2_SCRUB_CELL: cell hashes, _BLOCK: block roots, _SLOT: item roots) compared on the device
// with the kept one.  The kept layer of items [item0, item0 + n) starts at `kept` (32-byte rows) with `kstride` rows per item.
// Mismatches are appended to `bad` as (item, row) pairs in that order, at most `cap` of them; *n_bad counts all.  Reads the kept
// layer only.
int scrub_items(cp2_ctx* ctx, const ItemSource& src, uint64_t item0, uint64_t n, int level, const uint8_t* kept, size_t kstride, size_t cap,
                std::vector<uint64_t>& bad, uint64_t* n_bad);
// the finest level a dataset keeps: CP2_SCRUB_CELL (every node), _BLOCK (compact) or _SLOT (roots only)
int dataset_scrub_level(const cp2_dataset* ds);
// slots [first_slot, first_slot + n) of the dataset's local range at `level` (at most dataset_scrub_level): (slot, index) pairs
int dataset_scrub(cp2_dataset* ds, uint64_t first_slot, uint64_t n, int level, size_t cap, std::vector<uint64_t>& bad, uint64_t* n_bad);

// stage timings on stderr when CP2_TRACE is set (the reference's only tracing is shell `time`, workflow/prove.sh:30-37)
bool stream_serial();   // CP2_STREAM_SERIAL=1 (A/B tooling): the streamed build hashes its groups one launch after the other, as rounds 2-4 did

struct StageTimer {
  bool on;
  double t0;
  StageTimer();
  void lap(const char* what);
};

}  // namespace cp2i
