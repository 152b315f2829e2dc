// Fill sessions behind the C ABI (include/codex_p2.h): cp2_fill_begin, cp2_fill_add, cp2_fill_missing, cp2_fill_finish, cp2_fill_free,
// their checkpoints: cp2_fill_save, cp2_fill_resume, the sessions that serve while they fill: cp2_fill_keep_nodes, cp2_fill_block_proofs,
// the adds whose paths stop at a node the session holds: cp2_fill_anchors, cp2_fill_add_anchored, and the blocks taken over from the slot
// files on the strength of those nodes: cp2_fill_adopt, and the add of groups of blocks with their multiproofs: cp2_fill_add_multi.
//
// A node that takes on a slot holds the manifest's slot root and receives the slot's network blocks from peers, in any order, each with
// its Merkle path.  cp2_blocks_verify checks such blocks and forgets the block roots it computed; a session KEEPS them.  It owns the compact
// layout of its slots (cp2_dataset, dataset_obj.hpp: the tree over the block roots, layer-major over the local slots) from the start;
// every add runs verify's data path (repair_check_with, repair.cpp) and ends in k_block_path_commit, which walks each candidate's root up
// its path and, where the slot root comes out, stores the block root into layer 0.  The host's bitmap (fill_plan.hpp) says what is
// present; the proved blocks are written into the slot files by repair's writer.  When nothing is missing, finish builds the upper
// layers with the layer kernel (one launch per layer over all slots), compares the top layer with the stated roots and hands the buffer
// to a new compact dataset: no slot byte is read or hashed a second time.
//
// A session lives for as long as its blocks take to arrive, so it can be saved at any point (cp2_fill_save: geometry, source, stated roots,
// bitmap and layer 0 under a checksum, fill_checkpoint.hpp) and resumed by a later process (cp2_fill_resume).  Resume trusts the disk only as
// far as the device has re-checked it: every block the checkpoint calls present is read back (or, fake source, regenerated), hashed and
// reduced to its block root by the builders' kernels on repair's data path, and k_block_root_recheck compares that root with the row of
// layer 0 the checkpoint kept, zeroing the row where they differ; the host clears those blocks' bits, and they are missing again.  That is
// one judge for repair_check_with and two sources: slot files go through the host-side readers of fill_checkpoint.hpp
// (fill_slot_files_cover: what each file holds; fill_read_chunk: a chunk of the read plan into a host buffer), the fake source through
// the judge's `cells` hook (repair.hpp), which generates a chunk's cells on the device where a candidate chunk would be uploaded.
//
// A session that is still filling can vouch for the blocks it holds.  A path that ends in the stated slot root proves every node on it, and
// the compact buffer has a row for each, unused until finish.  After cp2_fill_keep_nodes every add ends in k_block_path_commit_nodes, which
// stores the proved siblings and ancestors where the tree has them; the host's second bitmap (FillPlan::known) says which rows hold
// authentic nodes, and cp2_fill_block_proofs serves a present block's proof with the gather cp2_dataset_block_proofs does on a dataset.
//
// The kept nodes also shorten what a peer has to send.  A computed node that equals an authentic node proves everything below it, so a
// block whose ancestor at level a is known needs its a lowest siblings only: cp2_fill_anchors names that level per block, and
// cp2_fill_add_anchored is cp2_fill_add with packed paths of those lengths, ending in k_block_path_commit_anchored, which compares each
// walk's result with the kept row instead of the slot root.  With the lowest anchors throughout a slot takes nBlocks - 1 siblings in all.
//
// The same argument lets a session take blocks from its own disk.  cp2_fill_adopt reads the absent blocks the slot files cover (with
// fill_slot_files_cover and fill_read_chunk, then repair_check_with), keeps their fresh block roots in a buffer of the session's own,
// builds the tree above them with the kept nodes wherever there are any (k_adopt_layer, one launch per layer) and keeps every subtree
// whose computed root equals a node the session knows, the stated slot root included (k_adopt_resolve); adopt_plan.hpp holds the host side.
//
// A checkpoint can carry the kept nodes too (cp2_fill_save_nodes, format CP2FILL2, node_ckpt_plan.hpp).  cp2_fill_resume_nodes is
// cp2_fill_resume and cp2_fill_keep_nodes, after which the rows the file calls known are candidates in a buffer of their own: top-down, one
// launch per layer, k_nodes_restore_layer recomputes every known parent that has a candidate child and takes the children over where the
// parent comes out, so a resumed session knows exactly what the device has re-derived from the stated slot roots.
//
// Blocks of one slot that arrive together share the upper parts of their paths.  cp2_fill_add_multi takes them in groups, each with its
// multiproof (multiproof_plan.hpp: every node the group cannot compute, once): the candidates go down the same data path, k_multiproof_layer
// builds each group's subtree (multiproof_check, multiproofs.cpp), and k_multiproof_commit copies what the proved groups leave -- the rows
// whole paths would have left -- into the buffer; the rest of the call is the other adds' tail (fill_add_tail).
//
// Multiproofs and kept nodes together: cp2_fill_multiproof_want lays a group out against what the session knows
// (multiproof_anchor_plan.hpp: only the rows it can neither compute nor already holds), cp2_fill_block_tree_rows serves such rows by their
// place from a session that is still filling, and cp2_fill_add_multi_anchored is cp2_fill_add_multi over that layout: the kept inputs are
// gathered from the buffer into the work table, the layers run as they are, and every group's tops are compared with the rows the session
// keeps (k_multiproof_tops, k_multiproof_fold) where cp2_fill_add_multi compares one top with the stated root.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "adopt_plan.hpp"
#include "block_proof_plan.hpp"
#include "dataset_obj.hpp"
#include "fill_checkpoint.hpp"
#include "fill_plan.hpp"
#include "fill_session.hpp"
#include "multiproof_anchor_plan.hpp"
#include "multiproof_plan.hpp"
#include "node_ckpt_plan.hpp"
#include "repair.hpp"

using namespace cp2i;

static_assert(FILL_NEW == CP2_FILL_NEW && FILL_MISMATCH == CP2_FILL_MISMATCH && FILL_DUPLICATE == CP2_FILL_DUPLICATE &&
              FILL_UNWRITTEN == CP2_FILL_UNWRITTEN, "fill_plan.hpp restates the header's statuses");
static_assert(FILL_PROOF_OK == CP2_FILL_PROOF_OK && FILL_PROOF_ABSENT == CP2_FILL_PROOF_ABSENT && FILL_PROOF_PARTIAL == CP2_FILL_PROOF_PARTIAL,
              "fill_plan.hpp restates the header's proof statuses");
static_assert(ADOPT_F_KNOWN == cp2k::ADOPT_KNOWN && ADOPT_F_CAND == cp2k::ADOPT_CAND && ADOPT_F_MATCH == cp2k::ADOPT_MATCH &&
              ADOPT_F_PROVED == cp2k::ADOPT_PROVED && ADOPT_F_ADOPTED == cp2k::ADOPT_ADOPTED, "adopt_plan.hpp restates the kernels' flag bits");
static_assert(NODE_F_KNOWN == cp2k::NODE_KNOWN && NODE_F_CAND == cp2k::NODE_CAND && NODE_F_RESTORED == cp2k::NODE_RESTORED &&
              NODE_F_REJECTED == cp2k::NODE_REJECTED, "node_ckpt_plan.hpp restates the kernel's flag states");
static_assert(BLOCK_PROOF_NO_ROW == NO_ROW, "k_gather_rows zero-fills the rows the plan marks as absent");
static_assert(FILL_WRITE == CP2_REPAIR_MATCH && FILL_SKIP == CP2_REPAIR_MISMATCH && FILL_WRITE_FAILED == CP2_REPAIR_UNWRITTEN,
              "repair_write takes and leaves repair's statuses");

// (the session behind the header's opaque cp2_fill: fill_session.hpp)

namespace {

cp2_fill_session* session(void* f) { return static_cast<cp2_fill_session*>(f); }
const cp2_fill_session* session(const void* f) { return static_cast<const cp2_fill_session*>(f); }

// (a buffer handed over without a copy: hand_over, fill_session.hpp)

constexpr uint64_t WHOLE_PATHS = ~(uint64_t)0;

// siblings: what an anchored add received (of n x depth a plain add would have); WHOLE_PATHS: a plain add, whose line says nothing of it
void fill_trace(size_t n, const uint32_t* status, size_t n_new, size_t block_size, uint64_t missing, double seconds, uint64_t siblings, size_t depth) {
  if (!std::getenv("CP2_TRACE")) return;
  size_t proved = 0;
  for (size_t i = 0; i < n; ++i) proved += status[i] != FILL_MISMATCH;
  const double bytes = (double)n * (double)block_size;
  char anchored[96] = "";
  if (siblings != WHOLE_PATHS)
    std::snprintf(anchored, sizeof anchored, ", anchored: %llu sibling(s) received of %llu", (unsigned long long)siblings,
                  (unsigned long long)n * (unsigned long long)depth);
  std::fprintf(stderr, "[cp2 trace] fill add: %zu request(s), %zu proved, %zu new, %llu still missing, %.0f bytes, %.3f s (%.2f GB/s)%s\n", n, proved,
               n_new, (unsigned long long)missing, bytes, seconds, seconds > 0 ? bytes / seconds / 1e9 : 0.0, anchored);
}

}  // namespace

// what cp2_fill_begin and cp2_fill_resume ask of (cfg, first_slot, n_local, slot_roots) before anything is allocated
int cp2i::fill_session_check(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, const uint8_t* slot_roots) {
  CP2_REFUSE_STUCK(ctx);
  std::string err;
  if (!fill_check_range(cfg->n_slots, first_slot, n_local, cfg->max_depth, cfg->max_log2_nslots, cfg->n_cells, cfg->cell_size,
                        cfg->file_base ? SLOT_FILE_MAX_CELL : 0, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (trees_check_geometry(cfg->cell_size, cfg->block_size, cfg->n_cells, n_local) != CP2_OK) {
    ctx->err = "fill: cell_size " + std::to_string(cfg->cell_size) + ", block_size " + std::to_string(cfg->block_size) + ", n_cells " +
               std::to_string(cfg->n_cells) + " is a geometry the tree builders refuse";
    return CP2_ERR_INVALID;
  }
  if (!slot_roots) {
    ctx->err = "fill: slot_roots must not be NULL";
    return CP2_ERR_INVALID;
  }
  return CP2_OK;
}

// the session of a checked (cfg, first_slot, n_local, slot_roots) with nothing uploaded yet: the plan, the compact buffer (as allocated),
// the buffer of the roots and their canonical form on the host
int cp2i::fill_session_alloc(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, const uint8_t* slot_roots,
                             std::unique_ptr<cp2_fill_session>* out) {
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<cp2_fill_session> f(new (std::nothrow) cp2_fill_session());
  if (!f) return CP2_ERR_ALLOC;
  f->ctx = ctx;
  f->cfg = *cfg;
  f->from_file = cfg->file_base != nullptr;
  if (f->from_file) f->file_base = cfg->file_base;
  f->cfg.file_base = nullptr;
  f->plan.init(first_slot, n_local, cfg->n_cells / (cfg->block_size / cfg->cell_size));
  CP2_TRY(f->compact.alloc(ctx, f->plan.rows * 32));            // what a compact dataset of these slots holds, once
  CP2_TRY(f->slot_roots.alloc(ctx, n_local * 32));
  f->roots.resize(n_local * 32);                                 // values of at least r are reduced, as everywhere else
  for (uint64_t s = 0; s < n_local; ++s) canonical_felt(slot_roots + s * 32, &f->roots[s * 32]);
  *out = std::move(f);
  return CP2_OK;
}

// ... and with the roots on the device
static int session_open(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, const uint8_t* slot_roots,
                        std::unique_ptr<cp2_fill_session>* out) {
  std::unique_ptr<cp2_fill_session> f;
  CP2_TRY(fill_session_alloc(ctx, cfg, first_slot, n_local, slot_roots, &f));
  CP2_HIP(ctx, hipMemcpyAsync(f->slot_roots.p, f->roots.data(), f->roots.size(), hipMemcpyHostToDevice, ctx->stream));
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *out = std::move(f);
  return CP2_OK;
}

extern "C" int cp2_fill_begin(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, const uint8_t* slot_roots, void** out) try {
  if (!ctx || !cfg || !out) return CP2_ERR_INVALID;
  *out = nullptr;
  CP2_TRY(fill_session_check(ctx, cfg, first_slot, n_local, slot_roots));
  std::unique_ptr<cp2_fill_session> f;
  CP2_TRY(session_open(ctx, cfg, first_slot, n_local, slot_roots, &f));
  *out = f.release();
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// What every add does once the device has judged its n requests (verdict[i] == 0: proved, its rows stored and marked): NEW / DUPLICATE, the
// writer and its roll-back, presence after the sync, the outputs and the trace line.  One body for cp2_fill_add, cp2_fill_add_anchored and
// cp2_fill_add_multi.
static int fill_add_tail(cp2_fill_session* f, const uint64_t* slot_block, const uint8_t* data, size_t n, const uint32_t* verdict, uint32_t* status,
                         size_t* n_new, std::chrono::steady_clock::time_point t0, uint64_t siblings, size_t depth) {
  cp2_ctx* ctx = f->ctx;
  const cp2_config& c = f->cfg;
  FillPlan& plan = f->plan;
  std::string err;
  std::vector<uint32_t> st(n);
  plan.resolve(slot_block, verdict, n, st.data());
  int r = CP2_OK;
  if (f->from_file) {                                // the NEW blocks into "<file_base><slot>.dat": repair's writer and its rules
    std::vector<uint32_t> w = FillPlan::write_mask(st.data(), n);
    size_t written_n = 0;
    std::vector<FileStamp> written;
    r = repair_write(f->file_base, c.block_size, slot_block, data, n, w.data(), &written_n, &written, &err);
    FillPlan::roll_back(slot_block, w, st.data());
  }
  const size_t set = plan.commit(slot_block, st.data(), n);   // present only now: an UNWRITTEN block stays missing and can be sent again
  std::copy(st.begin(), st.end(), status);
  if (n_new) *n_new = set;
  if (r != CP2_OK) ctx->err = err;
  fill_trace(n, status, set, c.block_size, plan.n_missing(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), siblings, depth);
  return r;
}

// What cp2_fill_add and cp2_fill_add_anchored do with n > 0 requests they have checked.  levels == NULL: every request brings its whole
// path, `paths` is n x depth rows and the walk ends at the stated slot root; otherwise request i brings levels[i] siblings, `paths` is
// packed in request order and the walk ends at the node the plan names.  Everything else is one body: the data path, the chunks,
// NEW / DUPLICATE, the writer and its roll-back, presence after the sync, the trace line.
static int fill_add_checked(cp2_fill_session* f, const uint64_t* slot_block, const uint8_t* data, const uint8_t* paths, const uint32_t* levels,
                            size_t n, uint32_t* status, size_t* n_new) {
  cp2_ctx* ctx = f->ctx;
  const cp2_config& c = f->cfg;
  FillPlan& plan = f->plan;
  std::string err;
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  // cp2_blocks_verify's data path; its last step also keeps the block roots that were proved
  const size_t depth = block_proof_depth(plan.n_blocks), path_bytes = depth * 32;
  std::vector<uint64_t> local_block, dest, path_off, anchor_row;
  if (levels) plan.device_requests_anchored(slot_block, levels, n, &local_block, &dest, &path_off, &anchor_row);
  else plan.device_requests(slot_block, n, &local_block, &dest);
  const bool keeps = plan.keeps_nodes;
  DevBuf d_req, d_dest, d_paths, d_walk, d_levels, d_off, d_anchor;   // (go after the streams have drained: DevBuf::release)
  RepairJudge judge;
  judge.begin = [&](size_t chunk) -> int {
    CP2_TRY(d_req.scratch(ctx, n * 16));
    CP2_TRY(d_dest.scratch(ctx, n * 8));
    CP2_HIP(ctx, hipMemcpyAsync(d_req.p, local_block.data(), n * 16, hipMemcpyHostToDevice, ctx->stream));
    CP2_HIP(ctx, hipMemcpyAsync(d_dest.p, dest.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
    if (levels) {                                    // a chunk's packed paths are one contiguous range: rows [path_off[c0], path_off[c0 + m])
      uint64_t most = 1;
      for (size_t c0 = 0; c0 < n; c0 += chunk) most = std::max(most, path_off[std::min(n, c0 + chunk)] - path_off[c0]);
      CP2_TRY(d_paths.scratch(ctx, (size_t)most * 32));
      CP2_TRY(d_walk.scratch(ctx, (size_t)most * 64));
      CP2_TRY(d_levels.scratch(ctx, n * 4));
      CP2_TRY(d_off.scratch(ctx, n * 8));
      CP2_TRY(d_anchor.scratch(ctx, n * 8));
      CP2_HIP(ctx, hipMemcpyAsync(d_levels.p, levels, n * 4, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, hipMemcpyAsync(d_off.p, path_off.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, hipMemcpyAsync(d_anchor.p, anchor_row.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
      return CP2_OK;
    }
    CP2_TRY(d_paths.scratch(ctx, chunk * path_bytes));
    if (keeps) CP2_TRY(d_walk.scratch(ctx, chunk * 2 * path_bytes));   // the chunk's siblings and ancestors as the walk meets them
    return CP2_OK;
  };
  // the chunk's paths travel with the chunk (the previous chunk's walk, earlier on this stream, has read its own)
  judge.stage = [&](size_t c0, size_t m, hipStream_t st) -> int {
    if (levels) {
      const size_t rows = (size_t)(path_off[c0 + m] - path_off[c0]);
      if (rows) CP2_HIP(ctx, hipMemcpyAsync(d_paths.p, paths + (size_t)path_off[c0] * 32, rows * 32, hipMemcpyHostToDevice, st));
      return CP2_OK;
    }
    CP2_HIP(ctx, hipMemcpyAsync(d_paths.p, paths + c0 * path_bytes, m * path_bytes, hipMemcpyHostToDevice, st));
    return CP2_OK;
  };
  judge.verdicts = [&](const uint8_t* fresh, size_t c0, size_t m, uint32_t* verdict, hipStream_t st) -> int {
    const uint64_t* tab = static_cast<const uint64_t*>(f->layer_tab.p);
    if (levels) {                                    // the same walk, each lane up to the kept node the plan named
      CP2_HIP(ctx, cp2k::launch_block_path_commit_anchored(fresh, d_paths.p, static_cast<const uint32_t*>(d_levels.p) + c0,
                                                           static_cast<const uint64_t*>(d_off.p) + c0, path_off[c0],
                                                           static_cast<const uint64_t*>(d_req.p) + 2 * c0, f->slot_roots.p,
                                                           static_cast<const uint64_t*>(d_dest.p) + c0, static_cast<const uint64_t*>(d_anchor.p) + c0,
                                                           tab, tab + depth + 1, plan.n_blocks, (uint32_t)depth, m, verdict, f->compact.p, plan.rows,
                                                           d_walk.p, st));
      return CP2_OK;
    }
    if (keeps) {                                     // the same walk; a proved path leaves all its nodes where the tree has them
      CP2_HIP(ctx, cp2k::launch_block_path_commit_nodes(fresh, d_paths.p, static_cast<const uint64_t*>(d_req.p) + 2 * c0, f->slot_roots.p,
                                                        static_cast<const uint64_t*>(d_dest.p) + c0, tab, tab + depth + 1, plan.n_blocks,
                                                        (uint32_t)depth, m, verdict, f->compact.p, plan.rows, d_walk.p, st));
      return CP2_OK;
    }
    CP2_HIP(ctx, cp2k::launch_block_path_commit(fresh, d_paths.p, static_cast<const uint64_t*>(d_req.p) + 2 * c0, f->slot_roots.p,
                                                static_cast<const uint64_t*>(d_dest.p) + c0, plan.n_blocks, (uint32_t)depth, m, verdict,
                                                f->compact.p, plan.rows, st));
    return CP2_OK;
  };
  std::vector<uint32_t> verdict(n);
  CP2_TRY(repair_check_with(ctx, c.cell_size, c.block_size, data, n, verdict.data(), judge));
  // written or not: the nodes of a proved path are authentic and stored
  if (levels) plan.mark_proved_anchored(slot_block, levels, verdict.data(), n);
  else if (keeps) plan.mark_proved(slot_block, verdict.data(), n);
  return fill_add_tail(f, slot_block, data, n, verdict.data(), status, n_new, t0, levels ? path_off[n] : WHOLE_PATHS, depth);
}

extern "C" int cp2_fill_add(void* fill, const uint64_t* slot_block, const uint8_t* data, const uint8_t* paths, size_t n, uint32_t* status,
                            size_t* n_new) try {
  cp2_fill_session* f = session(fill);
  if (!f) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  if (n && (!slot_block || !data || !paths || !status)) {
    ctx->err = "fill: slot_block, data, paths and status must not be NULL when n > 0";
    return CP2_ERR_INVALID;
  }
  std::string err;
  if (!f->plan.validate(slot_block, n, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n == 0) {
    if (n_new) *n_new = 0;
    return CP2_OK;
  }
  return fill_add_checked(f, slot_block, data, paths, nullptr, n, status, n_new);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_fill_add_multi(void* fill, const uint64_t* groups, size_t n_groups, const uint64_t* blocks, const uint8_t* data, const uint8_t* nodes,
                                  size_t n_rows, uint32_t* status, size_t* n_new) try {
  cp2_fill_session* f = session(fill);
  if (!f) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  const cp2_config& c = f->cfg;
  FillPlan& plan = f->plan;
  size_t n = 0;
  if ((n_groups && !groups) || !multiproof_count(groups, n_groups, &n) || (n && (!blocks || !data || !status)) || (n_rows && !nodes)) {
    ctx->err = "fill multi: groups, blocks, data and status must not be NULL when there are requests, nor nodes when n_rows > 0";
    return CP2_ERR_INVALID;
  }
  std::string err;
  if (!multiproof_validate("fill multi", "slot", groups, n_groups, blocks, plan.first_slot, plan.n_local, plan.n_blocks, true, n_rows, nullptr, &err) ||
      !plan.validate(nullptr, 0, &err)) {            // ... and, last, a finished session
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n_groups == 0) {
    if (n_new) *n_new = 0;
    return CP2_OK;
  }
  // the requests as every other add names them, and the plan of the groups' subtrees
  std::vector<uint64_t> slot_block(2 * n), counts(n_groups), nb(n_groups, plan.n_blocks), local(n_groups), want(n_groups);
  for (size_t g = 0, at = 0; g < n_groups; ++g) {
    counts[g] = groups[2 * g + 1];
    local[g] = groups[2 * g] - plan.first_slot;
    want[g] = (uint64_t)reinterpret_cast<uintptr_t>(f->slot_roots.p) + local[g] * 32;
    for (uint64_t j = 0; j < counts[g]; ++j, ++at) {
      slot_block[2 * at] = groups[2 * g];
      slot_block[2 * at + 1] = blocks[at];
    }
  }
  MultiproofPlan mp;
  if (!multiproof_plan(counts.data(), nb.data(), n_groups, blocks, &mp, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  // what a proved group leaves in the buffer: its block roots always, and in a session that keeps nodes every sent and computed row, each
  // where the compact layout has it (FillPlan::node_row) -- the rows mark_proved marks for whole paths.  Sent rows are stored as they
  // stand, so they go up canonical, as a whole path's siblings are stored.
  const size_t n_commit = plan.keeps_nodes ? mp.n_work : n;
  std::vector<uint32_t> src(n_commit);
  std::vector<uint64_t> dst(n_commit);
  for (size_t r = 0; r < n_commit; ++r) {
    src[r] = (uint32_t)r;
    dst[r] = (uint64_t)reinterpret_cast<uintptr_t>(f->compact.p) + plan.node_row(mp.row_level[r], local[mp.row_group[r]], mp.row_index[r]) * 32;
  }
  std::vector<uint8_t> sent(n_rows * 32);
  for (size_t r = 0; r < n_rows; ++r) canonical_felt(nodes + r * 32, &sent[r * 32]);
  DevBuf d_src, d_dst, d_group;                      // (go after the streams have drained: DevBuf::release)
  const auto commit = [&](const void* d_work, const uint32_t* d_verdict, hipStream_t st) -> int {
    CP2_TRY(d_src.scratch(ctx, n_commit * 4));
    CP2_TRY(d_dst.scratch(ctx, n_commit * 8));
    CP2_TRY(d_group.scratch(ctx, n_commit * 4));
    CP2_HIP(ctx, hipMemcpyAsync(d_src.p, src.data(), n_commit * 4, hipMemcpyHostToDevice, st));
    CP2_HIP(ctx, hipMemcpyAsync(d_dst.p, dst.data(), n_commit * 8, hipMemcpyHostToDevice, st));
    CP2_HIP(ctx, hipMemcpyAsync(d_group.p, mp.row_group.data(), n_commit * 4, hipMemcpyHostToDevice, st));
    CP2_HIP(ctx, cp2k::launch_multiproof_commit(d_work, mp.n_work, static_cast<const uint32_t*>(d_src.p), static_cast<const uint64_t*>(d_dst.p),
                                                static_cast<const uint32_t*>(d_group.p), d_verdict, (uint32_t)n_groups, n_commit, st));
    return CP2_OK;
  };
  std::vector<uint32_t> group_verdict(n_groups), verdict(n);
  CP2_TRY(multiproof_check(ctx, c.cell_size, c.block_size, mp, want.data(), n_groups, data, sent.data(), commit, group_verdict.data(), nullptr));
  for (size_t i = 0; i < n; ++i) verdict[i] = group_verdict[mp.row_group[i]];
  // written or not: the nodes of a proved group are authentic and stored
  if (plan.keeps_nodes) plan.mark_proved_multi(mp.row_group.data(), mp.row_level.data(), mp.row_index.data(), mp.n_work, local.data(), group_verdict.data());
  return fill_add_tail(f, slot_block.data(), data, n, verdict.data(), status, n_new, t0, n_rows, plan.depth());
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// ---- multiproofs against what the session knows -------------------------------------------------------------------------------------------
namespace {

// known(group, level, index) of a call's groups against the session as it stands; a session that keeps no nodes knows its roots only
auto session_knows(const FillPlan& plan, const uint64_t* groups) {
  return [&plan, groups](size_t g, size_t l, uint64_t i) {
    return plan.keeps_nodes && plan.is_known(plan.node_row(l, groups[2 * g] - plan.first_slot, i));
  };
}

}  // namespace

extern "C" int cp2_fill_multiproof_want(const void* fill, const uint64_t* groups, size_t n_groups, const uint64_t* blocks, uint64_t* level_index,
                                        size_t cap, size_t* n_rows, uint64_t* group_rows) try {
  const cp2_fill_session* f = session(fill);
  if (!f) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  const FillPlan& plan = f->plan;
  size_t n = 0;
  if (!n_rows || (n_groups && !groups) || !multiproof_count(groups, n_groups, &n) || (n && !blocks)) {
    ctx->err = "fill multiproof want: groups, blocks and n_rows must not be NULL when there are requests";
    return CP2_ERR_INVALID;
  }
  std::string err;
  std::vector<uint64_t> li, per(n_groups);
  uint64_t rows = 0;
  if (!multiproof_anchor_validate("fill multiproof want", groups, n_groups, blocks, plan.first_slot, plan.n_local, plan.n_blocks,
                                  session_knows(plan, groups), false, 0, &rows, per.data(), &li, &err) ||
      !plan.validate(nullptr, 0, &err)) {            // ... and, last, a finished session
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  *n_rows = (size_t)rows;
  if (group_rows) std::copy(per.begin(), per.end(), group_rows);
  if (rows && level_index && cap >= rows) std::memcpy(level_index, li.data(), li.size() * 8);
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_fill_block_tree_rows(void* fill, const uint64_t* places, size_t n, uint32_t* status, uint8_t* rows) try {
  cp2_fill_session* f = session(fill);
  if (!f) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  const FillPlan& plan = f->plan;
  if (n && (!places || !status)) {
    ctx->err = "fill tree rows: places and status must not be NULL when n > 0";
    return CP2_ERR_INVALID;
  }
  if (plan.finished) {
    ctx->err = "fill tree rows: the session is finished: its rows come from the dataset (cp2_dataset_block_tree_rows)";
    return CP2_ERR_INVALID;
  }
  if (!plan.keeps_nodes) {
    ctx->err = "fill tree rows: this session does not keep the nodes of the paths it proves: call cp2_fill_keep_nodes first";
    return CP2_ERR_INVALID;
  }
  std::string err;
  if (!tree_places_validate("fill tree rows", places, n, plan.first_slot, plan.n_local, plan.csizes, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n == 0) return CP2_OK;
  // the statuses from the host's bitmap; the stated slot root is known from the start and is served from the session's copy of it
  std::vector<uint32_t> st(n);
  std::vector<uint64_t> addr(n, 0);
  for (size_t i = 0; i < n; ++i) {
    const uint64_t local = places[3 * i] - plan.first_slot, l = places[3 * i + 1], r = plan.node_row((size_t)l, local, places[3 * i + 2]);
    if (l == plan.depth()) addr[i] = (uint64_t)reinterpret_cast<uintptr_t>(f->slot_roots.p) + local * 32;
    else if (plan.is_known(r)) addr[i] = (uint64_t)reinterpret_cast<uintptr_t>(f->compact.p) + r * 32;
    st[i] = addr[i] ? CP2_FILL_ROW_KNOWN : CP2_FILL_ROW_UNKNOWN;
  }
  if (rows) {                                        // an unknown row names no address: k_gather_addr leaves zeros there
    CP2_REFUSE_STUCK(ctx);
    CP2_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint8_t> out(n * 32);
    CP2_TRY(gather_rows_by_addr(ctx, addr, out.data()));
    std::memcpy(rows, out.data(), n * 32);
  }
  std::copy(st.begin(), st.end(), status);
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_fill_add_multi_anchored(void* fill, const uint64_t* groups, size_t n_groups, const uint64_t* blocks, const uint8_t* data,
                                           const uint8_t* nodes, size_t n_rows, uint32_t* status, size_t* n_new) try {
  cp2_fill_session* f = session(fill);
  if (!f) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  const cp2_config& c = f->cfg;
  FillPlan& plan = f->plan;
  size_t n = 0;
  if ((n_groups && !groups) || !multiproof_count(groups, n_groups, &n) || (n && (!blocks || !data || !status)) || (n_rows && !nodes)) {
    ctx->err = "fill multi anchored: groups, blocks, data and status must not be NULL when there are requests, nor nodes when n_rows > 0";
    return CP2_ERR_INVALID;
  }
  std::string err;
  // (8): a want list made before another add landed is stale: the session needs other rows now, and mostly fewer
  if (!multiproof_anchor_validate("fill multi anchored", groups, n_groups, blocks, plan.first_slot, plan.n_local, plan.n_blocks,
                                  session_knows(plan, groups), true, n_rows, nullptr, nullptr, nullptr, &err) ||
      !plan.validate(nullptr, 0, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (!plan.keeps_nodes) {
    ctx->err = "fill multi anchored: this session does not keep the nodes of the paths it proves: call cp2_fill_keep_nodes first, or use cp2_fill_add_multi";
    return CP2_ERR_INVALID;
  }
  if (n_groups == 0) {
    if (n_new) *n_new = 0;
    return CP2_OK;
  }
  std::vector<uint64_t> slot_block(2 * n), counts(n_groups), nb(n_groups, plan.n_blocks), local(n_groups);
  for (size_t g = 0, at = 0; g < n_groups; ++g) {
    counts[g] = groups[2 * g + 1];
    local[g] = groups[2 * g] - plan.first_slot;
    for (uint64_t j = 0; j < counts[g]; ++j, ++at) {
      slot_block[2 * at] = groups[2 * g];
      slot_block[2 * at + 1] = blocks[at];
    }
  }
  MultiproofAnchorPlan mp;
  if (!multiproof_anchor_plan(
          counts.data(), nb.data(), n_groups, blocks, [&](size_t g, size_t l, uint64_t i) { return plan.is_known(plan.node_row(l, local[g], i)); }, &mp,
          &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  // the plan's places made addresses: the kept inputs and what every top is compared with are rows of the session's buffer (the top of
  // level depth: the stated slot root); the commit list goes where node_row has each row
  const uint64_t compact = (uint64_t)reinterpret_cast<uintptr_t>(f->compact.p), roots = (uint64_t)reinterpret_cast<uintptr_t>(f->slot_roots.p);
  const auto addr_of = [&](size_t r) { return compact + plan.node_row(mp.row_level[r], local[mp.row_group[r]], mp.row_index[r]) * 32; };
  std::vector<uint64_t> kept_addr(mp.n_kept), top_want(mp.n_tops());
  std::vector<uint32_t> top_row_group(2 * mp.n_tops());
  for (size_t k = 0; k < mp.n_kept; ++k) kept_addr[k] = addr_of(mp.kept_base() + k);
  for (size_t t = 0; t < mp.n_tops(); ++t) {
    top_row_group[2 * t] = mp.top_row[t];
    top_row_group[2 * t + 1] = mp.top_group[t];
    top_want[t] = mp.top_level[t] == plan.depth() ? roots + local[mp.top_group[t]] * 32
                                                  : compact + plan.node_row(mp.top_level[t], local[mp.top_group[t]], mp.top_index[t]) * 32;
  }
  MultiproofAnchors anchors;
  anchors.n_kept = mp.n_kept;
  anchors.n_tops = mp.n_tops();
  anchors.kept_addr = kept_addr.data();
  anchors.top_row_group = top_row_group.data();
  anchors.top_want = top_want.data();
  anchors.top_off = mp.top_off.data();
  const size_t n_commit = mp.commit.size();
  std::vector<uint64_t> dst(n_commit);
  std::vector<uint32_t> c_group(n_commit), c_level(n_commit);
  std::vector<uint64_t> c_index(n_commit);
  for (size_t k = 0; k < n_commit; ++k) {
    const size_t r = mp.commit[k];
    dst[k] = addr_of(r);
    c_group[k] = mp.row_group[r];
    c_level[k] = mp.row_level[r];
    c_index[k] = mp.row_index[r];
  }
  std::vector<uint8_t> sent(n_rows * 32);            // stored as they stand, so they go up canonical
  for (size_t r = 0; r < n_rows; ++r) canonical_felt(nodes + r * 32, &sent[r * 32]);
  DevBuf d_src, d_dst, d_group;                      // (go after the streams have drained: DevBuf::release)
  const auto commit = [&](const void* d_work, const uint32_t* d_verdict, hipStream_t st) -> int {
    if (n_commit == 0) return CP2_OK;                // (every block root was known already)
    CP2_TRY(d_src.scratch(ctx, n_commit * 4));
    CP2_TRY(d_dst.scratch(ctx, n_commit * 8));
    CP2_TRY(d_group.scratch(ctx, n_commit * 4));
    CP2_HIP(ctx, hipMemcpyAsync(d_src.p, mp.commit.data(), n_commit * 4, hipMemcpyHostToDevice, st));
    CP2_HIP(ctx, hipMemcpyAsync(d_dst.p, dst.data(), n_commit * 8, hipMemcpyHostToDevice, st));
    CP2_HIP(ctx, hipMemcpyAsync(d_group.p, c_group.data(), n_commit * 4, hipMemcpyHostToDevice, st));
    CP2_HIP(ctx, cp2k::launch_multiproof_commit(d_work, mp.n_work, static_cast<const uint32_t*>(d_src.p), static_cast<const uint64_t*>(d_dst.p),
                                                static_cast<const uint32_t*>(d_group.p), d_verdict, (uint32_t)n_groups, n_commit, st));
    return CP2_OK;
  };
  std::vector<uint32_t> group_verdict(n_groups), verdict(n);
  CP2_TRY(multiproof_check(ctx, c.cell_size, c.block_size, mp, nullptr, n_groups, data, sent.data(), commit, group_verdict.data(), nullptr, &anchors));
  for (size_t i = 0; i < n; ++i) verdict[i] = group_verdict[mp.row_group[i]];
  // written or not: the nodes of a proved group are authentic and stored
  plan.mark_proved_multi(c_group.data(), c_level.data(), c_index.data(), n_commit, local.data(), group_verdict.data());
  if (std::getenv("CP2_TRACE"))
    std::fprintf(stderr, "[cp2 trace] fill add multi anchored: %zu group(s), %zu top(s), %zu kept input(s), %zu compression(s)\n", n_groups, mp.n_tops(),
                 mp.n_kept, mp.computed());
  return fill_add_tail(f, slot_block.data(), data, n, verdict.data(), status, n_new, t0, n_rows, plan.depth());
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_fill_missing(const void* fill, uint64_t* missing, size_t cap, uint64_t* n_missing) try {
  const cp2_fill_session* f = session(fill);
  if (!f || !n_missing) return CP2_ERR_INVALID;
  if (cap && !missing) {
    f->ctx->err = "fill: missing must not be NULL when cap > 0";
    return CP2_ERR_INVALID;
  }
  *n_missing = f->plan.missing(missing, cap);
  return CP2_OK;
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_fill_finish(void* fill, const char* cache_path, cp2_dataset** out) try {
  cp2_fill_session* f = session(fill);
  if (!f || !out) return CP2_ERR_INVALID;
  *out = nullptr;
  cp2_ctx* ctx = f->ctx;
  FillPlan& plan = f->plan;
  std::string err;
  if (!plan.may_finish(&err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  // the upper layers of all local trees from layer 0, layer-major, one launch per layer over all slots: the compact layout is exactly
  // what merkle_trees_dev writes for n_local trees of n_blocks leaves each
  CP2_TRY(merkle_trees_dev(ctx, f->compact.p, plan.n_blocks, plan.n_local, f->compact.p, true));
  // the top layer against the stated roots, on the device
  const size_t nl = (size_t)plan.n_local;
  DevBuf d_rows, d_verdict;
  CP2_TRY(d_rows.scratch(ctx, nl * 8));
  CP2_TRY(d_verdict.scratch(ctx, nl * 4));
  std::vector<uint64_t> rows(nl);
  for (size_t s = 0; s < nl; ++s) rows[s] = s;
  std::vector<uint32_t> verdict(nl);
  CP2_HIP(ctx, hipMemcpyAsync(d_rows.p, rows.data(), nl * 8, hipMemcpyHostToDevice, ctx->stream));
  CP2_HIP(ctx, cp2k::launch_repair_compare(f->compact.u8() + plan.coff.back() * 32, f->slot_roots.p, nl, static_cast<const uint64_t*>(d_rows.p), nl,
                                           static_cast<uint32_t*>(d_verdict.p), ctx->stream));
  CP2_HIP(ctx, hipMemcpyAsync(verdict.data(), d_verdict.p, nl * 4, hipMemcpyDeviceToHost, ctx->stream));
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t s = 0; s < nl; ++s)
    if (verdict[s] != 0) {
      ctx->err = "fill: the tree over the kept block roots of slot " + std::to_string(plan.first_slot + s) + " does not end in the stated slot root";
      return CP2_ERR_IO;
    }
  // the kept form, under the name and with the contents cp2_dataset_build_cached writes for a compact dataset (it loads this instead of
  // rebuilding), with the stamps of the slot files as they stand
  if (cache_path) {
    const int st = kept_save(ctx, kept_cache_path(cache_path).c_str(), kept_meta(f->cfg, f->plan.first_slot, f->plan.n_local, f->from_file, f->file_base, 2),
                             f->compact.p, f->plan.rows * 32);
    if (st != CP2_OK) {
      if (ctx->err.empty()) ctx->err = std::string("fill: cannot write the kept layers to ") + cache_path;
      return st;
    }
  }
  // the session's buffer becomes the compact buffer of an ordinary dataset (dataset_alloc_kept's layout), source as begun
  std::unique_ptr<cp2_dataset> ds = fill_dataset_shell(f);
  if (!ds) return CP2_ERR_ALLOC;
  hand_over(f->compact, ds->compact);
  plan.finished = true;
  if (std::getenv("CP2_TRACE"))
    std::fprintf(stderr, "[cp2 trace] fill finish: %llu slot(s) of %llu block(s), %zu layer(s) built, %.3f ms%s\n", (unsigned long long)plan.n_local,
                 (unsigned long long)plan.n_blocks, plan.csizes.size() - 1,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3, cache_path ? ", kept form saved" : "");
  *out = ds.release();
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// ---- checkpoints ------------------------------------------------------------------------------------------------------------------------
namespace {

FillCkptMeta session_meta(const cp2_fill_session* f) {
  FillCkptMeta m;
  const cp2_config& c = f->cfg;
  m.cell_size = c.cell_size; m.block_size = c.block_size; m.n_cells = c.n_cells; m.n_slots = c.n_slots;
  m.first_slot = f->plan.first_slot; m.n_local = f->plan.n_local;
  m.src = f->from_file ? FILL_SRC_FILE : FILL_SRC_FAKE;
  m.seed = c.seed;
  m.file_base = f->file_base;
  m.roots = f->roots;
  return m;
}

// a checkpoint's bytes at `path`: written beside it, synced and renamed, so that an older checkpoint there stays whole until the new one is
int write_checkpoint_file(cp2_ctx* ctx, const char* path, const std::vector<uint8_t>& buf) {
  TmpFile tmp(path);
  const bool made = tmp.ok(), done = made && pwrite_all(tmp.fd(), buf.data(), buf.size(), 0) && tmp.commit(true);
  const std::string why = std::strerror(errno);       // of the step that failed, before anything else can set it
  if (!done) {                                         // an older checkpoint at `path` stays as it is
    ctx->err = made ? "fill: cannot write checkpoint " + std::string(path) + " (through " + tmp.tmp_name() + "): " + why
                    : "fill: cannot create checkpoint " + tmp.tmp_name() + ": " + why;
    return CP2_ERR_IO;
  }
  return CP2_OK;
}

// A checkpoint file of either format in memory.  Its fixed head is read first and head_ok(fixed, size, &why) compares what it announces with
// the file's size before the buffer is sized; the whole file then goes to parse(buf, size, &why).
template <class HeadOk, class Parse>
int read_checkpoint_file(std::string* err, const char* path, HeadOk head_ok, Parse parse) {
  const std::string name(path);
  const int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) {
    *err = "fill: cannot open checkpoint " + name + ": " + std::strerror(errno);
    return CP2_ERR_IO;
  }
  const FdCloser closer{fd};
  struct stat sb;
  if (fstat(fd, &sb) != 0) {
    *err = "fill: cannot stat checkpoint " + name + ": " + std::strerror(errno);
    return CP2_ERR_IO;
  }
  const size_t size = (size_t)sb.st_size;
  uint8_t fixed[FILL_CKPT_FIXED] = {};
  std::string why;
  int e = size ? slot_file_read_rest(fd, fixed, std::min(size, sizeof fixed), 0) : 0;
  const bool ok = !e && head_ok(fixed, size, &why);
  std::vector<uint8_t> buf(ok ? size : 0);
  if (ok) e = slot_file_read_rest(fd, buf.data(), size, 0);
  if (e) {
    *err = "fill: cannot read checkpoint " + name + ": " + std::strerror(e);
    return CP2_ERR_IO;
  }
  if (!ok || !parse(buf.data(), size, &why)) {
    *err = "fill: checkpoint " + name + " " + why;
    return CP2_ERR_IO;
  }
  return CP2_OK;
}

// a CP2FILL1 file: of exactly the size its header states
int read_checkpoint(std::string* err, const char* path, FillCheckpoint* ck) {
  return read_checkpoint_file(
      err, path,
      [](const uint8_t* fixed, size_t size, std::string* why) {
        FillCkptMeta m;
        FillCkptLayout l;
        if (!fill_ckpt_fixed(fixed, size, &m, &l, why)) return false;
        if (size != l.size)
          *why = size < l.size ? "is truncated: " + std::to_string(size) + " bytes of " + std::to_string(l.size) : "is corrupt: longer than its header states";
        return size == l.size;
      },
      [&](const uint8_t* buf, size_t size, std::string* why) { return fill_ckpt_parse(buf, size, ck, why); });
}

// the same for a CP2FILL2 file, whose header bounds its size
int read_node_checkpoint(cp2_ctx* ctx, const char* path, NodeCheckpoint* ck) {
  return read_checkpoint_file(
      &ctx->err, path,
      [](const uint8_t* fixed, size_t size, std::string* why) {
        FillCkptMeta m;
        NodeCkptLayout l;
        return node_ckpt_fixed(fixed, size, &m, &l, why) && node_ckpt_size_ok(l, size, why);
      },
      [&](const uint8_t* buf, size_t size, std::string* why) { return node_ckpt_parse(buf, size, ck, why); });
}

// Every block the session calls present against what its source holds now; the global indices of those that no longer hash to their kept
// root are appended to `dropped` (their rows of layer 0 are zeros by then).  *bytes = what was read or regenerated.  One judge on repair's
// data path (repair_check_with) and two sources of the blocks: the fake source regenerates them on the device (the `cells` hook), slot
// files are read chunk by chunk (fill_read_chunk) and uploaded.
int recheck_present(cp2_fill_session* f, std::vector<uint64_t>* dropped, uint64_t* n_read, double* bytes) {
  cp2_ctx* ctx = f->ctx;
  const cp2_config& c = f->cfg;
  const FillPlan& plan = f->plan;
  const size_t bs = c.block_size, cpb = bs / c.cell_size;
  // the same expression as repair_check_with's chunks: a chunk of the read plan is a chunk of the data path, in one call over all entries
  // (fake source) as in one call per chunk (slot files)
  const size_t chunk = std::max<size_t>(1, (ctx->stage_bytes / 2) / bs);
  const FillReadPlan rp = fill_read_plan(plan.bits, plan.total(), plan.n_blocks, chunk);
  const size_t n = rp.g.size();
  *n_read = n;
  *bytes = (double)n * (double)bs;
  if (n == 0) return CP2_OK;
  std::vector<uint32_t> verdict(n);
  std::vector<uint64_t> seeds, firsts;
  DevBuf d_dest, d_seeds, d_firsts;                  // (go after the streams have drained: DevBuf::release)
  size_t at = 0;                                     // the plan entry that is request 0 of the current call
  RepairJudge judge;
  judge.begin = [&](size_t) -> int {                 // the destination rows of the whole plan, once, whatever the number of calls
    if (d_dest.p) return CP2_OK;
    CP2_TRY(d_dest.scratch(ctx, n * 8));
    CP2_HIP(ctx, hipMemcpyAsync(d_dest.p, rp.g.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));   // (coff[0] == 0: a global index is its row)
    if (f->from_file) return CP2_OK;
    CP2_TRY(d_seeds.scratch(ctx, n * 8));
    CP2_TRY(d_firsts.scratch(ctx, n * 8));
    CP2_HIP(ctx, hipMemcpyAsync(d_seeds.p, seeds.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
    CP2_HIP(ctx, hipMemcpyAsync(d_firsts.p, firsts.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
    return CP2_OK;
  };
  judge.verdicts = [&](const uint8_t* fresh, size_t c0, size_t m, uint32_t* v, hipStream_t st) -> int {
    CP2_HIP(ctx, cp2k::launch_block_root_recheck(fresh, static_cast<const uint64_t*>(d_dest.p) + at + c0, m, v, f->compact.p, plan.total(), st));
    return CP2_OK;
  };
  if (!f->from_file) {
    seeds.resize(n);
    firsts.resize(n);
    for (size_t i = 0; i < n; ++i) {
      seeds[i] = cp2_slot_seed(c.seed, plan.first_slot + rp.g[i] / plan.n_blocks);
      firsts[i] = (rp.g[i] % plan.n_blocks) * cpb;
    }
    judge.cells = [&](size_t c0, size_t m, uint8_t* d_cells, hipStream_t st) -> int {
      CP2_HIP(ctx, cp2k::launch_gen_fake_cells_many(static_cast<const uint64_t*>(d_seeds.p) + c0, static_cast<const uint64_t*>(d_firsts.p) + c0, cpb,
                                                    m * cpb, c.cell_size, d_cells, st));
      return CP2_OK;
    };
    CP2_TRY(repair_check_with(ctx, c.cell_size, bs, nullptr, n, verdict.data(), judge));
  } else {
    std::unique_ptr<uint8_t[]> host(new uint8_t[std::min(n, chunk) * bs]);
    for (size_t k = 0; k < rp.n_chunks(); ++k) {
      std::string bad;
      int err = 0;
      if (!fill_read_chunk(rp, k, f->file_base, plan.first_slot, bs, host.get(), &bad, &err)) {
        ctx->err = slot_file_error(bad, err);
        return CP2_ERR_IO;
      }
      at = rp.chunk_begin(k);
      CP2_TRY(repair_check_with(ctx, c.cell_size, bs, host.get(), rp.chunk_end(k) - at, verdict.data() + at, judge));
    }
  }
  for (size_t i = 0; i < n; ++i)
    if (verdict[i] != 0) dropped->push_back(rp.g[i]);
  return CP2_OK;
}

}  // namespace

int cp2i::fill_read_checkpoint(std::string* err, const char* path, FillCheckpoint* ck) { return read_checkpoint(err, path, ck); }

extern "C" int cp2_fill_save(const void* fill, const char* path) try {
  const cp2_fill_session* f = session(fill);
  if (!f || !path) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  if (f->plan.finished) {
    ctx->err = "fill: the session is finished: its durable form is the kept cache of cp2_fill_finish, not a checkpoint";
    return CP2_ERR_INVALID;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<uint8_t> buf;
  FillCkptLayout l;
  if (!fill_ckpt_begin(session_meta(f), f->plan.bits, &buf, &l)) {
    ctx->err = "fill: the session is larger than a checkpoint describes";
    return CP2_ERR_INVALID;
  }
  // layer 0 in one download; rows of absent blocks hold whatever the allocation held and are zeroed on the host before anything is written
  CP2_HIP(ctx, hipMemcpyAsync(buf.data() + l.layer0_at, f->compact.p, (size_t)l.total * 32, hipMemcpyDeviceToHost, ctx->stream));
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  fill_ckpt_seal(&buf, l);
  CP2_TRY(write_checkpoint_file(ctx, path, buf));
  if (std::getenv("CP2_TRACE"))
    std::fprintf(stderr, "[cp2 trace] fill save: %llu of %llu block(s) present, %zu bytes\n", (unsigned long long)f->plan.n_present,
                 (unsigned long long)f->plan.total(), buf.size());
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// What cp2_fill_resume and cp2_fill_resume_nodes do with a checkpoint they have read (`ck`: meta, presence bitmap, layer 0): is it a
// description of exactly this session, what the slot files can no longer back, the session, the re-check.  `dropped`: the global indices
// of the blocks taken back.
static int resume_checked(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, const uint8_t* slot_roots, const char* path,
                          int flags, FillCheckpoint& ck, std::unique_ptr<cp2_fill_session>* out, std::vector<uint64_t>* dropped_out) {
  const auto t0 = std::chrono::steady_clock::now();
  FillCkptMeta want;
  want.cell_size = cfg->cell_size; want.block_size = cfg->block_size; want.n_cells = cfg->n_cells; want.n_slots = cfg->n_slots;
  want.first_slot = first_slot; want.n_local = n_local;
  want.src = cfg->file_base ? FILL_SRC_FILE : FILL_SRC_FAKE;
  want.seed = cfg->seed;
  if (cfg->file_base) want.file_base = cfg->file_base;
  want.roots.resize(n_local * 32);
  for (uint64_t s = 0; s < n_local; ++s) canonical_felt(slot_roots + s * 32, &want.roots[s * 32]);
  const std::string differs = fill_ckpt_differs(ck.meta, want);
  if (!differs.empty()) {
    ctx->err = "fill: checkpoint " + std::string(path) + " describes another session: " + differs;
    return CP2_ERR_INVALID;
  }
  const bool recheck = !(flags & CP2_RESUME_TRUST_FILES);
  const uint64_t n_blocks = ck.meta.n_blocks();
  uint64_t present = 0;
  for (uint64_t w : ck.bits) present += (uint64_t)__builtin_popcountll(w);
  // slot files first: what a file is too short to back (or no file at all) is dropped without a read; absence is a state, not an error
  std::vector<uint64_t>& dropped = *dropped_out;
  dropped.clear();
  if (recheck && cfg->file_base) {
    std::vector<uint64_t> whole;
    std::string bad;
    if (!fill_slot_files_cover(want.file_base, first_slot, n_local, cfg->block_size, &whole, &bad)) {
      ctx->err = slot_file_error(bad, 0);
      return CP2_ERR_IO;
    }
    fill_ckpt_drop_short(whole, n_blocks, &ck.bits, &ck.layer0, &dropped);
  }
  std::unique_ptr<cp2_fill_session> f;
  CP2_TRY(session_open(ctx, cfg, first_slot, n_local, slot_roots, &f));
  if (!f->plan.restore(ck.bits)) {
    ctx->err = "fill: checkpoint " + std::string(path) + " is corrupt: its bitmap is not one of this session";
    return CP2_ERR_IO;
  }
  CP2_HIP(ctx, hipMemcpyAsync(f->compact.p, ck.layer0.data(), ck.layer0.size(), hipMemcpyHostToDevice, ctx->stream));
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t n_read = 0;
  double bytes = 0;
  if (recheck) {
    std::vector<uint64_t> changed;
    CP2_TRY(recheck_present(f.get(), &changed, &n_read, &bytes));
    (void)f->plan.drop(changed.data(), changed.size());
    dropped.insert(dropped.end(), changed.begin(), changed.end());
  }
  if (std::getenv("CP2_TRACE")) {
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "[cp2 trace] fill resume: %llu block(s) present in the checkpoint, %llu re-read, %zu dropped, %.0f bytes, %.3f s (%.2f GB/s)\n",
                 (unsigned long long)present, (unsigned long long)n_read, dropped.size(), bytes, seconds, seconds > 0 ? bytes / seconds / 1e9 : 0.0);
  }
  *out = std::move(f);
  return CP2_OK;
}

extern "C" int cp2_fill_resume(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, const uint8_t* slot_roots, const char* path,
                               int flags, void** out, uint64_t* n_dropped) try {
  if (!ctx || !cfg || !out || !path) return CP2_ERR_INVALID;
  *out = nullptr;
  if (flags & ~CP2_RESUME_TRUST_FILES) {
    ctx->err = "fill: unknown resume flag bits";
    return CP2_ERR_INVALID;
  }
  CP2_TRY(fill_session_check(ctx, cfg, first_slot, n_local, slot_roots));
  // the checkpoint: intact, then a description of exactly this session
  FillCheckpoint ck;
  CP2_TRY(read_checkpoint(&ctx->err, path, &ck));
  std::unique_ptr<cp2_fill_session> f;
  std::vector<uint64_t> dropped;
  CP2_TRY(resume_checked(ctx, cfg, first_slot, n_local, slot_roots, path, flags, ck, &f, &dropped));
  if (n_dropped) *n_dropped = dropped.size();
  *out = f.release();
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// ---- sessions that serve ------------------------------------------------------------------------------------------------------------------
extern "C" int cp2_fill_keep_nodes(void* fill) try {
  cp2_fill_session* f = session(fill);
  if (!f) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  FillPlan& plan = f->plan;
  if (plan.finished) {
    ctx->err = "fill: the session is finished: its proofs come from the dataset (cp2_dataset_block_proofs)";
    return CP2_ERR_INVALID;
  }
  if (plan.keeps_nodes) return CP2_OK;               // one-way, and once
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  // the two tables the kernel takes a row from: layer_off, then layer_size
  const size_t layers = plan.csizes.size();
  std::vector<uint64_t> tab(2 * layers);
  for (size_t l = 0; l < layers; ++l) {
    tab[l] = plan.coff[l];
    tab[layers + l] = plan.csizes[l];
  }
  DevBuf d_tab;
  CP2_TRY(d_tab.alloc(ctx, tab.size() * 8));
  CP2_HIP(ctx, hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  // layer 0: the rows of absent blocks hold whatever the allocation held, and no kernel may read a row that was never written
  const size_t total = (size_t)plan.total();
  std::vector<uint8_t> layer0;
  if (plan.n_present == 0) {
    CP2_HIP(ctx, hipMemsetAsync(f->compact.p, 0, total * 32, ctx->stream));
  } else if (plan.n_missing()) {
    layer0.resize(total * 32);
    CP2_HIP(ctx, hipMemcpyAsync(layer0.data(), f->compact.p, total * 32, hipMemcpyDeviceToHost, ctx->stream));
    CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t g = 0; g < total; ++g)
      if (!((plan.bits[g >> 6] >> (g & 63)) & 1)) std::memset(&layer0[g * 32], 0, 32);
    CP2_HIP(ctx, hipMemcpyAsync(f->compact.p, layer0.data(), total * 32, hipMemcpyHostToDevice, ctx->stream));
  }
  // every upper layer once, exactly as finish builds them; a parent of an unknown child comes out as a value nobody reads
  CP2_TRY(merkle_trees_dev(ctx, f->compact.p, plan.n_blocks, plan.n_local, f->compact.p, true));
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "fill: building the upper layers failed on the device";
    return CP2_ERR_HIP;
  }
  hand_over(d_tab, f->layer_tab);
  plan.derive_from_presence();
  plan.keeps_nodes = true;
  if (std::getenv("CP2_TRACE")) {
    uint64_t servable = 0;
    for (uint64_t s = 0; s < plan.n_local; ++s)
      for (uint64_t b = 0; b < plan.n_blocks; ++b) servable += plan.servable(s, b);
    std::fprintf(stderr, "[cp2 trace] fill keep nodes: %llu of %llu block(s) present, %llu servable, %zu layer(s) built, %.3f ms\n",
                 (unsigned long long)plan.n_present, (unsigned long long)plan.total(), (unsigned long long)servable, layers - 1,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
  }
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_fill_block_proofs(void* fill, const uint64_t* slot_block, size_t n, uint32_t* status, uint8_t* block_roots, uint8_t* paths) try {
  cp2_fill_session* f = session(fill);
  if (!f) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  const FillPlan& plan = f->plan;
  if (n && (!slot_block || !status)) {
    ctx->err = "fill proofs: slot_block and status must not be NULL when n > 0";
    return CP2_ERR_INVALID;
  }
  if (plan.finished) {
    ctx->err = "fill proofs: the session is finished: its proofs come from the dataset (cp2_dataset_block_proofs)";
    return CP2_ERR_INVALID;
  }
  if (!plan.keeps_nodes) {
    ctx->err = "fill proofs: this session does not keep the nodes of the paths it proves: call cp2_fill_keep_nodes first";
    return CP2_ERR_INVALID;
  }
  std::string err;
  if (!block_proofs_validate(slot_block, n, plan.first_slot, plan.n_local, plan.n_blocks, &err)) {
    ctx->err = "fill proofs:" + err.substr(err.find(':') + 1);
    return CP2_ERR_INVALID;
  }
  if (n == 0) return CP2_OK;
  const auto t0 = std::chrono::steady_clock::now();
  // the statuses, from the host's two bitmaps
  std::vector<uint32_t> st(n);
  size_t count[3] = {0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    st[i] = plan.proof_status(slot_block[2 * i] - plan.first_slot, slot_block[2 * i + 1]);
    ++count[st[i]];
  }
  if (block_roots || paths) {
    CP2_REFUSE_STUCK(ctx);
    CP2_HIP(ctx, hipSetDevice(ctx->device));
    // the rows of every request: its block root, then its siblings bottom first; a request that is not served names no row at all
    const size_t depth = plan.depth(), per = depth + 1;
    std::vector<uint64_t> rows(n * per, BLOCK_PROOF_NO_ROW);
    for (size_t i = 0; i < n; ++i) {
      if (st[i] != FILL_PROOF_OK) continue;
      const uint64_t s = slot_block[2 * i], b = slot_block[2 * i + 1];
      rows[i * per] = plan.dest_row(s, b);
      block_proof_rows(plan.coff, plan.csizes, s - plan.first_slot, b, depth, &rows[i * per + 1]);
    }
    CP2_TRY(gather_block_proofs(ctx, f->compact.p, plan.rows, rows, depth, "fill proofs: a row lies outside the session's buffer", block_roots, paths));
  }
  std::copy(st.begin(), st.end(), status);
  if (std::getenv("CP2_TRACE"))
    std::fprintf(stderr, "[cp2 trace] fill proofs: %zu request(s), %zu served, %zu absent, %zu partial, %.6f s\n", n, count[FILL_PROOF_OK],
                 count[FILL_PROOF_ABSENT], count[FILL_PROOF_PARTIAL], std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// ---- paths that stop at a node the session holds ---------------------------------------------------------------------------------------------
extern "C" int cp2_fill_anchors(const void* fill, const uint64_t* slot_block, size_t n, uint32_t* levels) try {
  const cp2_fill_session* f = session(fill);
  if (!f) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  const FillPlan& plan = f->plan;
  if (n && (!slot_block || !levels)) {
    ctx->err = "fill anchors: slot_block and levels must not be NULL when n > 0";
    return CP2_ERR_INVALID;
  }
  if (plan.finished) {
    ctx->err = "fill anchors: the session is finished: it accepts only cp2_fill_free";
    return CP2_ERR_INVALID;
  }
  std::string err;
  if (!block_proofs_validate(slot_block, n, plan.first_slot, plan.n_local, plan.n_blocks, &err)) {
    ctx->err = "fill anchors:" + err.substr(err.find(':') + 1);
    return CP2_ERR_INVALID;
  }
  for (size_t i = 0; i < n; ++i) levels[i] = (uint32_t)plan.anchor_level(slot_block[2 * i] - plan.first_slot, slot_block[2 * i + 1]);
  return CP2_OK;
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_fill_add_anchored(void* fill, const uint64_t* slot_block, const uint8_t* data, const uint32_t* levels, const uint8_t* paths,
                                     size_t n, uint32_t* status, size_t* n_new) try {
  cp2_fill_session* f = session(fill);
  if (!f) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  if (n && (!slot_block || !data || !levels || !status)) {
    ctx->err = "fill: slot_block, data, levels and status must not be NULL when n > 0";
    return CP2_ERR_INVALID;
  }
  std::string err;
  if (!f->plan.validate_anchored(slot_block, levels, n, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (!paths)
    for (size_t i = 0; i < n; ++i)
      if (levels[i]) {
        ctx->err = "fill: request " + std::to_string(i) + ": paths must not be NULL when a level is not 0";
        return CP2_ERR_INVALID;
      }
  if (n == 0) {
    if (n_new) *n_new = 0;
    return CP2_OK;
  }
  return fill_add_checked(f, slot_block, data, paths, levels, n, status, n_new);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// ---- adopting blocks from disk ------------------------------------------------------------------------------------------------------------
namespace {

// The absent blocks of local slots [s0, s0 + ns) that their files cover (fill_slot_files_cover), read with the re-check's reader
// (fill_read_chunk) and reduced to their block roots on repair's data path; the roots land in `fresh` (one row per block of the read plan,
// in its order).  Nothing of the session is touched: the caller takes the roots over once every read has succeeded.
int adopt_read(cp2_fill_session* f, uint64_t s0, uint64_t ns, std::vector<uint64_t>* read_bits, FillReadPlan* rp, DevBuf* fresh) {
  cp2_ctx* ctx = f->ctx;
  const cp2_config& c = f->cfg;
  const FillPlan& plan = f->plan;
  const size_t bs = c.block_size;
  std::vector<uint64_t> whole;
  std::string bad;
  if (!fill_slot_files_cover(f->file_base, plan.first_slot + s0, ns, bs, &whole, &bad)) {   // absence is a state, as in cp2_fill_resume
    ctx->err = slot_file_error(bad, 0);
    return CP2_ERR_IO;
  }
  *read_bits = adopt_read_bits(plan, s0, ns, whole);
  const size_t chunk = std::max<size_t>(1, (ctx->stage_bytes / 2) / bs);          // repair_check_with's chunks
  *rp = fill_read_plan(*read_bits, plan.total(), plan.n_blocks, chunk);
  const size_t n = rp->g.size();
  if (n == 0) return CP2_OK;
  CP2_TRY(fresh->scratch(ctx, n * 32));
  std::unique_ptr<uint8_t[]> host(new uint8_t[std::min(n, chunk) * bs]);
  std::vector<uint32_t> verdict(std::min(n, chunk));
  for (size_t k = 0; k < rp->n_chunks(); ++k) {
    const size_t i0 = rp->chunk_begin(k), m = rp->chunk_end(k) - i0;
    int err = 0;
    if (!fill_read_chunk(*rp, k, f->file_base, plan.first_slot, bs, host.get(), &bad, &err)) {
      ctx->err = slot_file_error(bad, err);
      return CP2_ERR_IO;
    }
    RepairJudge judge;                                   // no verdict here: the chunk's roots are kept for the judgement of the whole tree
    judge.verdicts = [&](const uint8_t* roots, size_t c0, size_t mm, uint32_t* v, hipStream_t st) -> int {
      CP2_HIP(ctx, hipMemsetAsync(v, 0, mm * 4, st));
      CP2_HIP(ctx, hipMemcpyAsync(fresh->u8() + (i0 + c0) * 32, roots, mm * 32, hipMemcpyDeviceToDevice, st));
      return CP2_OK;
    };
    CP2_TRY(repair_check_with(ctx, c.cell_size, bs, host.get(), m, verdict.data(), judge));
  }
  return CP2_OK;
}

}  // namespace

extern "C" int cp2_fill_adopt(void* fill, uint64_t first_slot, uint64_t n_slots, int flags, uint64_t* n_read, uint64_t* n_adopted) try {
  cp2_fill_session* f = session(fill);
  if (!f) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  FillPlan& plan = f->plan;
  if (plan.finished) {
    ctx->err = "fill adopt: the session is finished: it accepts only cp2_fill_free";
    return CP2_ERR_INVALID;
  }
  if (!plan.keeps_nodes) {
    ctx->err = "fill: this session does not keep the nodes of the paths it proves: call cp2_fill_keep_nodes first";
    return CP2_ERR_INVALID;
  }
  if (flags & ~CP2_ADOPT_NO_READ) {
    ctx->err = "fill adopt: unknown flag bits";
    return CP2_ERR_INVALID;
  }
  if (n_slots == 0) {
    first_slot = plan.first_slot;
    n_slots = plan.n_local;
  }
  if (first_slot < plan.first_slot || first_slot - plan.first_slot >= plan.n_local || n_slots > plan.n_local - (first_slot - plan.first_slot)) {
    ctx->err = "fill adopt: slots " + std::to_string(first_slot) + " + " + std::to_string(n_slots) + " are not inside the local range " +
               std::to_string(plan.first_slot) + " + " + std::to_string(plan.n_local);
    return CP2_ERR_INVALID;
  }
  if (!f->from_file) {
    ctx->err = "fill adopt: a session of the fake source has no slot files to adopt from";
    return CP2_ERR_INVALID;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t s0 = first_slot - plan.first_slot, ns = n_slots;
  const size_t depth = plan.depth(), total = (size_t)plan.total();
  // the reads: nothing of the session changes until every one of them has succeeded
  uint64_t read = 0;
  if (!(flags & CP2_ADOPT_NO_READ)) {
    std::vector<uint64_t> read_bits;
    FillReadPlan rp;
    DevBuf fresh;
    CP2_TRY(adopt_read(f, s0, ns, &read_bits, &rp, &fresh));
    read = rp.g.size();
    if (!f->adopt_roots.p) CP2_TRY(f->adopt_roots.alloc(ctx, total * 32));
    for (size_t i = 0; i < rp.g.size();) {               // runs of consecutive blocks: one copy each (an intact file is one run)
      size_t j = i + 1;
      while (j < rp.g.size() && rp.g[j] == rp.g[j - 1] + 1) ++j;
      CP2_HIP(ctx, hipMemcpyAsync(f->adopt_roots.u8() + (size_t)rp.g[i] * 32, fresh.u8() + i * 32, (j - i) * 32, hipMemcpyDeviceToDevice, ctx->stream));
      i = j;
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
      (void)hipGetLastError();
      ctx->err = "fill adopt: keeping the block roots failed on the device";
      return CP2_ERR_HIP;
    }
    adopt_remember(plan, s0, ns, read_bits, &f->adopt_have);
  }
  // the judgement: flag bytes up, one launch per layer, the resolve, flag bytes down
  uint64_t n_cand = 0;
  std::vector<uint8_t> up = adopt_flags(plan, s0, ns, &f->adopt_have, &n_cand);
  AdoptVerdict verdict;
  verdict.adopted.resize((size_t)ns);
  if (n_cand) {
    const size_t rows = plan.rows;
    std::vector<uint64_t> off(plan.coff.begin(), plan.coff.end()), sizes(plan.csizes.begin(), plan.csizes.end());
    const uint64_t* tab = static_cast<const uint64_t*>(f->layer_tab.p);
    DevBuf d_cand, d_flags, d_out;
    CP2_TRY(d_cand.scratch(ctx, rows * 32));
    CP2_TRY(d_flags.scratch(ctx, rows));
    CP2_TRY(d_out.scratch(ctx, rows));
    std::vector<uint8_t> down(rows);
    CP2_HIP(ctx, hipMemcpyAsync(d_cand.p, f->adopt_roots.p, total * 32, hipMemcpyDeviceToDevice, ctx->stream));   // (coff[0] == 0: layer 0 comes first)
    CP2_HIP(ctx, hipMemcpyAsync(d_flags.p, up.data(), rows, hipMemcpyHostToDevice, ctx->stream));
    CP2_HIP(ctx, hipMemsetAsync(d_out.p, 0, rows, ctx->stream));
    CP2_HIP(ctx, cp2k::launch_adopt_layers(f->compact.p, d_cand.p, d_flags.u8(), f->slot_roots.p, off.data(), sizes.data(), (uint32_t)depth,
                                           plan.n_local, s0, ns, rows, ctx->stream));
    CP2_HIP(ctx, cp2k::launch_adopt_resolve(f->compact.p, d_cand.p, d_flags.u8(), d_out.u8(), tab, tab + depth + 1, (uint32_t)depth, plan.n_local,
                                            s0, ns, plan.coff[depth], rows, ctx->stream));
    CP2_HIP(ctx, hipMemcpyAsync(down.data(), d_out.p, rows, hipMemcpyDeviceToHost, ctx->stream));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
      (void)hipGetLastError();
      ctx->err = "fill adopt: the judgement failed on the device";
      return CP2_ERR_HIP;
    }
    verdict = adopt_apply(&plan, s0, ns, down);           // the proved rows are known from here on: they are authentic and stored
  }
  // presence: each file with adopted blocks made durable once, then its bits
  int r = CP2_OK;
  uint64_t adopted = 0;
  for (uint64_t i = 0; i < ns; ++i) {
    const std::vector<uint64_t>& blocks = verdict.adopted[(size_t)i];
    if (blocks.empty()) continue;
    const std::string fname = slot_file_name(f->file_base, plan.first_slot + s0 + i);
    const int fd = open(fname.c_str(), O_RDONLY | O_CLOEXEC);
    const int e = fd < 0 ? errno : fdatasync(fd) != 0 ? errno : 0;
    if (fd >= 0) close(fd);
    if (e) {                                             // this file's blocks stay absent; their nodes stay known, as with CP2_FILL_UNWRITTEN
      if (r == CP2_OK) ctx->err = "fill adopt: cannot sync " + fname + ": " + std::strerror(e);
      r = CP2_ERR_IO;
      continue;
    }
    adopted += adopt_commit(&plan, blocks);
  }
  if (n_read) *n_read = read;
  if (n_adopted) *n_adopted = adopted;
  if (std::getenv("CP2_TRACE")) {
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), bytes = (double)read * (double)f->cfg.block_size;
    std::fprintf(stderr, "[cp2 trace] fill adopt: %llu block(s) read, %llu candidate(s), %llu adopted, %llu row(s) proved, %.0f bytes, %.3f s (%.2f GB/s)\n",
                 (unsigned long long)read, (unsigned long long)n_cand, (unsigned long long)adopted, (unsigned long long)verdict.rows_proved, bytes,
                 seconds, seconds > 0 ? bytes / seconds / 1e9 : 0.0);
  }
  return r;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// ---- checkpoints that carry the kept nodes ----------------------------------------------------------------------------------------------------
extern "C" int cp2_fill_save_nodes(const void* fill, const char* path) try {
  const cp2_fill_session* f = session(fill);
  if (!f || !path) return CP2_ERR_INVALID;
  cp2_ctx* ctx = f->ctx;
  const FillPlan& plan = f->plan;
  if (plan.finished) {
    ctx->err = "fill: the session is finished: its durable form is the kept cache of cp2_fill_finish, not a checkpoint";
    return CP2_ERR_INVALID;
  }
  if (!plan.keeps_nodes) {
    ctx->err = "fill: this session does not keep the nodes of the paths it proves: call cp2_fill_keep_nodes first, or save it with cp2_fill_save";
    return CP2_ERR_INVALID;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const FillCkptMeta meta = session_meta(f);
  NodeCkptLayout l;
  if (meta.cell_size == 0 || meta.block_size < meta.cell_size || !node_ckpt_layout(meta.file_base.size(), meta.n_local, meta.n_blocks(), &l)) {
    ctx->err = "fill: the session is larger than a checkpoint describes";
    return CP2_ERR_INVALID;
  }
  // the buffer below the top rows in one download; what is neither present nor known never reaches the file
  std::vector<uint8_t> image(plan.rows * 32), buf;
  const size_t below_top = plan.coff[plan.depth()] * 32;
  CP2_HIP(ctx, hipMemcpyAsync(image.data(), f->compact.p, below_top, hipMemcpyDeviceToHost, ctx->stream));
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!node_ckpt_serialise(meta, plan, image.data(), &buf)) {
    ctx->err = "fill: the session is larger than a checkpoint describes";
    return CP2_ERR_INVALID;
  }
  CP2_TRY(write_checkpoint_file(ctx, path, buf));
  if (std::getenv("CP2_TRACE")) {
    uint64_t known = 0;
    for (uint64_t w : plan.known) known += (uint64_t)__builtin_popcountll(w);
    std::fprintf(stderr, "[cp2 trace] fill save nodes: %llu of %llu block(s) present, %llu of %zu row(s) known, %zu bytes\n",
                 (unsigned long long)plan.n_present, (unsigned long long)plan.total(), (unsigned long long)known, plan.rows, buf.size());
  }
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_fill_resume_nodes(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, const uint8_t* slot_roots,
                                     const char* path, int flags, void** out, uint64_t* n_dropped, uint64_t* n_restored, uint64_t* n_unproved,
                                     uint64_t* n_rejected) try {
  if (!ctx || !cfg || !out || !path) return CP2_ERR_INVALID;
  *out = nullptr;
  if (flags & ~CP2_RESUME_TRUST_FILES) {
    ctx->err = "fill: unknown resume flag bits";
    return CP2_ERR_INVALID;
  }
  CP2_TRY(fill_session_check(ctx, cfg, first_slot, n_local, slot_roots));
  const auto t0 = std::chrono::steady_clock::now();
  // either format: a CP2FILL1 file states no nodes, and the result is cp2_fill_resume followed by cp2_fill_keep_nodes
  NodeCheckpoint ck;
  const bool with_nodes = !file_has_magic(path, "CP2FILL1");
  if (with_nodes) CP2_TRY(read_node_checkpoint(ctx, path, &ck));
  else CP2_TRY(read_checkpoint(&ctx->err, path, &ck.base));
  // layer 0 as the file states it: the shared resume zeroes the rows of the blocks it drops, and those rows are candidates
  const std::vector<uint8_t> stated0 = with_nodes ? ck.base.layer0 : std::vector<uint8_t>();
  std::unique_ptr<cp2_fill_session> f;
  std::vector<uint64_t> dropped;
  CP2_TRY(resume_checked(ctx, cfg, first_slot, n_local, slot_roots, path, flags, ck.base, &f, &dropped));
  // step 1: D, what presence gives -- absent rows zeroed, every upper layer built once, derive_from_presence
  CP2_TRY(cp2_fill_keep_nodes(f.get()));
  FillPlan& plan = f->plan;
  NodeRestoreCounts counts;
  uint64_t n_cand = 0;
  if (with_nodes) {
    // step 2: the candidates, in a buffer of their own
    NodeRestorePlan rp;
    if (!node_restore_plan(plan, ck.known, stated0, ck.mid, &rp)) {
      ctx->err = "fill: checkpoint " + std::string(path) + " is corrupt: its known bitmap is not one of this session";
      return CP2_ERR_IO;
    }
    n_cand = rp.n_cand;
    std::vector<uint8_t> down = rp.flags;
    if (n_cand) {
      // step 3: top-down, one launch per layer; the flag bytes come back once
      const size_t rows = plan.rows;
      std::vector<uint64_t> off(plan.coff.begin(), plan.coff.end()), sizes(plan.csizes.begin(), plan.csizes.end());
      DevBuf d_cand, d_flags;
      CP2_TRY(d_cand.scratch(ctx, rows * 32));
      CP2_TRY(d_flags.scratch(ctx, rows));
      CP2_HIP(ctx, hipMemcpyAsync(d_cand.p, rp.cand.data(), rows * 32, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, hipMemcpyAsync(d_flags.p, rp.flags.data(), rows, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, cp2k::launch_nodes_restore_layers(f->compact.p, d_cand.p, d_flags.u8(), f->slot_roots.p, off.data(), sizes.data(),
                                                     (uint32_t)plan.depth(), plan.n_local, rows, ctx->stream));
      CP2_HIP(ctx, hipMemcpyAsync(down.data(), d_flags.p, rows, hipMemcpyDeviceToHost, ctx->stream));
      if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        ctx->err = "fill: restoring the kept nodes failed on the device";
        return CP2_ERR_HIP;
      }
    }
    // a top row whose bit is taken over holds what a proved path left there: the stated root
    const uint64_t top = plan.coff[plan.depth()];
    for (uint64_t s = 0; s < plan.n_local;) {
      if (!node_ckpt_bit(ck.known, top + s) || plan.is_known(top + s)) { ++s; continue; }
      uint64_t e = s + 1;
      while (e < plan.n_local && node_ckpt_bit(ck.known, top + e) && !plan.is_known(top + e)) ++e;
      CP2_HIP(ctx, hipMemcpyAsync(f->compact.u8() + (size_t)(top + s) * 32, f->slot_roots.u8() + (size_t)s * 32, (size_t)(e - s) * 32,
                                  hipMemcpyDeviceToDevice, ctx->stream));
      s = e;
    }
    CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    counts = node_restore_apply(&plan, ck.known, rp.flags, down);
  }
  if (std::getenv("CP2_TRACE"))
    std::fprintf(stderr, "[cp2 trace] fill resume nodes: %s, %llu candidate row(s), %llu restored, %llu rejected, %llu unproved, %zu dropped, %.3f s\n",
                 with_nodes ? "CP2FILL2" : "CP2FILL1 (no nodes stated)", (unsigned long long)n_cand, (unsigned long long)counts.restored,
                 (unsigned long long)counts.rejected, (unsigned long long)counts.unproved, dropped.size(),
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  if (n_dropped) *n_dropped = dropped.size();
  if (n_restored) *n_restored = counts.restored;
  if (n_unproved) *n_unproved = counts.unproved;
  if (n_rejected) *n_rejected = counts.rejected;
  *out = f.release();
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" void cp2_fill_free(void* fill) { delete session(fill); }
