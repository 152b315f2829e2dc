// Block proofs behind the C ABI (include/codex_p2.h): cp2_block_proof_depth, cp2_dataset_block_proofs, cp2_blocks_verify and
// cp2_dataset_repair_blocks_proved.
//
// The proof of network block b of a slot is merkleProof(bigTree, b) (reference/nim/proof_input/src/merkle.nim:21-42): the block root and
// one sibling per layer of the tree over the slot's block roots, zero where the sibling is out of range.  A dataset that keeps that tree
// (every node, or the compact layers) SERVES such proofs with one gather; a node that holds nothing but a slot root CHECKS a block
// against it: the candidate's cells are hashed and reduced to the block root on repair's data path (repair_check_with, repair.cpp), and
// k_block_path_roots runs reconstructRoot (merkle.nim:51-74) from that root up the path, one verdict per request.  With a path beside
// each candidate a repair needs no kept block roots, so it works on a roots-only dataset too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "block_proof_plan.hpp"
#include "dataset_obj.hpp"
#include "repair.hpp"

using namespace cp2i;

static_assert(BLOCK_PROOF_NO_ROW == NO_ROW, "k_gather_rows zero-fills the rows the plan marks as absent");
static_assert(CP2_BLOCK_MATCH == CP2_REPAIR_MATCH && CP2_BLOCK_MISMATCH == CP2_REPAIR_MISMATCH, "repair_check_with's verdicts serve both");

namespace {

// n candidates checked against slot roots in device memory (d_slot_roots: 32-byte rows, indexed by root_block[2 i]); root_block and
// paths are host arrays.  status[i] = CP2_BLOCK_MATCH / _MISMATCH; block_roots (host, may be NULL) receives what each candidate hashed to.
int verify_paths(cp2_ctx* ctx, size_t cell_size, size_t block_size, uint64_t n_blocks, const void* d_slot_roots, const uint64_t* root_block,
                 const uint8_t* data, const uint8_t* paths, size_t n, uint32_t* status, uint8_t* block_roots) {
  const size_t depth = block_proof_depth(n_blocks), path_bytes = depth * 32;
  DevBuf d_req, d_paths, d_out;                      // (go after the streams have drained: DevBuf::release)
  RepairJudge judge;
  judge.begin = [&](size_t chunk) -> int {
    CP2_TRY(d_req.scratch(ctx, n * 16));
    CP2_TRY(d_paths.scratch(ctx, chunk * path_bytes));
    if (block_roots) CP2_TRY(d_out.scratch(ctx, n * 32));
    CP2_HIP(ctx, hipMemcpyAsync(d_req.p, root_block, n * 16, hipMemcpyHostToDevice, ctx->stream));
    return CP2_OK;
  };
  // the chunk's paths travel with the chunk: depth x 32 bytes per block (the previous chunk's walk, earlier on this stream, has read its own)
  judge.stage = [&](size_t c0, size_t m, hipStream_t st) -> int {
    CP2_HIP(ctx, hipMemcpyAsync(d_paths.p, paths + c0 * path_bytes, m * path_bytes, hipMemcpyHostToDevice, st));
    return CP2_OK;
  };
  judge.verdicts = [&](const uint8_t* fresh, size_t c0, size_t m, uint32_t* verdict, hipStream_t st) -> int {
    CP2_HIP(ctx, cp2k::launch_block_path_roots(fresh, d_paths.p, static_cast<const uint64_t*>(d_req.p) + 2 * c0, d_slot_roots, n_blocks, (uint32_t)depth,
                                               m, verdict, block_roots ? d_out.u8() + c0 * 32 : nullptr, st));
    return CP2_OK;
  };
  std::vector<uint32_t> st(n);
  CP2_TRY(repair_check_with(ctx, cell_size, block_size, data, n, st.data(), judge));
  if (block_roots) {
    std::vector<uint8_t> roots(n * 32);
    CP2_HIP(ctx, hipMemcpyAsync(roots.data(), d_out.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(block_roots, roots.data(), n * 32);
  }
  std::copy(st.begin(), st.end(), status);
  return CP2_OK;
}

void verify_trace(size_t n, const uint32_t* status, size_t block_size, size_t depth, double seconds) {
  if (!std::getenv("CP2_TRACE")) return;
  size_t matched = 0;
  for (size_t i = 0; i < n; ++i) matched += status[i] == CP2_BLOCK_MATCH;
  const double bytes = (double)n * (double)block_size;
  std::fprintf(stderr, "[cp2 trace] block verify: %zu request(s) of depth %zu, %zu matched, %.0f bytes, %.3f s (%.2f GB/s)\n", n, depth, matched, bytes,
               seconds, seconds > 0 ? bytes / seconds / 1e9 : 0.0);
}

}  // namespace

int cp2i::gather_block_proofs(cp2_ctx* ctx, const void* nodes, size_t n_rows, const std::vector<uint64_t>& rows, size_t depth, const char* outside,
                              uint8_t* block_roots, uint8_t* paths) {
  for (uint64_t r : rows)
    if (r != BLOCK_PROOF_NO_ROW && r >= n_rows) {
      ctx->err = outside;
      return CP2_ERR_INVALID;
    }
  const size_t per = depth + 1, n = rows.size() / per;
  // the one gather is by address (k_gather_addr): a row index is an address once the buffer is named
  std::vector<uint64_t> addr(rows.size());
  for (size_t r = 0; r < rows.size(); ++r) addr[r] = rows[r] == BLOCK_PROOF_NO_ROW ? 0 : (uint64_t)reinterpret_cast<uintptr_t>(nodes) + rows[r] * 32;
  std::vector<uint8_t> out(rows.size() * 32);
  CP2_TRY(gather_rows_by_addr(ctx, addr, out.data()));
  for (size_t i = 0; i < n; ++i) {
    if (block_roots) std::memcpy(block_roots + i * 32, &out[i * per * 32], 32);
    if (paths) std::memcpy(paths + i * depth * 32, &out[(i * per + 1) * 32], depth * 32);
  }
  return CP2_OK;
}

int cp2i::gather_rows_by_addr(cp2_ctx* ctx, const std::vector<uint64_t>& addr, uint8_t* out) {
  if (addr.empty()) return CP2_OK;
  DevBuf d_addr, d_out;
  CP2_TRY(d_addr.scratch(ctx, addr.size() * 8));
  CP2_TRY(d_out.scratch(ctx, addr.size() * 32));
  CP2_HIP(ctx, hipMemcpyAsync(d_addr.p, addr.data(), addr.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  CP2_HIP(ctx, cp2k::launch_gather_addr(static_cast<const uint64_t*>(d_addr.p), addr.size(), 32, d_out.p, ctx->stream));
  CP2_HIP(ctx, hipMemcpyAsync(out, d_out.p, addr.size() * 32, hipMemcpyDeviceToHost, ctx->stream));
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return CP2_OK;
}

extern "C" size_t cp2_block_proof_depth(size_t cell_size, size_t block_size, size_t n_cells) {
  if (trees_check_geometry(cell_size, block_size, n_cells, 1) != CP2_OK) return 0;
  return block_proof_depth(n_cells / (block_size / cell_size));
}

extern "C" int cp2_dataset_block_proofs(cp2_dataset* ds, const uint64_t* slot_block, size_t n, uint8_t* block_roots, uint8_t* paths) try {
  if (!ds) return CP2_ERR_INVALID;
  cp2_ctx* ctx = ds->ctx;
  const cp2_config& c = ds->cfg;
  if (n && (!slot_block || !paths)) {
    ctx->err = "block proofs: slot_block and paths must not be NULL when n > 0";
    return CP2_ERR_INVALID;
  }
  if (repair_dataset_mode(ds) == 0) {
    ctx->err = "block proofs: this dataset keeps only its slot roots, no block roots and no layers above them to take a path from: build it with every "
               "node or the compact layers kept (cp2_set_keep_trees)";
    return CP2_ERR_INVALID;
  }
  const uint64_t n_blocks = c.n_cells / (c.block_size / c.cell_size);
  std::string err;
  if (!block_proofs_validate(slot_block, n, ds->first_slot, ds->n_local, n_blocks, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n == 0) return CP2_OK;
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  // the rows of every request: its block root, then its siblings bottom first (the big tree of every node kept, or the compact layers)
  const size_t depth = block_proof_depth(n_blocks), per = depth + 1;
  const std::vector<size_t>& offs = ds->trees ? ds->trees->toff : ds->coff;
  const std::vector<size_t>& sizes = ds->trees ? ds->trees->tsizes : ds->csizes;
  if (offs.size() != per || sizes.size() != per || (ds->trees && ds->trees->units_per_slot != 1)) {
    ctx->err = "block proofs: the kept layers of this dataset are not those of whole slot trees";
    return CP2_ERR_INVALID;
  }
  const RepairKept k = repair_dataset_kept(ds);
  std::vector<uint64_t> rows(n * per);
  for (size_t i = 0; i < n; ++i) {
    const uint64_t s = slot_block[2 * i], b = slot_block[2 * i + 1];
    rows[i * per] = repair_dataset_row(ds, s, b);
    block_proof_rows(offs, sizes, s - ds->first_slot, b, depth, &rows[i * per + 1]);
  }
  return gather_block_proofs(ctx, k.nodes, k.rows, rows, depth, "block proofs: a row lies outside the kept nodes", block_roots, paths);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_blocks_verify(cp2_ctx* ctx, size_t cell_size, size_t block_size, size_t n_cells, const uint8_t* slot_roots, size_t n_roots,
                                 const uint64_t* root_block, const uint8_t* data, const uint8_t* paths, size_t n, uint32_t* status,
                                 uint8_t* block_roots) try {
  if (!ctx) return CP2_ERR_INVALID;
  if (trees_check_geometry(cell_size, block_size, n_cells, 1) != CP2_OK) {
    ctx->err = "block verify: cell_size " + std::to_string(cell_size) + ", block_size " + std::to_string(block_size) + ", n_cells " +
               std::to_string(n_cells) + " is a geometry the tree builders refuse";
    return CP2_ERR_INVALID;
  }
  if (n && (!slot_roots || !root_block || !data || !paths || !status)) {
    ctx->err = "block verify: slot_roots, root_block, data, paths and status must not be NULL when n > 0";
    return CP2_ERR_INVALID;
  }
  const uint64_t n_blocks = n_cells / (block_size / cell_size);
  std::string err;
  if (!block_verify_validate(root_block, n, n_roots, n_blocks, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n == 0) return CP2_OK;
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  DevBuf d_slot_roots;                               // the slot roots once per call
  CP2_TRY(d_slot_roots.scratch(ctx, n_roots * 32));
  CP2_HIP(ctx, hipMemcpyAsync(d_slot_roots.p, slot_roots, n_roots * 32, hipMemcpyHostToDevice, ctx->stream));
  CP2_TRY(verify_paths(ctx, cell_size, block_size, n_blocks, d_slot_roots.p, root_block, data, paths, n, status, block_roots));
  verify_trace(n, status, block_size, block_proof_depth(n_blocks), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_dataset_repair_blocks_proved(cp2_dataset* ds, const uint64_t* slot_block, const uint8_t* data, const uint8_t* paths, size_t n,
                                                int flags, const char* cache_path, uint32_t* status, size_t* n_written) try {
  if (!ds) return CP2_ERR_INVALID;
  cp2_ctx* ctx = ds->ctx;
  const cp2_config& c = ds->cfg;
  std::string err;
  // repair's refusals without the roots-only one (tree mode stated as 1: a path needs no kept block root), plus the paths
  if (repair_refuse(c, ds->from_file, 1, slot_block, data, n, flags, status, ds->first_slot, ds->n_local, &err) != CP2_OK) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n && !paths) {
    ctx->err = "repair: paths must not be NULL when n > 0";
    return CP2_ERR_INVALID;
  }
  if (n == 0) {
    if (n_written) *n_written = 0;
    return CP2_OK;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  // verdicts against the dataset's own slot roots, whatever else it keeps: request i names root slot - first_slot of the local roots
  const uint64_t n_blocks = c.n_cells / (c.block_size / c.cell_size);
  std::vector<uint64_t> root_block(2 * n);
  for (size_t i = 0; i < n; ++i) {
    root_block[2 * i] = slot_block[2 * i] - ds->first_slot;
    root_block[2 * i + 1] = slot_block[2 * i + 1];
  }
  std::vector<uint32_t> st(n);
  CP2_TRY(verify_paths(ctx, c.cell_size, c.block_size, n_blocks, dataset_roots_dev(ds), root_block.data(), data, paths, n, st.data(), nullptr));
  size_t written_n = 0, restamped = 0;
  int r = CP2_OK;
  if (!(flags & CP2_REPAIR_CHECK_ONLY)) {
    std::vector<FileStamp> written;
    r = repair_write(ds->file_base, c.block_size, slot_block, data, n, st.data(), &written_n, &written, &err);
    if (cache_path && !written.empty()) {   // (after a failed file too: the files before it are written and synced)
      std::string rerr;
      const int rs = repair_restamp_caches({std::string(cache_path), std::string(cache_path) + ".kept"}, c, ds->n_local, c.n_cells, ds->first_slot, 1,
                                           ds->file_base, written, &restamped, &rerr);
      if (r == CP2_OK && rs != CP2_OK) { r = rs; err = rerr; }
    }
  }
  std::copy(st.begin(), st.end(), status);
  if (n_written) *n_written = written_n;
  if (r != CP2_OK) ctx->err = err;
  repair_trace("proved repair", n, status, written_n, c.block_size, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), restamped,
               cache_path != nullptr);
  return r;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
