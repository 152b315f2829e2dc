// Block repair behind the C ABI: cp2_dataset_repair_blocks (include/codex_p2.h); cp2_multi_dataset_repair_blocks (multi_gpu.cpp) runs
// repair_check per shard and repair_write / repair_restamp_caches once over all of them.
//
// A scrub names the network blocks of a slot that no longer hash to what the dataset keeps; the node fetches or re-decodes them and
// hands the candidates in here.  Each candidate is checked ALONE against the block root the dataset keeps for it (the last layer of a
// block tree when every node is kept, layer 0 of the compact layers): its cells are hashed by k_hash_cells, reduced to the block root by
// the layer kernel (one segment per block, exactly as the builders make block trees) and compared by k_repair_compare, one verdict per
// request.  Only candidates that match are written, grouped by slot file, each file synced once; the cache stamps of the files written
// then follow the writes, so that the next cp2_dataset_build_cached loads the cache instead of rebuilding the range.
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
#include <new>
#include <string>
#include <vector>

#include "dataset_obj.hpp"
#include "repair.hpp"

using namespace cp2i;

namespace {
constexpr size_t SMALL_BYTES = (size_t)32 << 20;     // pageable chunks up to this size: one upload, as cp2_hash_cells does
constexpr size_t PIECE_BYTES = (size_t)128 << 20;    // caller-pinned chunks are uploaded and hashed in pieces of this size

}  // namespace

int cp2i::repair_check(cp2_ctx* ctx, const RepairKept& k, size_t cell_size, size_t block_size, const uint8_t* data, const uint64_t* rows,
                       size_t n, uint32_t* status) {
  if (n == 0) return CP2_OK;
  DevBuf d_rows;                                     // (goes after the streams have drained: DevBuf::release)
  RepairJudge judge;
  judge.begin = [&](size_t) -> int {
    CP2_TRY(d_rows.scratch(ctx, n * 8));
    CP2_HIP(ctx, hipMemcpyAsync(d_rows.p, rows, n * 8, hipMemcpyHostToDevice, ctx->stream));
    return CP2_OK;
  };
  // each root against the kept row of its request
  judge.verdicts = [&](const uint8_t* fresh, size_t c0, size_t m, uint32_t* verdict, hipStream_t st) -> int {
    CP2_HIP(ctx, cp2k::launch_repair_compare(fresh, k.nodes, k.rows, static_cast<const uint64_t*>(d_rows.p) + c0, m, verdict, st));
    return CP2_OK;
  };
  return repair_check_with(ctx, cell_size, block_size, data, n, status, judge);
}

int cp2i::repair_check_with(cp2_ctx* ctx, size_t cell_size, size_t block_size, const uint8_t* data, size_t n, uint32_t* status,
                            const RepairJudge& judge) {
  if (n == 0) return CP2_OK;
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const size_t cpb = block_size / cell_size;
  const std::vector<size_t> sizes = layer_sizes_of(cpb);
  size_t below_root = 0, per_block = 0;              // nodes of one block tree under its root layer, and in all
  for (size_t j = 0; j < sizes.size(); ++j) {
    per_block += sizes[j];
    if (j + 1 < sizes.size()) below_root += sizes[j];
  }
  // requests per chunk: half the context's staging in candidate bytes (the node buffer of a chunk holds about as much again)
  const size_t chunk = std::max<size_t>(1, std::min<size_t>(n, (ctx->stage_bytes / 2) / block_size));
  const bool pinned = !judge.cells && (judge.host ? judge.host_pinned : host_array_pinned(data, n * block_size, PIECE_BYTES));
  DevBuf d_verdict, d_nodes, d_cells;                // (device buffers go after every stream has drained: DevBuf::release)
  if (judge.begin) CP2_TRY(judge.begin(chunk));
  CP2_TRY(d_verdict.scratch(ctx, n * 4));
  CP2_TRY(d_nodes.scratch(ctx, chunk * per_block * 32));
  const size_t last = n - (n - 1) / chunk * chunk;   // requests of the last chunk
  if (judge.cells || pinned || chunk * block_size <= SMALL_BYTES || last * block_size <= SMALL_BYTES) CP2_TRY(d_cells.scratch(ctx, chunk * block_size));
  hipStream_t aux = nullptr, copy = nullptr;
  hipEvent_t ready = nullptr, up = nullptr, aux_done = nullptr;
  struct Guard {
    hipStream_t* copy; hipEvent_t* ev[3];
    ~Guard() {
      if (*copy) { (void)hipStreamSynchronize(*copy); (void)hipStreamDestroy(*copy); }
      for (auto e : ev) if (*e) (void)hipEventDestroy(*e);
    }
  } guard{&copy, {&ready, &up, &aux_done}};
  if (pinned) {
    CP2_TRY(aux_stream(ctx, &aux, 1));
    CP2_HIP(ctx, hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
    CP2_HIP(ctx, hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    CP2_HIP(ctx, hipEventCreateWithFlags(&up, hipEventDisableTiming));
    CP2_HIP(ctx, hipEventCreateWithFlags(&aux_done, hipEventDisableTiming));
  }
  const size_t piece = std::max<size_t>(1, PIECE_BYTES / block_size) * block_size;
  for (size_t c0 = 0; c0 < n; c0 += chunk) {
    const size_t m = std::min(chunk, n - c0), bytes = m * block_size;
    const uint8_t* src = data && !judge.host ? data + c0 * block_size : nullptr;
    if (judge.host && !judge.cells) CP2_TRY(judge.host(c0, m, &src));
    if (pinned) {
      // the copy engine reads the caller's memory in place, piece by piece; each piece is hashed as soon as it has landed, the pieces
      // alternating between the context's two hashing streams.  Nothing of this chunk starts before the previous one is compared.
      CP2_HIP(ctx, hipEventRecord(ready, ctx->stream));
      CP2_HIP(ctx, hipStreamWaitEvent(copy, ready, 0));
      CP2_HIP(ctx, hipStreamWaitEvent(aux, ready, 0));
      size_t j = 0;
      for (size_t at = 0; at < bytes; at += piece, ++j) {
        const size_t len = std::min(piece, bytes - at);
        hipStream_t hs = (j & 1) ? aux : ctx->stream;
        CP2_HIP(ctx, hipMemcpyAsync(d_cells.u8() + at, src + at, len, hipMemcpyHostToDevice, copy));
        CP2_HIP(ctx, hipEventRecord(up, copy));
        CP2_HIP(ctx, hipStreamWaitEvent(hs, up, 0));
        CP2_HIP(ctx, cp2k::launch_hash_cells(d_cells.u8() + at, cell_size, len / cell_size, d_nodes.u8() + at / cell_size * 32, hs));
      }
      CP2_HIP(ctx, hipEventRecord(aux_done, aux));
      CP2_HIP(ctx, hipStreamWaitEvent(ctx->stream, aux_done, 0));
    } else if (!judge.cells && bytes > SMALL_BYTES) {
      // large pageable chunks: the pinned ingestion ring, uploads and hashing overlapped (cp2_hash_cells' path); the ring writes the
      // leaves from both hashing streams, so the previous chunk's reads of the node buffer are waited for first
      if (c0) CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
      CP2_TRY(hash_host_cells_pipelined(ctx, src, cell_size, m * cpb, d_nodes.u8()));
    } else {                                         // one upload, or the caller's device-side source in its place
      if (judge.cells) CP2_TRY(judge.cells(c0, m, d_cells.u8(), ctx->stream));
      else CP2_HIP(ctx, hipMemcpyAsync(d_cells.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, cp2k::launch_hash_cells(d_cells.p, cell_size, m * cpb, d_nodes.p, ctx->stream));
    }
    // what the verdicts of this chunk read beside its roots, queued behind the hashing; the block trees of the chunk (segment = block,
    // layer-major); then the verdicts of its requests from the root layer
    if (judge.stage) CP2_TRY(judge.stage(c0, m, ctx->stream));
    CP2_TRY(merkle_trees_dev(ctx, d_nodes.p, cpb, m, d_nodes.p, true));
    CP2_TRY(judge.verdicts(d_nodes.u8() + below_root * m * 32, c0, m, static_cast<uint32_t*>(d_verdict.p) + c0, ctx->stream));
  }
  std::vector<uint32_t> v(n);
  CP2_HIP(ctx, hipMemcpyAsync(v.data(), d_verdict.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "repair: the check failed on the device";
    return CP2_ERR_HIP;
  }
  for (size_t i = 0; i < n; ++i) status[i] = v[i] == 0 ? CP2_REPAIR_MATCH : CP2_REPAIR_MISMATCH;
  return CP2_OK;
}

int cp2i::repair_write(const std::string& base, size_t block_size, const uint64_t* slot_block, const uint8_t* data, size_t n, uint32_t* status,
                       size_t* n_written, std::vector<FileStamp>* written, std::string* err) {
  return repair_write_rows(base, block_size, slot_block, data, nullptr, n, status, n_written, written, err);
}

int cp2i::repair_write_rows(const std::string& base, size_t block_size, const uint64_t* slot_block, const uint8_t* data, const size_t* row, size_t n,
                            uint32_t* status, size_t* n_written, std::vector<FileStamp>* written, std::string* err) {
  std::vector<size_t> matched;
  for (size_t i = 0; i < n; ++i)
    if (status[i] == CP2_REPAIR_MATCH) matched.push_back(i);
  const std::vector<WriteGroup> groups = repair_write_groups(slot_block, matched);
  // every file's stat before the first write: the cache stamps follow only writes to files the cache still described
  std::vector<FileStamp> stamps(groups.size());
  for (size_t g = 0; g < groups.size(); ++g) {
    stamps[g].slot = groups[g].slot;
    (void)repair_stat_stamp(slot_file_name(base, groups[g].slot), stamps[g].before);
  }
  for (size_t g = 0; g < groups.size(); ++g) {
    const std::string name = slot_file_name(base, groups[g].slot);
    const int what = repair_write_file(name, block_size, groups[g].reqs.size(), [&](size_t k) { return slot_block[2 * groups[g].reqs[k] + 1] * (uint64_t)block_size; },
                                       [&](size_t k) { const size_t i = groups[g].reqs[k]; return data + (row ? row[i] : i) * block_size; });
    if (what) {
      *err = "cannot write " + name + ": " + repair_write_reason(what);
      for (size_t h = g; h < groups.size(); ++h)
        for (size_t i : groups[h].reqs) status[i] = CP2_REPAIR_UNWRITTEN;
      return CP2_ERR_IO;
    }
    (void)repair_stat_stamp(name, stamps[g].after);
    written->push_back(stamps[g]);
    *n_written += groups[g].reqs.size();
  }
  return CP2_OK;
}

int cp2i::repair_restamp_caches(const std::vector<std::string>& paths, const cp2_config& cfg, uint64_t n_items, size_t n_cells, uint64_t first_item,
                                uint64_t units_per_slot, const std::string& base, const std::vector<FileStamp>& written, size_t* restamped,
                                std::string* err) {
  CacheHead want;                                       // the items a cache must describe for its stamps to follow the writes
  want.n_items = n_items; want.cell_size = cfg.cell_size; want.block_size = cfg.block_size; want.n_cells = n_cells;
  want.src = (uint64_t)CellSrc::File; want.first_item = first_item; want.units_per_slot = units_per_slot; want.base = base;
  for (const std::string& p : paths) {
    size_t r = 0;
    CP2_TRY(cache_restamp(p.c_str(), want, written, &r, err));
    *restamped += r;
  }
  return CP2_OK;
}

int cp2i::repair_refuse(const cp2_config& cfg, bool from_file, int tree_mode, const uint64_t* slot_block, const uint8_t* data, size_t n, int flags,
                        const uint32_t* status, uint64_t first_slot, uint64_t n_local, std::string* err) {
  if (n && (!slot_block || !data || !status)) {
    *err = "repair: slot_block, data and status must not be NULL when n > 0";
    return CP2_ERR_INVALID;
  }
  if (flags & ~CP2_REPAIR_CHECK_ONLY) {
    *err = "repair: unknown flag bits 0x" + [](int f) { char b[16]; std::snprintf(b, sizeof b, "%x", (unsigned)f); return std::string(b); }(flags & ~CP2_REPAIR_CHECK_ONLY);
    return CP2_ERR_INVALID;
  }
  if (tree_mode == 0) {
    *err = "repair: this dataset keeps only its slot roots, no block roots to check a block against: write the slot whole, then rebuild or scrub it";
    return CP2_ERR_INVALID;
  }
  if (!from_file && !(flags & CP2_REPAIR_CHECK_ONLY)) {
    *err = "repair: this dataset's cells come from the fake source and it has no slot files to write: only CP2_REPAIR_CHECK_ONLY is accepted";
    return CP2_ERR_INVALID;
  }
  const uint64_t n_blocks = cfg.n_cells / (cfg.block_size / cfg.cell_size);
  return repair_validate(slot_block, n, first_slot, n_local, n_blocks, err) ? CP2_OK : CP2_ERR_INVALID;
}

void cp2i::repair_trace(const char* what, size_t n, const uint32_t* status, size_t n_written, size_t block_size, double seconds, size_t restamped,
                        bool cache) {
  if (!std::getenv("CP2_TRACE")) return;
  size_t matched = 0;
  for (size_t i = 0; i < n; ++i) matched += status[i] != CP2_REPAIR_MISMATCH;
  const double bytes = (double)n * (double)block_size;
  std::fprintf(stderr, "[cp2 trace] %s: %zu request(s), %zu matched, %zu written, %.0f bytes, %.3f s (%.2f GB/s), cache %s\n", what, n, matched,
               n_written, bytes, seconds, seconds > 0 ? bytes / seconds / 1e9 : 0.0,
               !cache ? "not given" : (restamped ? (std::to_string(restamped) + " stamp(s) restamped").c_str() : "not restamped"));
}

int cp2i::repair_dataset_mode(const cp2_dataset* ds) { return ds->trees ? 1 : ds->tree_mode; }

RepairKept cp2i::repair_dataset_kept(const cp2_dataset* ds) {
  RepairKept k;
  const DevBuf& b = ds->trees ? ds->trees->nodes : ds->compact;
  k.nodes = b.u8();
  k.rows = b.bytes / 32;
  return k;
}

uint64_t cp2i::repair_dataset_row(const cp2_dataset* ds, uint64_t slot, uint64_t block) {
  const uint64_t local = slot - ds->first_slot;
  if (const cp2_slot_trees* t = ds->trees) return repair_row_full(t->boff.back(), t->bsizes.back(), t->nblocks, local, block);
  return repair_row_compact(ds->coff[0], ds->csizes[0], local, block);
}

extern "C" int cp2_dataset_repair_blocks(cp2_dataset* ds, const uint64_t* slot_block, const uint8_t* data, size_t n, int flags, const char* cache_path,
                                         uint32_t* status, size_t* n_written) try {
  if (!ds) return CP2_ERR_INVALID;
  cp2_ctx* ctx = ds->ctx;
  std::string err;
  if (repair_refuse(ds->cfg, ds->from_file, repair_dataset_mode(ds), slot_block, data, n, flags, status, ds->first_slot, ds->n_local, &err) != CP2_OK) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n == 0) {
    if (n_written) *n_written = 0;
    return CP2_OK;
  }
  CP2_REFUSE_STUCK(ctx);
  const auto t0 = std::chrono::steady_clock::now();
  const cp2_config& c = ds->cfg;
  const RepairKept k = repair_dataset_kept(ds);           // the kept block root of every request: a row of the dataset's node buffer
  std::vector<uint64_t> rows(n);
  for (size_t i = 0; i < n; ++i) rows[i] = repair_dataset_row(ds, slot_block[2 * i], slot_block[2 * i + 1]);
  std::vector<uint32_t> st(n);
  CP2_TRY(repair_check(ctx, k, c.cell_size, c.block_size, data, rows.data(), n, st.data()));
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
  repair_trace("repair", n, status, written_n, c.block_size, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), restamped,
               cache_path != nullptr);
  return r;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
