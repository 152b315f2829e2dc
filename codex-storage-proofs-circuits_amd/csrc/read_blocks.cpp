// Listed blocks read back verified, with their proofs, behind the C ABI: cp2_datasets_read_blocks and cp2_dataset_read_blocks
// (include/codex_p2.h).
//
// A node that answers a peer, or spot-checks what it stores, names blocks of the slots it holds: (dataset, slot, block).  Each block is
// read from its slot file into the row of its request (the caller's `data`, or a pooled pinned chunk buffer when the call only checks),
// uploaded from there, hashed and reduced to its block root on repair's data path (repair_check_with, repair.cpp) and compared with the
// block root the dataset keeps for it by k_repair_compare_addr -- one absolute address per request, so the requests of many datasets
// share every launch.  The kept roots and the paths above them do not depend on what was read: one k_gather_addr and one download per
// call fetch them all.  What the plan decides -- refusals, read order, chunks, packed path offsets, the address tables -- is
// read_blocks_plan.hpp.  Chunk k + 1 is read on the context's ingestion threads while chunk k is uploaded and hashed.
//
// Where the time goes on the device: 1119 permutations per block in k_hash_cells and the block-tree layers, as in every other pass over
// block bytes.  The compare and the gather are what this file adds there, a few bytes per block.
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
#include "read_blocks_plan.hpp"
#include "repair.hpp"

using namespace cp2i;

static_assert(READ_BLOCKS_CHECK_ONLY == CP2_READ_CHECK_ONLY, "the plan's flag is the boundary's");
static_assert(CP2_READ_OK == CP2_REPAIR_MATCH && CP2_READ_DAMAGED == CP2_REPAIR_MISMATCH, "repair_check_with's verdicts are the statuses");

namespace {

// Where the blocks of a pass come from.  read: the file-sourced requests of chunk k, each into row_of(i), on host threads (false: *err
// is the message, CP2_ERR_IO).  fake (may be empty: none): per request, whether the device regenerates it from seeds[i] (cp2_slot_seed)
// and firsts[i] (its first cell).  A later source over a fill session's present blocks is another `read` and nothing else.
struct BlockSource {
  size_t n_chunks = 0;
  std::function<bool(size_t k, const std::function<uint8_t*(size_t)>& row_of, std::string* err)> read;
  std::vector<uint8_t> fake;
  std::vector<uint64_t> seeds, firsts;
};

// The middle of the pass: n requests in chunks of `chunk`, request i judged against the 32 bytes at addr[i]; addr (n + path rows
// entries, read_blocks_addr_table) gathered whole into `gathered` (host, addr.size() x 32 bytes).  data (n x block_size, may be NULL):
// every row is filled; nothing is zeroed here.  *touched: the requests whose rows may hold file bytes when the pass fails.
int read_pass(cp2_ctx* ctx, size_t cell_size, size_t block_size, size_t n, size_t chunk, const std::vector<uint64_t>& addr, BlockSource& src,
              uint8_t* data, uint8_t* gathered, uint32_t* status, size_t* touched) {
  const size_t cpb = block_size / cell_size;
  const bool any_fake = !src.fake.empty();
  PinBuf ring[2];                                    // check only: two chunk buffers, whatever n is
  if (!data)
    for (auto& b : ring) CP2_TRY(b.alloc(ctx, std::min(n, chunk) * block_size));
  DevBuf d_addr, d_gen;                              // (go after the streams have drained: DevBuf::release)
  std::string read_err[2];
  bool read_ok[2] = {true, true};
  auto base_of = [&](size_t k) { return data ? data + k * chunk * block_size : ring[k & 1].u8(); };
  {
    Workers reader(1);                               // one chunk ahead; the chunk's files are spread over the ingestion threads inside
    auto start = [&](size_t k) {
      if (k >= src.n_chunks) return;
      *touched = std::min(n, (k + 1) * chunk);
      uint8_t* base = base_of(k);
      const size_t c0 = k * chunk;
      reader.submit([&, k, base, c0] {
        read_ok[k & 1] = src.read(k, [&](size_t i) { return base + (i - c0) * block_size; }, &read_err[k & 1]);
      });
    };
    // chunk k's rows, read; chunk k + 1 started.  A ring buffer is read into again only after the chunk that was uploaded from it is done.
    auto take = [&](size_t c0, const uint8_t** out) -> int {
      const size_t k = c0 / chunk;
      reader.wait_idle();
      if (!read_ok[k & 1]) {
        ctx->err = read_err[k & 1];
        return CP2_ERR_IO;
      }
      if (!data && k > 0) CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
      start(k + 1);
      *out = base_of(k);
      return CP2_OK;
    };
    RepairJudge judge;
    judge.begin = [&](size_t) -> int {
      CP2_TRY(d_addr.scratch(ctx, n * 8));
      CP2_HIP(ctx, hipMemcpyAsync(d_addr.p, addr.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
      if (any_fake) {
        CP2_TRY(d_gen.scratch(ctx, n * 16));
        CP2_HIP(ctx, hipMemcpyAsync(d_gen.p, src.seeds.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
        CP2_HIP(ctx, hipMemcpyAsync(d_gen.u8() + n * 8, src.firsts.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
      }
      start(0);
      return CP2_OK;
    };
    judge.host = [&](size_t c0, size_t, const uint8_t** out) -> int { return take(c0, out); };
    judge.host_pinned = data ? host_array_pinned(data, n * block_size, (size_t)128 << 20) : true;
    if (any_fake) {
      // a chunk with regenerated blocks is put together on the device: runs of file rows uploaded, runs of fake rows generated in place
      // (and downloaded into the caller's rows), all on the stream the chunk is hashed on
      judge.cells = [&](size_t c0, size_t m, uint8_t* d_cells, hipStream_t st) -> int {
        const uint8_t* rows = nullptr;
        CP2_TRY(take(c0, &rows));
        const uint64_t* seeds = static_cast<const uint64_t*>(d_gen.p);
        for (size_t a = 0; a < m;) {
          size_t b = a + 1;
          while (b < m && src.fake[c0 + b] == src.fake[c0 + a]) ++b;
          const size_t off = a * block_size, len = (b - a) * block_size;
          if (src.fake[c0 + a]) {
            CP2_HIP(ctx, cp2k::launch_gen_fake_cells_many(seeds + c0 + a, seeds + n + c0 + a, cpb, (b - a) * cpb, cell_size, d_cells + off, st));
            if (data) CP2_HIP(ctx, hipMemcpyAsync(data + (c0 + a) * block_size, d_cells + off, len, hipMemcpyDeviceToHost, st));
          } else {
            CP2_HIP(ctx, hipMemcpyAsync(d_cells + off, rows + off, len, hipMemcpyHostToDevice, st));
          }
          a = b;
        }
        return CP2_OK;
      };
    }
    judge.verdicts = [&](const uint8_t* fresh, size_t c0, size_t m, uint32_t* verdict, hipStream_t st) -> int {
      CP2_HIP(ctx, cp2k::launch_repair_compare_addr(fresh, static_cast<const uint64_t*>(d_addr.p) + c0, m, verdict, st));
      return CP2_OK;
    };
    const int r = repair_check_with(ctx, cell_size, block_size, nullptr, n, status, judge);
    reader.wait_idle();                              // (a chunk read ahead of a pass that failed writes into rows of this scope)
    if (r != CP2_OK) {
      (void)hipStreamSynchronize(ctx->stream);       // nothing of the pass reads a ring buffer or writes a caller's row after this
      return r;
    }
  }
  return gather_rows_by_addr(ctx, addr, gathered);
}

ReadDataset describe(const cp2_ctx* ctx, cp2_dataset* const* ds, size_t k) {
  ReadDataset d;
  const cp2_dataset* p = ds[k];
  d.same_as = k;
  if (!p) { d.null = true; return d; }
  for (size_t j = 0; j < k; ++j)
    if (ds[j] == p) { d.same_as = j; break; }
  d.foreign = p->ctx != ctx;
  d.cell_size = p->cfg.cell_size;
  d.block_size = p->cfg.block_size;
  d.n_cells = p->cfg.n_cells;
  d.first_slot = p->first_slot;
  d.n_local = p->n_local;
  d.mode = repair_dataset_mode(p);
  d.from_file = p->from_file;
  d.base = p->file_base;
  d.seed = p->cfg.seed;
  if (d.mode == 0 || d.foreign) return d;
  d.nodes = (uint64_t)reinterpret_cast<uintptr_t>(repair_dataset_kept(p).nodes);
  if (const cp2_slot_trees* t = p->trees) {
    d.whole = t->units_per_slot == 1;
    d.root_off = t->boff.back();
    d.root_size = t->bsizes.back();
    d.offs.assign(t->toff.begin(), t->toff.end());
    d.sizes.assign(t->tsizes.begin(), t->tsizes.end());
  } else {
    d.whole = true;
    d.root_off = p->coff.empty() ? 0 : p->coff[0];
    d.root_size = p->csizes.empty() ? 0 : p->csizes[0];
    d.offs.assign(p->coff.begin(), p->coff.end());
    d.sizes.assign(p->csizes.begin(), p->csizes.end());
  }
  return d;
}

// the one implementation: outputs are written only when the whole call succeeded (data excepted: its rows are read into in place, and
// hold zeros wherever the call had written when it fails)
int read_blocks(cp2_ctx* ctx, cp2_dataset* const* ds, size_t n_ds, const uint64_t* req, size_t n, int flags, uint8_t* data, uint8_t* block_roots,
                uint8_t* paths, uint64_t* path_off, bool packed, uint32_t* status, size_t* n_ok) {
  ReadArgs a;
  a.ds = ds != nullptr; a.req = req != nullptr; a.data = data != nullptr; a.status = status != nullptr;
  a.paths = paths != nullptr;
  a.path_off = packed ? path_off != nullptr : a.paths;   // (the single form's layout needs no offsets)
  a.n_ds = n_ds; a.n = n; a.flags = flags;
  std::vector<ReadDataset> sets;
  if (ds && n)
    for (size_t k = 0; k < n_ds; ++k) sets.push_back(describe(ctx, ds, k));
  std::string err;
  if (!read_blocks_validate(a, sets, req, &err)) {
    ctx->err = err;
    return CP2_ERR_INVALID;
  }
  if (n == 0) {
    if (n_ok) *n_ok = 0;
    return CP2_OK;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  const size_t cs = sets[0].cell_size, bs = sets[0].block_size;
  const size_t chunk = read_blocks_chunk(ctx->stage_bytes, bs, n);
  const ReadPlan plan = read_blocks_plan(sets, req, n, chunk);
  const std::vector<uint64_t> off = read_blocks_path_off(sets, req, n);
  const std::vector<uint64_t> addr = read_blocks_addr_table(sets, req, n, off);
  BlockSource src;
  src.n_chunks = plan.n_chunks();
  const int threads = fill_threads(ctx);
  src.read = [&](size_t k, const std::function<uint8_t*(size_t)>& row_of, std::string* e) {
    std::string bad;
    int eno = 0;
    if (read_blocks_read_chunk(plan, k, sets, req, bs, row_of, threads, &bad, &eno)) return true;
    *e = slot_file_error(bad, eno);
    return false;
  };
  bool any_fake = false;
  for (size_t i = 0; i < n; ++i) any_fake |= !sets[req[3 * i]].from_file;
  if (any_fake) {
    src.fake.resize(n);
    src.seeds.assign(n, 0);
    src.firsts.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
      const ReadDataset& d = sets[req[3 * i]];
      src.fake[i] = d.from_file ? 0 : 1;
      if (d.from_file) continue;
      src.seeds[i] = cp2_slot_seed(d.seed, req[3 * i + 1]);
      src.firsts[i] = req[3 * i + 2] * (bs / cs);
    }
  }
  std::vector<uint32_t> st(n);
  std::vector<uint8_t> gathered(addr.size() * 32);
  size_t touched = 0;
  const int r = read_pass(ctx, cs, bs, n, chunk, addr, src, data, gathered.data(), st.data(), &touched);
  if (r != CP2_OK) {
    if (data) std::memset(data, 0, touched * bs);
    return r;
  }
  size_t ok = 0;
  for (size_t i = 0; i < n; ++i) {
    status[i] = st[i];
    if (st[i] == CP2_READ_OK) ++ok;
    else if (data) std::memset(data + i * bs, 0, bs);   // no byte that failed its check is left in an output
  }
  if (block_roots) std::memcpy(block_roots, gathered.data(), n * 32);
  if (paths) std::memcpy(paths, gathered.data() + n * 32, (size_t)off[n] * 32);
  if (packed && path_off) std::copy(off.begin(), off.end(), path_off);
  if (n_ok) *n_ok = ok;
  if (std::getenv("CP2_TRACE")) {
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), bytes = (double)n * (double)bs;
    std::fprintf(stderr, "[cp2 trace] read blocks: %zu dataset(s), %zu request(s), %zu chunk(s), %.0f bytes, %.3f s (%.2f GB/s), %zu damaged\n", n_ds, n,
                 plan.n_chunks(), bytes, s, s > 0 ? bytes / s / 1e9 : 0.0, n - ok);
  }
  return CP2_OK;
}

}  // namespace

extern "C" int cp2_datasets_read_blocks(cp2_ctx* ctx, cp2_dataset* const* ds, size_t n_ds, const uint64_t* req, size_t n, int flags, uint8_t* data,
                                        uint8_t* block_roots, uint8_t* paths, uint64_t* path_off, uint32_t* status, size_t* n_ok) try {
  if (!ctx) return CP2_ERR_INVALID;
  return read_blocks(ctx, ds, n_ds, req, n, flags, data, block_roots, paths, path_off, true, status, n_ok);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_dataset_read_blocks(cp2_dataset* ds, const uint64_t* slot_block, size_t n, int flags, uint8_t* data, uint8_t* block_roots,
                                       uint8_t* paths, uint32_t* status, size_t* n_ok) try {
  if (!ds) return CP2_ERR_INVALID;
  // the many-dataset pass with one dataset, on the dataset's own context; one depth, so the packed paths ARE cp2_dataset_block_proofs' layout
  std::vector<uint64_t> req;
  if (slot_block) {
    req.resize(3 * n);
    for (size_t i = 0; i < n; ++i) {
      req[3 * i] = 0;
      req[3 * i + 1] = slot_block[2 * i];
      req[3 * i + 2] = slot_block[2 * i + 1];
    }
  }
  cp2_dataset* const one[1] = {ds};
  return read_blocks(ds->ctx, one, 1, slot_block ? req.data() : nullptr, n, flags, data, block_roots, paths, nullptr, false, status, n_ok);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
