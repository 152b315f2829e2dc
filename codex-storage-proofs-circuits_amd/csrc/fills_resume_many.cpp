// cp2_fills_resume_many behind the C ABI (include/codex_p2.h): many fill sessions of one context resumed from their checkpoints in one pass.
//
// After a restart a node brings every session back through cp2_fill_resume (fill.cpp): per session a checkpoint read, two allocations,
// two uploads with a drain each, and a re-check with its own data-path set-up that reads block by block on one thread into a pageable
// buffer, reading and hashing in turns.  Nothing of that is session-wide but the buffers the session owns.  Here the checkpoints are read
// and parsed on the context's ingestion threads, every check of every entry runs before a session exists, all sessions are opened and
// their roots and surviving layer-0 rows go up through one pinned staging buffer -- one copy, one scatter launch, one drain --, and the
// re-check is ONE pass of read_pass.hpp -- the chunked reader of cp2_datasets_read_blocks: each file opened once per chunk, the files
// spread over the ingestion threads, two pooled pinned buffers one chunk ahead of the hashing -- over every present block of every
// session, judged by k_block_root_recheck_addr through one absolute address per block.  What the call means is defined by the call that
// exists: per entry, cp2_fill_resume; fills_resume_plan.hpp holds the host side -- the order and words of the checks, the request list,
// the owners, the address table, the verdict index turned back into (entry, block).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "fill_checkpoint.hpp"
#include "fill_session.hpp"
#include "fills_resume_plan.hpp"
#include "kernels.hpp"
#include "read_pass.hpp"
#include "workers.hpp"

using namespace cp2i;

static_assert(FILLS_RESUME_TRUST_FILES == CP2_RESUME_TRUST_FILES, "the plan's flag is the boundary's");
static_assert(FILLS_RESUME_INVALID == CP2_ERR_INVALID && FILLS_RESUME_IO == CP2_ERR_IO, "the plan's statuses are the boundary's");

namespace {

double seconds_since(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); }

struct Entry {
  const cp2_config* cfg = nullptr;
  uint64_t first_slot = 0, n_local = 0;
  const uint8_t* slot_roots = nullptr;
  const char* path = nullptr;
};

// Everything after the argument checks.  The sessions it opens stay in `f` whatever it returns: the caller frees them behind a drained
// stream when the call fails.
int resume_many(cp2_ctx* ctx, const std::vector<Entry>& e, int flags, std::vector<std::unique_ptr<cp2_fill_session>>& f, std::vector<uint64_t>& n_dropped) {
  const size_t n = e.size();
  const bool recheck = !(flags & CP2_RESUME_TRUST_FILES);
  const int threads = fill_threads(ctx);
  const auto t0 = std::chrono::steady_clock::now();
  ResumeManyRefusal why;

  // ---- the checkpoints: intact, then a description of exactly the entry's session; on the ingestion threads, the lowest index reported ----
  std::vector<FillCheckpoint> ck(n);
  std::vector<ResumeManyFound> found(n);
  on_threads(threads, n, [&](int, size_t k) {
    const int st = fill_read_checkpoint(&found[k].text, e[k].path, &ck[k]);
    if (st != CP2_OK) {
      found[k].status = st;
      return true;
    }
    const cp2_config& c = *e[k].cfg;
    FillCkptMeta want;
    want.cell_size = c.cell_size; want.block_size = c.block_size; want.n_cells = c.n_cells; want.n_slots = c.n_slots;
    want.first_slot = e[k].first_slot; want.n_local = e[k].n_local;
    want.src = c.file_base ? FILL_SRC_FILE : FILL_SRC_FAKE;
    want.seed = c.seed;
    if (c.file_base) want.file_base = c.file_base;
    want.roots.resize(e[k].n_local * 32);
    for (uint64_t s = 0; s < e[k].n_local; ++s) canonical_felt(e[k].slot_roots + s * 32, &want.roots[s * 32]);
    found[k] = fills_resume_describes(ck[k].meta, want, e[k].path);
    return true;
  });
  if (fills_resume_first_failed(found, &why)) {
    ctx->err = why.text;
    return why.status;
  }
  uint64_t present = 0;
  for (const FillCheckpoint& c : ck)
    for (uint64_t w : c.bits) present += (uint64_t)__builtin_popcountll(w);

  // ---- what the slot files can no longer back: dropped without a read; absence is a state, a stat that fails is an error ------------------
  std::vector<std::vector<uint64_t>> dropped(n);
  if (recheck) {
    on_threads(threads, n, [&](int, size_t k) {
      if (!e[k].cfg->file_base) return true;
      std::vector<uint64_t> whole;
      std::string bad;
      if (!fill_slot_files_cover(e[k].cfg->file_base, e[k].first_slot, e[k].n_local, e[k].cfg->block_size, &whole, &bad)) {
        found[k] = {CP2_ERR_IO, slot_file_error(bad, 0)};
        return true;
      }
      fill_ckpt_drop_short(whole, ck[k].meta.n_blocks(), &ck[k].bits, &ck[k].layer0, &dropped[k]);
      return true;
    });
    if (fills_resume_first_failed(found, &why)) {
      ctx->err = why.text;
      return why.status;
    }
  }
  const double s_ckpt = seconds_since(t0);

  // ---- every session, as cp2_fill_begin makes it; roots and layer 0 through pinned staging, one drain --------------------------------------
  const auto t1 = std::chrono::steady_clock::now();
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<size_t> sizes(2 * n);
  size_t up_bytes = 0;
  for (size_t k = 0; k < n; ++k) {
    const int st = fill_session_alloc(ctx, e[k].cfg, e[k].first_slot, e[k].n_local, e[k].slot_roots, &f[k]);
    if (st == CP2_OK && !f[k]->plan.restore(ck[k].bits)) {
      ctx->err = fills_resume_entry(k) + "fill: checkpoint " + std::string(e[k].path) + " is corrupt: its bitmap is not one of this session";
      return CP2_ERR_IO;
    }
    if (st != CP2_OK) {
      ctx->err = fills_resume_entry(k) + ctx->err;
      return st;
    }
    sizes[2 * k] = f[k]->roots.size();
    sizes[2 * k + 1] = ck[k].layer0.size();
    up_bytes += sizes[2 * k] + sizes[2 * k + 1];
  }
  {
    // Roots and layer 0 of every session are 32-byte rows: they are packed into one pinned staging buffer with one destination address
    // per row behind them, go up as one copy per piece and are written to where each session keeps them by k_scatter_rows_addr (items of
    // one row), so that N sessions cost one upload and one launch, not 2 N copies.  A piece is drained before the buffer is packed again
    // or handed back: one drain in all unless the sessions' rows exceed the staging size (the last cut always flushes).
    const size_t piece = std::max<size_t>(32, std::min(up_bytes, ctx->stage_bytes) / 32 * 32);
    PinBuf stage;
    DevBuf d_stage;                                      // (goes after the stream has drained: DevBuf::release)
    CP2_TRY(stage.alloc(ctx, piece + piece / 4));
    CP2_TRY(d_stage.scratch(ctx, piece + piece / 4));
    uint64_t* tab = reinterpret_cast<uint64_t*>(stage.u8() + piece);
    for (const ResumeManyCut& c : fills_resume_cuts(sizes, piece)) {
      const size_t k = c.seg / 2;
      const bool roots = c.seg % 2 == 0;
      const uint8_t* src = (roots ? f[k]->roots.data() : ck[k].layer0.data()) + c.off;
      const uint64_t dst = (uint64_t)reinterpret_cast<uintptr_t>(roots ? f[k]->slot_roots.p : f[k]->compact.p) + c.off;
      std::memcpy(stage.u8() + c.at, src, c.len);
      for (size_t r = 0; r < c.len / 32; ++r) tab[c.at / 32 + r] = dst + r * 32;
      if (!c.flush) continue;
      const size_t rows = (c.at + c.len) / 32;
      CP2_HIP(ctx, hipMemcpyAsync(d_stage.p, stage.p, rows * 32, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, hipMemcpyAsync(d_stage.u8() + piece, tab, rows * 8, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, cp2k::launch_scatter_rows_addr(d_stage.p, 1, reinterpret_cast<const uint64_t*>(d_stage.u8() + piece), 1, rows, ctx->stream));
      CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  const double s_open = seconds_since(t1);

  // ---- the re-check: one pass over every present block of every session ----------------------------------------------------------------------
  const auto t2 = std::chrono::steady_clock::now();
  FillsResumePlan plan;
  size_t n_chunks = 0;
  double bytes = 0;
  std::vector<uint32_t> verdict;
  if (recheck) {
    const size_t cs = e[0].cfg->cell_size, bs = e[0].cfg->block_size;
    std::vector<ResumeManySession> s(n);
    for (size_t k = 0; k < n; ++k) {
      const FillPlan& p = f[k]->plan;                   // (coff[0] == 0: a global index is its row of the compact buffer)
      s[k].bits = p.bits;
      s[k].n_blocks = p.n_blocks; s[k].first_slot = p.first_slot; s[k].n_local = p.n_local;
      s[k].from_file = f[k]->from_file;
      s[k].base = f[k]->file_base;
      s[k].seed = f[k]->cfg.seed;
      s[k].layer0 = (uint64_t)reinterpret_cast<uintptr_t>(f[k]->compact.p) + (uint64_t)p.coff[0] * 32;
    }
    plan.build(s, cs, bs, [](uint64_t seed, uint64_t slot) { return cp2_slot_seed(seed, slot); });
    const size_t m = plan.n();
    bytes = (double)m * (double)bs;
    if (m > 0) {
      const size_t chunk = read_blocks_chunk(ctx->stage_bytes, bs, m);
      const ReadPlan rp = plan.read_plan(chunk);
      n_chunks = rp.n_chunks();
      BlockSource src;
      src.n_chunks = n_chunks;
      src.read = [&](size_t k, const std::function<uint8_t*(size_t)>& row_of, std::string* err) {
        std::string bad;
        int eno = 0;
        if (plan.read_chunk(rp, k, row_of, threads, &bad, &eno)) return true;
        *err = slot_file_error(bad, eno);                // a read error is an error, never a dropped block
        return false;
      };
      src.fake = plan.fake;
      src.seeds = plan.seeds;
      src.firsts = plan.firsts;
      verdict.assign(m, 0);
      const ReadJudge judge = [&](const uint8_t* fresh, const uint64_t* d_addr, size_t cnt, uint32_t* v, hipStream_t st) {
        return cp2k::launch_block_root_recheck_addr(fresh, d_addr, cnt, v, st);
      };
      size_t touched = 0;
      CP2_TRY(read_pass(ctx, cs, bs, m, chunk, plan.addr, src, judge, nullptr, nullptr, verdict.data(), &touched));
    }
  }
  const double s_check = seconds_since(t2);

  // ---- the host's half of a drop: the presence bits, per session ----------------------------------------------------------------------------
  const auto t3 = std::chrono::steady_clock::now();
  uint64_t all_dropped = 0;
  if (recheck && plan.n() > 0) {
    const std::vector<std::vector<uint64_t>> changed = plan.drops(verdict.data());
    for (size_t k = 0; k < n; ++k) {
      (void)f[k]->plan.drop(changed[k].data(), changed[k].size());
      dropped[k].insert(dropped[k].end(), changed[k].begin(), changed[k].end());
    }
  }
  for (size_t k = 0; k < n; ++k) {
    n_dropped[k] = dropped[k].size();
    all_dropped += n_dropped[k];
  }
  if (std::getenv("CP2_TRACE")) {
    const double s = seconds_since(t0);
    std::fprintf(stderr, "[cp2 trace] fills resume many: %zu session(s), %llu block(s) present in the checkpoints, %zu re-read, %llu dropped, %zu chunk(s), "
                 "%.0f bytes, %.3f s (%.2f GB/s; %.3f checkpoints, %.3f opens and uploads, %.3f re-check, %.3f host drops)\n", n,
                 (unsigned long long)present, plan.n(), (unsigned long long)all_dropped, n_chunks, bytes, s, s > 0 ? bytes / s / 1e9 : 0.0, s_ckpt,
                 s_open, s_check, seconds_since(t3));
  }
  return CP2_OK;
}

}  // namespace

extern "C" int cp2_fills_resume_many(cp2_ctx* ctx, const void* const* cfgs_in, const uint64_t* ranges, const uint8_t* const* slot_roots,
                                     const char* const* paths, size_t n_fills, int flags, void** out, uint64_t* n_dropped) try {
  if (!ctx) return CP2_ERR_INVALID;
  if (out)
    for (size_t k = 0; k < n_fills; ++k) out[k] = nullptr;
  // ---- arguments, then every entry in order: before a checkpoint is opened -----------------------------------------------------------------
  const cp2_config* const* cfgs = reinterpret_cast<const cp2_config* const*>(cfgs_in);   // (void in the header, like `fills`: cp2_config* each)
  ResumeManyArgs a;
  a.cfgs = cfgs != nullptr; a.ranges = ranges != nullptr; a.slot_roots = slot_roots != nullptr; a.paths = paths != nullptr; a.out = out != nullptr;
  a.n_fills = n_fills; a.flags = flags;
  const bool lists = a.cfgs && a.ranges && a.slot_roots && a.paths;
  std::vector<ResumeManyEntry> ea(lists ? n_fills : 0);
  std::vector<Entry> e(lists ? n_fills : 0);
  for (size_t k = 0; k < e.size(); ++k) {
    e[k] = {cfgs[k], ranges[2 * k], ranges[2 * k + 1], slot_roots[k], paths[k]};
    ea[k] = {cfgs[k] != nullptr, slot_roots[k] != nullptr, paths[k] != nullptr, cfgs[k] ? cfgs[k]->cell_size : 0, cfgs[k] ? cfgs[k]->block_size : 0};
  }
  int refused_with = CP2_ERR_INVALID;                  // (a context that takes no work is CP2_ERR_HIP, by the single call's check)
  ResumeManyRefusal why;
  const bool fine = fills_resume_check_args(a, ea.data(), [&](size_t k, std::string* text) {
    const int st = fill_session_check(ctx, e[k].cfg, e[k].first_slot, e[k].n_local, e[k].slot_roots);
    if (st == CP2_OK) return false;
    refused_with = st;
    *text = ctx->err;
    return true;
  }, &why);
  if (!fine) {
    ctx->err = why.text;
    return refused_with;
  }
  if (n_fills == 0) return CP2_OK;
  CP2_REFUSE_STUCK(ctx);

  std::vector<std::unique_ptr<cp2_fill_session>> f(n_fills);
  std::vector<uint64_t> dropped(n_fills, 0);
  const int r = resume_many(ctx, e, flags, f, dropped);
  if (r != CP2_OK) {
    // nothing queued by the call reads a pooled buffer or writes a session's buffer after this; then the sessions go
    (void)hipStreamSynchronize(ctx->stream);
    f.clear();
    return r;
  }
  for (size_t k = 0; k < n_fills; ++k) out[k] = f[k].release();
  if (n_dropped) std::copy(dropped.begin(), dropped.end(), n_dropped);
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
