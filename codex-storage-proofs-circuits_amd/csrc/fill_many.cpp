// cp2_fills_add_many behind the C ABI (include/codex_p2.h): proved blocks added to many fill sessions of one context in one pass.
//
// A node that takes on slots of many datasets runs one fill session per dataset (fill.cpp), and the blocks of all of them arrive
// interleaved.  One cp2_fill_add per session is a repair_check_with pass of its own -- a data-path set-up, launches that last a wave's
// lifetime whatever their size, a drain -- for a few blocks each.  Nothing in the device work needs a chunk's blocks to belong to one
// session: k_hash_cells and the block-tree layers see block bytes only, and the path walk is per lane.  So this call is fill_add_checked's
// pass (fill.cpp) once over all n blocks: begin uploads the session table and the request arrays, stage the chunk's contiguous range of
// the packed paths, and the verdicts come from k_block_path_commit_many, which takes the session per lane.  What the call means is defined
// by the calls that exist: per session, cp2_fill_add (levels == NULL) or cp2_fill_add_anchored on the subsequence of the requests that name
// it; fill_many_plan.hpp holds that host side.  The writer takes a session's NEW requests by index from their rows of the call's data:
// no block byte is copied per session.  The writes are serial, session after session.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <new>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fill_many_plan.hpp"
#include "fill_session.hpp"
#include "repair.hpp"

using namespace cp2i;

static_assert(sizeof(FillManyDesc) == sizeof(cp2k::FillManySession) && offsetof(FillManyDesc, tree) == offsetof(cp2k::FillManySession, tree) &&
              offsetof(FillManyDesc, n_rows) == offsetof(cp2k::FillManySession, n_rows) &&
              offsetof(FillManyDesc, slot_roots) == offsetof(cp2k::FillManySession, slot_roots) &&
              offsetof(FillManyDesc, n_local) == offsetof(cp2k::FillManySession, n_local) &&
              offsetof(FillManyDesc, layer_tab) == offsetof(cp2k::FillManySession, layer_tab) &&
              offsetof(FillManyDesc, n_blocks) == offsetof(cp2k::FillManySession, n_blocks) &&
              offsetof(FillManyDesc, depth) == offsetof(cp2k::FillManySession, depth), "fill_many_plan.hpp restates the kernels' session descriptor");
static_assert(FillPlan::ANCHOR_SLOT_ROOT == ~(uint64_t)0, "k_block_path_commit_many reads UINT64_MAX as the stated slot root");

extern "C" int cp2_fills_add_many(cp2_ctx* ctx, void* const* fills, size_t n_fills, const uint64_t* req, const uint8_t* data, const uint32_t* levels,
                                  const uint8_t* paths, size_t n, uint32_t* status, size_t* n_new) try {
  if (!ctx) return CP2_ERR_INVALID;
  if (n && (!fills || !req || !data || !status)) {
    ctx->err = "fills: fills, req, data and status must not be NULL when n > 0";
    return CP2_ERR_INVALID;
  }
  if (!fills) {                                        // (n == 0: nothing to check or to do)
    if (n_new) std::fill(n_new, n_new + n_fills, (size_t)0);
    return CP2_OK;
  }
  // ---- every check of every session and request, before any device or file work ---------------------------------------------------------
  std::vector<cp2_fill_session*> f(n_fills);
  for (size_t k = 0; k < n_fills; ++k) {
    f[k] = static_cast<cp2_fill_session*>(fills[k]);
    const char* what = !f[k]                                             ? "is NULL"
                       : f[k]->ctx != ctx                                ? "belongs to another context"
                       : f[k]->cfg.cell_size != f[0]->cfg.cell_size      ? "has another cell_size than fills[0]"
                       : f[k]->cfg.block_size != f[0]->cfg.block_size    ? "has another block_size than fills[0]"
                                                                         : nullptr;
    if (what) {
      ctx->err = "fills: fills[" + std::to_string(k) + "] " + what;
      return CP2_ERR_INVALID;
    }
  }
  const size_t twice = fill_many_listed_twice(fills, n_fills);
  if (twice < n_fills) {
    ctx->err = "fills: fills[" + std::to_string(twice) + "] is listed twice: one session takes one writer";
    return CP2_ERR_INVALID;
  }
  std::vector<FillManyIn> in(n_fills);
  for (size_t k = 0; k < n_fills; ++k)
    in[k] = {&f[k]->plan, (uint64_t)(uintptr_t)f[k]->compact.p, (uint64_t)(uintptr_t)f[k]->slot_roots.p, (uint64_t)(uintptr_t)f[k]->layer_tab.p};
  FillManyPlan mp;
  FillManyRefusal why;
  if (!mp.group(req, n, n_fills, &why) || !mp.validate(in.data(), levels, paths != nullptr, &why)) {
    ctx->err = why.text;
    return CP2_ERR_INVALID;
  }
  if (n_new) std::fill(n_new, n_new + n_fills, (size_t)0);
  if (n == 0) return CP2_OK;
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  const cp2_config& c = f[0]->cfg;
  mp.tables(in.data(), req);

  // ---- the pass: fill_add_checked's, once over all n rows of `data` -----------------------------------------------------------------------
  const std::vector<uint64_t>& path_off = mp.path_off;
  DevBuf d_tab, d_sess, d_req, d_dest, d_paths, d_walk, d_levels, d_off, d_anchor;   // (go after the streams have drained: DevBuf::release)
  auto upload = [&](DevBuf& d, const void* src, size_t bytes) -> int {
    CP2_TRY(d.scratch(ctx, bytes));
    CP2_HIP(ctx, hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return CP2_OK;
  };
  RepairJudge judge;
  judge.begin = [&](size_t chunk) -> int {
    CP2_TRY(upload(d_tab, mp.table.data(), n_fills * sizeof(FillManyDesc)));
    CP2_TRY(upload(d_sess, mp.session_of.data(), n * 8));
    CP2_TRY(upload(d_req, mp.local_block.data(), n * 16));
    CP2_TRY(upload(d_dest, mp.dest.data(), n * 8));
    CP2_TRY(upload(d_levels, mp.levels.data(), n * 4));
    CP2_TRY(upload(d_off, path_off.data(), n * 8));
    CP2_TRY(upload(d_anchor, mp.anchor_row.data(), n * 8));
    const uint64_t most = mp.most_path_rows(chunk);
    CP2_TRY(d_paths.scratch(ctx, (size_t)most * 32));
    CP2_TRY(d_walk.scratch(ctx, (size_t)most * 64));
    return CP2_OK;
  };
  // the chunk's paths travel with the chunk (the previous chunk's walk, earlier on this stream, has read its own)
  judge.stage = [&](size_t c0, size_t m, hipStream_t st) -> int {
    const size_t rows = (size_t)(path_off[c0 + m] - path_off[c0]);
    if (rows) CP2_HIP(ctx, hipMemcpyAsync(d_paths.p, paths + (size_t)path_off[c0] * 32, rows * 32, hipMemcpyHostToDevice, st));
    return CP2_OK;
  };
  judge.verdicts = [&](const uint8_t* fresh, size_t c0, size_t m, uint32_t* verdict, hipStream_t st) -> int {
    CP2_HIP(ctx, cp2k::launch_block_path_commit_many(fresh, d_paths.p, static_cast<const cp2k::FillManySession*>(d_tab.p), n_fills,
                                                     static_cast<const uint64_t*>(d_sess.p) + c0, static_cast<const uint32_t*>(d_levels.p) + c0,
                                                     static_cast<const uint64_t*>(d_off.p) + c0, path_off[c0],
                                                     static_cast<const uint64_t*>(d_req.p) + 2 * c0, static_cast<const uint64_t*>(d_dest.p) + c0,
                                                     static_cast<const uint64_t*>(d_anchor.p) + c0, mp.whole, m, verdict, d_walk.p, st));
    return CP2_OK;
  };
  std::vector<uint32_t> verdict(n), st(n);
  CP2_TRY(repair_check_with(ctx, c.cell_size, c.block_size, data, n, verdict.data(), judge));

  // ---- per session: what the verdicts make known, NEW / DUPLICATE, the writer and its roll-back, presence ---------------------------------
  int r = CP2_OK;
  std::string first_err;
  double write_seconds = 0;
  size_t all_new = 0;
  for (size_t k = 0; k < n_fills; ++k) {
    auto write = [&](size_t, std::vector<uint32_t>& w) {   // the NEW blocks into "<file_base><slot>.dat": repair's writer and its rules
      const auto w0 = std::chrono::steady_clock::now();
      size_t written_n = 0;
      std::vector<FileStamp> written;
      std::string err;
      const int wr = repair_write_rows(f[k]->file_base, c.block_size, mp.pairs_of(k), data, mp.rows_of(k), w.size(), w.data(), &written_n, &written, &err);
      if (wr != CP2_OK && r == CP2_OK) {                   // the first failing file in `fills` order; the other sessions still write
        r = wr;
        first_err = err;
      }
      write_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    };
    const size_t set = mp.apply(k, f[k]->plan, verdict.data(), f[k]->from_file, write, st.data());
    if (n_new) n_new[k] = set;
    all_new += set;
  }
  std::copy(st.begin(), st.end(), status);
  if (r != CP2_OK) ctx->err = first_err;
  if (std::getenv("CP2_TRACE")) {
    size_t proved = 0;
    for (size_t i = 0; i < n; ++i) proved += verdict[i] == 0;
    const double bytes = (double)n * (double)c.block_size, seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "[cp2 trace] fills add many: %zu session(s), %zu request(s), %zu proved, %zu new, %llu sibling(s) received, %.0f bytes, "
                 "%.3f s (%.2f GB/s), %.3f s writing\n", n_fills, n, proved, all_new, (unsigned long long)path_off[n], bytes, seconds,
                 seconds > 0 ? bytes / seconds / 1e9 : 0.0, write_seconds);
  }
  return r;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
