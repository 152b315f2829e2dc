// cp2_fills_finish_many behind the C ABI (include/codex_p2.h): many fill sessions of one context finished in one pass.
//
// A node that takes on slots of many datasets runs one fill session per dataset.  cp2_fill_finish (fill.cpp) is per session one
// k_compress_layer launch per layer of the tree over the block roots -- in a one-slot session each a lone wave or less --, an upload of a
// row table, a k_repair_compare launch, a download and a drain.  Nothing of that device work is session-wide but launch arguments: here
// level l of every session's trees is ONE launch of k_finish_layer_many, which takes the session per lane from the descriptor table
// cp2_fills_add_many already uses and compares with the stated roots on each tree's last level.  One upload of the tables, one launch per
// level, one download of one verdict per (session, local slot), one drain.  What the call means is defined by the call that exists:
// per session, cp2_fill_finish; fill_finish_plan.hpp holds the host side -- the checks, the tables, the verdict index turned back into
// (fills index, slot), and the order saves -> objects -> hand-over that keeps the call all or nothing.  The kept forms are written serially
// in `fills` order through the single call's kept_save / kept_meta / kept_cache_path.
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

#include "cache_file.hpp"
#include "fill_finish_plan.hpp"
#include "fill_session.hpp"
#include "kernels.hpp"
#include "trees.hpp"

using namespace cp2i;

extern "C" int cp2_fills_finish_many(cp2_ctx* ctx, void* const* fills, size_t n_fills, const char* const* cache_paths, cp2_dataset** out) try {
  if (!ctx) return CP2_ERR_INVALID;
  if (n_fills && (!fills || !out)) {
    ctx->err = "fills: fills and out must not be NULL when n_fills > 0";
    return CP2_ERR_INVALID;
  }
  if (n_fills == 0) return CP2_OK;
  // ---- every check of every session, before any device or file work -------------------------------------------------------------------------
  std::vector<cp2_fill_session*> f(n_fills);
  std::vector<FillFinishIn> in(n_fills);
  for (size_t k = 0; k < n_fills; ++k) {
    f[k] = static_cast<cp2_fill_session*>(fills[k]);
    if (f[k]) in[k] = {&f[k]->plan, f[k]->ctx == ctx, (uint64_t)(uintptr_t)f[k]->compact.p, (uint64_t)(uintptr_t)f[k]->slot_roots.p};
  }
  FillFinishRefusal why;
  if (!fill_finish_check(fills, in.data(), n_fills, &why)) {
    ctx->err = why.text;
    return CP2_ERR_INVALID;
  }
  CP2_REFUSE_STUCK(ctx);
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  const auto ms_since = [](std::chrono::steady_clock::time_point a) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count() * 1e3;
  };
  FillFinishPlan fp;
  fp.tables(in.data(), n_fills);

  // ---- the pass: one upload, one launch per level, one download, one drain --------------------------------------------------------------
  // the device tables travel as one block: descriptors, verdict offsets, prefixes (8-byte entries), then sess_of (4-byte entries)
  const size_t b_tab = n_fills * sizeof(FillManyDesc), b_voff = fp.voff.size() * 8, b_pre = fp.prefix.size() * 8, b_sess = fp.sess_of.size() * 4;
  const size_t nv = (size_t)fp.n_verdicts();
  std::vector<uint8_t> host(b_tab + b_voff + b_pre + b_sess);
  std::memcpy(host.data(), fp.table.data(), b_tab);
  std::memcpy(host.data() + b_tab, fp.voff.data(), b_voff);
  if (b_pre) std::memcpy(host.data() + b_tab + b_voff, fp.prefix.data(), b_pre);
  if (b_sess) std::memcpy(host.data() + b_tab + b_voff + b_pre, fp.sess_of.data(), b_sess);
  DevBuf d_tables, d_verdict;                       // (go after the stream has drained: DevBuf::release)
  CP2_TRY(d_tables.scratch(ctx, host.size()));
  CP2_TRY(d_verdict.scratch(ctx, nv * 4));
  std::vector<uint32_t> verdict(nv);
  const auto t1 = std::chrono::steady_clock::now();
  CP2_HIP(ctx, hipMemcpyAsync(d_tables.p, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
  CP2_HIP(ctx, cp2k::launch_finish_layers_many(reinterpret_cast<const cp2k::FillManySession*>(d_tables.u8()), n_fills,
                                               reinterpret_cast<const uint64_t*>(d_tables.u8() + b_tab),
                                               reinterpret_cast<const uint64_t*>(d_tables.u8() + b_tab + b_voff),
                                               reinterpret_cast<const uint32_t*>(d_tables.u8() + b_tab + b_voff + b_pre), fp.level_off.data(),
                                               fp.level_cnt.data(), fp.level_work.data(), fp.n_levels(), static_cast<uint32_t*>(d_verdict.p),
                                               ctx->stream));
  CP2_HIP(ctx, hipMemcpyAsync(verdict.data(), d_verdict.p, nv * 4, hipMemcpyDeviceToHost, ctx->stream));
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const double ms_plan = std::chrono::duration<double>(t1 - t0).count() * 1e3, ms_device = ms_since(t1);
  if (fp.first_mismatch(verdict.data(), in.data(), &why)) {   // no dataset is made, no session is finished
    ctx->err = why.text;
    return CP2_ERR_IO;
  }

  // ---- saves, then the n objects, then the hand-overs: fill_finish_commit's order ---------------------------------------------------------
  std::vector<std::unique_ptr<cp2_dataset>> ds(n_fills);
  size_t saved = 0;
  const auto t2 = std::chrono::steady_clock::now();
  auto t3 = t2;
  const int r = fill_finish_commit(
      n_fills, [&](size_t k) { return cache_paths && cache_paths[k]; },
      [&](size_t k) {
        ctx->err.clear();                                          // what a failing save says is its own, not an earlier call's
        const int st = kept_save(ctx, kept_cache_path(cache_paths[k]).c_str(),
                                 kept_meta(f[k]->cfg, f[k]->plan.first_slot, f[k]->plan.n_local, f[k]->from_file, f[k]->file_base, 2), f[k]->compact.p,
                                 f[k]->plan.rows * 32);
        if (st != CP2_OK && ctx->err.empty()) ctx->err = std::string("fill: cannot write the kept layers to ") + cache_paths[k];
        if (st != CP2_OK) ctx->err = "fills: fills[" + std::to_string(k) + "]: " + ctx->err;
        return st;
      },
      [&](size_t k) {
        if (k == 0) t3 = std::chrono::steady_clock::now();
        ds[k] = fill_dataset_shell(f[k]);
        return ds[k] != nullptr;
      },
      [&](size_t k) {
        hand_over(f[k]->compact, ds[k]->compact);
        f[k]->plan.finished = true;
      },
      CP2_ERR_ALLOC, &saved);
  if (r != CP2_OK) return r;
  for (size_t k = 0; k < n_fills; ++k) out[k] = ds[k].release();
  if (std::getenv("CP2_TRACE"))
    std::fprintf(stderr, "[cp2 trace] fills finish many: %zu session(s), %zu slot(s), %llu row(s) built, %zu launch(es), %zu kept form(s) saved, "
                 "%.3f ms (%.3f planning, %.3f tables up + launches + verdicts down, %.3f saving, %.3f objects and hand-over)\n", n_fills, nv,
                 (unsigned long long)fp.rows_built, fp.launches, saved, ms_since(t0), ms_plan, ms_device,
                 std::chrono::duration<double>(t3 - t2).count() * 1e3, ms_since(t3));
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
