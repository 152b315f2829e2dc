// Proof inputs across datasets behind the C ABI: cp2_proof_inputs_generate_many / cp2_proof_inputs_export_many (include/codex_p2.h).
//
// generateProofInput (reference/nim/proof_input/src/gen_input/bn254.nim:35-79) takes a dataset, a slot and an entropy on every call;
// so do these, for n requests at once.  A storage node holds one slot each of many datasets and proves every one of them each period
// with that slot's own entropy: one call here instead of one cp2_proof_input_generate (a handful of latency-bound launches and a
// synchronise) per slot.
//
// One pass over a set of requests, whatever datasets they belong to:
//   1. k_sample_many: one lane per (request, counter) -- cellIndex (sample/bn254.nim:16-27) from the request's descriptor; for
//      requests whose dataset keeps every node, the absolute device addresses of the path siblings and of the leaf; for compact
//      requests the touched network block.  One synchronise: the host needs the touched blocks.
//   2. Compact requests: the touched blocks are regenerated (k_gen_fake_cells_many, one launch for every fake-source dataset) or read
//      whole from the slot files on the context's fill threads, hashed as one batch of one-block "slots" (k_hash_cells and the layer
//      kernels: the singleton layer on top of each is not used), and each rebuilt block root is checked against its own dataset's
//      stored one.  The sampled cells of resident fake-source requests are regenerated in the same way (one more launch).
//   3. k_gather_addr: one launch fetches the paths and leaves of every request, one more the sampled cells out of the rebuilt blocks.
//   4. One download, then the cells of resident file-source requests are read on the host, and the objects are made.
// The compact work is cut into passes whose touched blocks fit the context's staging chunk (CODEX_P2_STAGE_MB).  Requests whose
// dataset keeps only its slot roots are proved one at a time (one slot rebuild each), as cp2_proof_inputs_generate_batch does.
//
// The engine behind both entry points (cp2i::prove_requests, dataset_obj.hpp) is also the compact branch of
// cp2_proof_inputs_generate_batch (proof_input.cpp): n requests on one dataset under one entropy, error texts without the request.
//
// Shared with the one-dataset routes, and not in here: the shape refusals validate() passes on (proof_shape_refusal) and the two-stage
// pipeline cp2_proof_inputs_export_many is one call of (export_in_chunks), both in proof_export.hpp; the reader of the touched blocks
// and of the sampled cells of a slot file (slot_file_read_list, fill_pipeline.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "dataset_obj.hpp"
#include "proof_input_obj.hpp"
#include "trees.hpp"

using namespace cp2i;

namespace {

struct Req {
  cp2_dataset* ds = nullptr;
  uint64_t slot = 0;
  uint8_t entropy[32];   // canonical
  size_t at = 0;         // index in the output array of this chunk
  size_t id = 0;         // index in the caller's arrays (what error texts name)
};

int refuse(cp2_ctx* ctx, size_t i, const std::string& why) {
  ctx->err = "request " + std::to_string(i) + ": " + why;
  return CP2_ERR_INVALID;
}

size_t depth_of(size_t n) { return layer_sizes_of(n).size() - 1; }

// the SampleAndProve template arguments (cp2_proof_inputs_verify's rule)
bool same_circuit(const cp2_config& a, const cp2_config& b) {
  return a.max_depth == b.max_depth && a.max_log2_nslots == b.max_log2_nslots && a.cell_size == b.cell_size && a.block_size == b.block_size &&
         a.n_samples == b.n_samples;
}

// every refusal of the contract that needs no device
int validate(cp2_ctx* ctx, cp2_dataset* const* ds, const uint64_t* slot_idx, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const cp2_dataset* d = ds[i];
    if (!d) return refuse(ctx, i, "NULL dataset");
    if (d->ctx != ctx) return refuse(ctx, i, "its dataset belongs to another context");
    const cp2_config& c = d->cfg;
    if (!same_circuit(c, ds[0]->cfg))
      return refuse(ctx, i, "its circuit parameters (maxDepth, maxLog2NSlots, cellSize, blockSize, nSamples) differ from request 0's");
    const uint64_t s = slot_idx[i];
    if (s < d->first_slot || s - d->first_slot >= d->n_local)
      return refuse(ctx, i, "slot " + std::to_string(s) + " is not local to its dataset (slots " + std::to_string(d->first_slot) + " .. " +
                                std::to_string(d->first_slot + d->n_local - 1) + ")");
    if (!d->have_roots && !(d->first_slot == 0 && d->n_local == c.n_slots))
      return refuse(ctx, i, "its dataset has no dataset tree: not all of its slots are local and cp2_dataset_set_roots was never called");
    const std::string shape = proof_shape_refusal(c, config_slot_tree_depth(c), config_dataset_tree_depth(c));
    if (!shape.empty()) return refuse(ctx, i, shape);
    if (!d->trees && d->tree_mode == 2 && d->csizes.size() - 1 != depth_of(c.n_cells / (c.block_size / c.cell_size)))
      return refuse(ctx, i, "its compact layers do not match its configuration");
  }
  return CP2_OK;
}

// The root each request's dataset tree holds for its slot (what cp2_dataset_set_roots was given) against the slot's built root: one
// gather over all requests.  In the node model the roots come from the manifest; a wrong one would give an input.json the circuit rejects.
int check_roots(cp2_ctx* ctx, cp2_dataset* const* ds, const uint64_t* slot_idx, size_t n) {
  std::vector<uint64_t> a(n);
  for (size_t i = 0; i < n; ++i)
    a[i] = (uint64_t)reinterpret_cast<uintptr_t>(dataset_roots_dev(ds[i])) + (slot_idx[i] - ds[i]->first_slot) * 32;
  std::vector<uint8_t> got(n * 32);
  DevBuf d_a, d_r;
  CP2_TRY(d_a.scratch(ctx, n * 8));
  CP2_TRY(d_r.scratch(ctx, n * 32));
  CP2_HIP(ctx, hipMemcpyAsync(d_a.p, a.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
  CP2_HIP(ctx, cp2k::launch_gather_addr(static_cast<const uint64_t*>(d_a.p), n, 32, d_r.p, ctx->stream));
  CP2_HIP(ctx, hipMemcpyAsync(got.data(), d_r.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; ++i)
    if (std::memcmp(&got[i * 32], &ds[i]->dlayers[slot_idx[i] * 32], 32) != 0)
      return refuse(ctx, i, "the root its dataset tree holds for slot " + std::to_string(slot_idx[i]) +
                                " (cp2_dataset_set_roots) differs from the slot's built root");
  return CP2_OK;
}

// checks, dataset trees and root comparison for a whole call: nothing is sampled before all of it has passed
int prepare(cp2_ctx* ctx, cp2_dataset* const* ds, const uint64_t* slot_idx, size_t n) {
  CP2_TRY(validate(ctx, ds, slot_idx, n));
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<cp2_dataset*> bare;                                             // every slot is local (validate); a dataset once
  for (size_t i = 0; i < n; ++i)
    if (!ds[i]->have_roots) bare.push_back(ds[i]);
  std::sort(bare.begin(), bare.end());
  bare.erase(std::unique(bare.begin(), bare.end()), bare.end());
  CP2_TRY(set_roots_pass(ctx, bare.data(), nullptr, bare.size(), nullptr));
  return check_roots(ctx, ds, slot_idx, n);
}

// what an error text of this call starts with: the *_many entry points name the request, the one-dataset calls have none to name
std::string who(bool named, const Req* r) { return named ? "request " + std::to_string(r->id) + ": " : std::string(); }

// One pass.  rq in this order: resident fake-source, resident file-source, compact fake-source, compact file-source requests.
int run_pass(cp2_ctx* ctx, const std::vector<const Req*>& rq, size_t n_rf, size_t n_rfile, size_t n_cf, bool named, cp2_proof_input** out) {
  const size_t n = rq.size(), nr = n_rf + n_rfile;
  const cp2_config& c0 = rq[0]->ds->cfg;
  const size_t ns = c0.n_samples, md = (size_t)c0.max_depth, cs = c0.cell_size, bs = c0.block_size, cpb = bs / cs;
  const size_t T = n * ns, R = nr * ns, C = T - R, RF = n_rf * ns, CF = n_cf * ns;
  auto store = std::make_shared<BatchStore>();
  if (T) {
    // ---- descriptors and the table of distinct tree geometries, once per pass
    std::vector<cp2k::ManyReq> reqs(n);
    std::vector<cp2k::TreeGeom> geoms;
    std::map<std::string, uint32_t> geom_of;
    for (size_t j = 0; j < n; ++j) {
      const cp2_dataset* ds = rq[j]->ds;
      cp2k::ManyReq& q = reqs[j];
      std::memset(&q, 0, sizeof q);
      std::memcpy(q.entropy, rq[j]->entropy, 32);
      std::memcpy(q.slot_root, &ds->dlayers[rq[j]->slot * 32], 32);     // layer 0 of the dataset tree (checked against the built root)
      q.n_cells = ds->cfg.n_cells;
      q.cpb = cpb;
      if (j < nr) {
        cp2k::TreeGeom g;
        std::memset(&g, 0, sizeof g);
        trees_geom(ds->trees, &g);
        auto it = geom_of.emplace(std::string(reinterpret_cast<const char*>(&g), sizeof g), (uint32_t)geoms.size());
        if (it.second) geoms.push_back(g);
        q.geom = it.first->second;
        q.nodes = (uint64_t)reinterpret_cast<uintptr_t>(ds->trees->nodes.p);
        q.slot = rq[j]->slot - ds->first_slot;
      }
    }
    // ---- host staging first: it must outlive the device scratch, whose release drains the stream, on every way out
    std::vector<uint64_t> blk(C), gen, cpaths, ctail, ccell;
    std::vector<uint8_t> checks(2 * C * 32);
    PinBuf h_blocks;
    // ---- device scratch: addresses = [paths T x md][leaves T][per compact lane: stored block root, rebuilt block root]
    const size_t rows = T * md + T + 2 * C;
    DevBuf d_req, d_geom, d_idx, d_blk, d_addr, d_rows, d_cells, d_gen, d_caddr;
    CP2_TRY(d_req.scratch(ctx, n * sizeof(cp2k::ManyReq)));
    CP2_TRY(d_geom.scratch(ctx, std::max<size_t>(1, geoms.size()) * sizeof(cp2k::TreeGeom)));
    CP2_TRY(d_idx.scratch(ctx, T * 8));
    CP2_TRY(d_blk.scratch(ctx, T * 8));
    CP2_TRY(d_addr.scratch(ctx, rows * 8));
    CP2_TRY(d_rows.scratch(ctx, rows * 32));
    CP2_TRY(d_cells.scratch(ctx, (C * cpb + T) * cs));                  // [touched blocks C x cpb cells][the sampled cells, T]
    CP2_TRY(store->idx.alloc(ctx, T * 8));
    CP2_TRY(store->paths.alloc(ctx, T * md * 32));
    CP2_TRY(store->leaves.alloc(ctx, T * 32));
    CP2_TRY(store->cells.alloc(ctx, T * cs));
    uint8_t* cells_out = d_cells.u8() + C * cpb * cs;
    uint64_t* addr = static_cast<uint64_t*>(d_addr.p);
    CP2_HIP(ctx, hipMemcpyAsync(d_req.p, reqs.data(), n * sizeof(cp2k::ManyReq), hipMemcpyHostToDevice, ctx->stream));
    if (!geoms.empty())
      CP2_HIP(ctx, hipMemcpyAsync(d_geom.p, geoms.data(), geoms.size() * sizeof(cp2k::TreeGeom), hipMemcpyHostToDevice, ctx->stream));
    CP2_HIP(ctx, cp2k::launch_sample_many(static_cast<const cp2k::ManyReq*>(d_req.p), static_cast<const cp2k::TreeGeom*>(d_geom.p), n,
                                          (uint32_t)ns, (uint32_t)md, static_cast<uint64_t*>(d_idx.p), static_cast<uint64_t*>(d_blk.p), addr,
                                          ctx->stream));
    CP2_HIP(ctx, hipMemcpyAsync(store->idx.p, d_idx.p, T * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (C) CP2_HIP(ctx, hipMemcpyAsync(blk.data(), static_cast<uint64_t*>(d_blk.p) + R, C * 8, hipMemcpyDeviceToHost, ctx->stream));
    CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t* idx = static_cast<const uint64_t*>(store->idx.p);

    // ---- fake-source cells: the touched blocks of compact requests (groups of cpb rows), the sampled cells of resident ones (rows)
    gen.assign((CF + RF) * 2, 0);
    uint64_t* seeds = gen.data();
    uint64_t* firsts = seeds + CF + RF;
    for (size_t q = 0; q < CF; ++q) {
      const Req* r = rq[nr + q / ns];
      seeds[q] = cp2_slot_seed(r->ds->cfg.seed, r->slot);
      firsts[q] = blk[q] * cpb;
    }
    for (size_t p = 0; p < RF; ++p) {
      const Req* r = rq[p / ns];
      seeds[CF + p] = cp2_slot_seed(r->ds->cfg.seed, r->slot);
      firsts[CF + p] = idx[p];
    }
    if (CF + RF) {
      CP2_TRY(d_gen.scratch(ctx, gen.size() * 8));
      const uint64_t* dg = static_cast<const uint64_t*>(d_gen.p);
      CP2_HIP(ctx, hipMemcpyAsync(d_gen.p, gen.data(), gen.size() * 8, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, cp2k::launch_gen_fake_cells_many(dg, dg + CF + RF, cpb, CF * cpb, cs, d_cells.p, ctx->stream));
      CP2_HIP(ctx, cp2k::launch_gen_fake_cells_many(dg + CF, dg + CF + RF + CF, 1, RF, cs, cells_out, ctx->stream));
    }
    // ---- file-source touched blocks: one read per block, on the fill threads, then one upload behind the generated ones
    if (C > CF) {
      const size_t n_req_file = (C - CF) / ns;
      CP2_TRY(h_blocks.alloc(ctx, (C - CF) * bs));
      std::vector<std::string> failed(fill_threads(ctx));
      on_threads(fill_threads(ctx), n_req_file, [&](int w, size_t k) {
        const size_t q0 = CF + k * ns;                                     // compact lane of the request's first counter
        const Req* r = rq[nr + q0 / ns];
        const std::string fname = slot_file_name(r->ds->file_base, r->slot);
        size_t bad = 0;
        const int err = slot_file_read_list(fname, ns, [&](size_t) { return bs; }, [&](size_t c) { return blk[q0 + c] * bs; },
                                            [&](size_t c) { return h_blocks.u8() + (q0 - CF + c) * bs; }, &bad);
        if (err >= 0)
          failed[w] = who(named, r) + (err ? "block " + std::to_string(blk[q0 + bad]) + " of slot " : std::string("slot ")) + std::to_string(r->slot) +
                      ": " + slot_file_error(fname, err);
        return err < 0;
      });
      for (const auto& f : failed)
        if (!f.empty()) { ctx->err = f; return CP2_ERR_IO; }
      CP2_HIP(ctx, hipMemcpyAsync(d_cells.u8() + CF * bs, h_blocks.p, (C - CF) * bs, hipMemcpyHostToDevice, ctx->stream));
    }
    // ---- the touched blocks' trees: one hash launch and one layer pass for all of them
    cp2_slot_trees* mini = nullptr;
    struct Mini { cp2_slot_trees*& t; ~Mini() { cp2_slot_trees_free(t); } } mini_guard{mini};
    if (C) {
      cpaths.assign(C * md, 0);
      ctail.assign(3 * C, 0);
      ccell.assign(C, 0);
      CP2_TRY(cp2_slot_trees_build_dev(ctx, d_cells.p, C, cs, bs, cpb, &mini));
      const size_t depth_b = depth_of(cpb);
      const uint64_t mb = (uint64_t)reinterpret_cast<uintptr_t>(mini->nodes.p);
      std::vector<uint64_t> rr(depth_b + 1);
      for (size_t q = 0; q < C; ++q) {
        const Req* r = rq[nr + q / ns];
        const cp2_dataset* ds = r->ds;
        const uint64_t ls = r->slot - ds->first_slot, cell = idx[R + q], b = blk[q], in_block = cell % cpb;
        const uint64_t kb = (uint64_t)reinterpret_cast<uintptr_t>(ds->compact.p);
        uint64_t* P = &cpaths[q * md];
        path_rows(mini, q, in_block, depth_b + 1, rr.data());            // inside the block (the singleton's entry above is not used)
        for (size_t d = 0; d < depth_b; ++d) P[d] = rr[d] == NO_ROW ? 0 : mb + rr[d] * 32;
        uint64_t j = b, m = ds->cfg.n_cells / cpb;
        for (size_t d = 0; d + 1 < ds->csizes.size(); ++d) {               // block root to slot root, from the stored layers (merkle.nim:21-42)
          const uint64_t sib = j ^ 1;
          P[depth_b + d] = sib < m ? kb + (ds->coff[d] + ls * ds->csizes[d] + sib) * 32 : 0;
          j >>= 1;
          m = (m + 1) >> 1;
        }
        ctail[q] = mb + (q * cpb + in_block) * 32;                         // the leaf: layer 0 of the rebuilt block
        ctail[C + 2 * q] = kb + (ds->coff[0] + ls * ds->csizes[0] + b) * 32;   // the stored block root
        ctail[C + 2 * q + 1] = mb + (mini->toff[0] + q) * 32;              // the rebuilt one
        ccell[q] = (uint64_t)reinterpret_cast<uintptr_t>(d_cells.u8()) + (q * cpb + in_block) * cs;
      }
      CP2_TRY(d_caddr.scratch(ctx, C * 8));
      CP2_HIP(ctx, hipMemcpyAsync(addr + R * md, cpaths.data(), C * md * 8, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, hipMemcpyAsync(addr + T * md + R, ctail.data(), 3 * C * 8, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, hipMemcpyAsync(d_caddr.p, ccell.data(), C * 8, hipMemcpyHostToDevice, ctx->stream));
      CP2_HIP(ctx, cp2k::launch_gather_addr(static_cast<const uint64_t*>(d_caddr.p), C, cs, cells_out + R * cs, ctx->stream));
    }
    // ---- every path and leaf in one gather, one download
    CP2_HIP(ctx, cp2k::launch_gather_addr(addr, rows, 32, d_rows.p, ctx->stream));
    CP2_HIP(ctx, hipMemcpyAsync(store->paths.p, d_rows.p, T * md * 32, hipMemcpyDeviceToHost, ctx->stream));
    CP2_HIP(ctx, hipMemcpyAsync(store->leaves.p, d_rows.u8() + T * md * 32, T * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (C) CP2_HIP(ctx, hipMemcpyAsync(checks.data(), d_rows.u8() + (T * md + T) * 32, 2 * C * 32, hipMemcpyDeviceToHost, ctx->stream));
    CP2_HIP(ctx, hipMemcpyAsync(store->cells.p, cells_out, T * cs, hipMemcpyDeviceToHost, ctx->stream));
    CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t q = 0; q < C; ++q)
      if (std::memcmp(&checks[2 * q * 32], &checks[(2 * q + 1) * 32], 32) != 0) {   // the data no longer hashes to the stored block root
        const Req* r = rq[nr + q / ns];
        ctx->err = who(named, r) + "block " + std::to_string(blk[q]) + " of slot " + std::to_string(r->slot) +
                   " does not hash to its stored root (slot data changed since the build?)";
        return CP2_ERR_IO;
      }
    // ---- resident file-source requests: the sampled cells from the slot files (slot.nim:57-68)
    if (R > RF) {
      std::vector<std::string> failed(fill_threads(ctx));
      on_threads(fill_threads(ctx), n_rfile, [&](int w, size_t k) {
        const Req* r = rq[n_rf + k];
        const std::string fname = slot_file_name(r->ds->file_base, r->slot);
        const size_t p0 = (n_rf + k) * ns;
        const int err = slot_file_read_list(fname, ns, [&](size_t) { return cs; }, [&](size_t c) { return idx[p0 + c] * cs; },
                                            [&](size_t c) { return store->cells.u8() + (p0 + c) * cs; });
        if (err >= 0) failed[w] = who(named, r) + slot_file_error(fname, err);
        return err < 0;
      });
      for (const auto& f : failed)
        if (!f.empty()) { ctx->err = f; return CP2_ERR_IO; }
    }
  }
  // ---- the objects (nothing can fail on the device any more)
  std::vector<ProofItem> items(n);
  for (size_t j = 0; j < n; ++j) items[j] = {rq[j]->ds, rq[j]->slot, rq[j]->entropy, &out[rq[j]->at]};
  return proof_inputs_from_store(items.data(), n, store, store->cells.u8());
}

}  // namespace

// The proof inputs of requests [0, n) (arrays already offset by the caller; the *_many entry points have run prepare()).  All or nothing.
int cp2i::prove_requests(cp2_ctx* ctx, cp2_dataset* const* ds, const uint64_t* slot_idx, const uint8_t* entropies, size_t n, size_t at0,
                         bool named, cp2_proof_input** out) {
  for (size_t i = 0; i < n; ++i) out[i] = nullptr;
  if (n == 0) return CP2_OK;
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<Req> req(n);
  std::vector<const Req*> res_fake, res_file, cmp_fake, cmp_file, roots_only;
  for (size_t i = 0; i < n; ++i) {
    req[i].ds = ds[i];
    req[i].slot = slot_idx[i];
    req[i].at = i;
    req[i].id = at0 + i;
    canonical_felt(entropies + 32 * i, req[i].entropy);                  // a field element in the reference (types/bn254.nim:21)
    const cp2_dataset* d = ds[i];
    (d->trees ? (d->from_file ? res_file : res_fake) : d->tree_mode == 2 ? (d->from_file ? cmp_file : cmp_fake) : roots_only).push_back(&req[i]);
  }
  auto fail = [&](int st) {
    for (size_t i = 0; i < n; ++i) { cp2_proof_input_free(out[i]); out[i] = nullptr; }
    return st;
  };
  // roots-only datasets: one slot rebuild per request, as cp2_proof_inputs_generate_batch does (not batched)
  for (const Req* r : roots_only) {
    const int st = cp2_proof_inputs_generate_batch(r->ds, &r->slot, 1, r->entropy, &out[r->at]);
    if (st != CP2_OK) {
      ctx->err = who(named, r) + ctx->err;
      return fail(st);
    }
  }
  // the rest in passes: every resident request in the first, the compact ones in chunks whose touched blocks fit the staging chunk
  const cp2_config& c0 = ds[0]->cfg;
  const size_t per_req = std::max<size_t>(1, (size_t)c0.n_samples * c0.block_size);
  const size_t chunk = std::max<size_t>(1, ctx->stage_bytes / per_req);
  std::vector<const Req*> compact(cmp_fake);
  compact.insert(compact.end(), cmp_file.begin(), cmp_file.end());
  const size_t n_res = res_fake.size() + res_file.size();
  size_t c = 0;
  for (bool first = true; first ? n_res + compact.size() > 0 : c < compact.size(); first = false) {
    std::vector<const Req*> rq;
    if (first) {
      rq = res_fake;
      rq.insert(rq.end(), res_file.begin(), res_file.end());
    }
    const size_t c1 = std::min(compact.size(), c + chunk);
    rq.insert(rq.end(), compact.begin() + (long)c, compact.begin() + (long)c1);
    const size_t n_cf = c < cmp_fake.size() ? std::min(c1, cmp_fake.size()) - c : 0;
    const int st = run_pass(ctx, rq, first ? res_fake.size() : 0, first ? res_file.size() : 0, n_cf, named, out);
    if (st != CP2_OK) return fail(st);
    c = c1;
  }
  return CP2_OK;
}

extern "C" int cp2_proof_inputs_generate_many(cp2_ctx* ctx, cp2_dataset* const* ds, const uint64_t* slot_idx, const uint8_t* entropies, size_t n,
                                              cp2_proof_input** out) try {
  if (!ctx) return CP2_ERR_INVALID;
  if (n && (!ds || !slot_idx || !entropies || !out)) {
    ctx->err = "cp2_proof_inputs_generate_many: NULL array";
    return CP2_ERR_INVALID;
  }
  for (size_t i = 0; i < n; ++i) out[i] = nullptr;
  if (n == 0) return CP2_OK;
  CP2_REFUSE_STUCK(ctx);
  CP2_TRY(prepare(ctx, ds, slot_idx, n));
  return prove_requests(ctx, ds, slot_idx, entropies, n, 0, true, out);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// The same, serialised (and written where paths[i] != NULL) as cp2_dataset_export_proof_inputs does it, by the same pipeline
// (export_in_chunks, proof_export.hpp): while the host threads turn chunk k into JSON text, the device already samples and gathers
// chunk k+1.
extern "C" int cp2_proof_inputs_export_many(cp2_ctx* ctx, cp2_dataset* const* ds, const uint64_t* slot_idx, const uint8_t* entropies, size_t n,
                                            const char* const* paths, int threads, size_t batch, uint64_t* total_bytes) try {
  if (!ctx) return CP2_ERR_INVALID;
  if (n && (!ds || !slot_idx || !entropies)) {
    ctx->err = "cp2_proof_inputs_export_many: NULL array";
    return CP2_ERR_INVALID;
  }
  if (total_bytes) *total_bytes = 0;
  if (n == 0) return CP2_OK;
  CP2_REFUSE_STUCK(ctx);
  CP2_TRY(prepare(ctx, ds, slot_idx, n));
  return export_in_chunks(n, batch, threads, [&](size_t b0, size_t m, cp2_proof_input** out) {
    return prove_requests(ctx, ds + b0, slot_idx + b0, entropies + 32 * b0, m, b0, true, out);
  }, [&](size_t i) { return paths ? paths[i] : nullptr; }, total_bytes);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
