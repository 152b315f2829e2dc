// Proof inputs read back and checked as the circuit checks them, behind the C ABI (include/codex_p2.h):
//   cp2_proof_input_parse_json   input.json text -> a cp2_proof_input holding the field elements the circuit reads (json_parse.hpp)
//   cp2_proof_input_cell_felts   the sampled cells as those field elements
//   cp2_proof_inputs_verify      what SampleAndProve accepts (circuit/codex/sample_cells.circom:58-148), on the GPU (k_verify_samples)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "json_parse.hpp"
#include "kernels.hpp"
#include "proof_input_obj.hpp"

using namespace cp2i;

namespace {

int refuse(char* msg, size_t msg_len, const std::string& why) {
  if (msg && msg_len) std::snprintf(msg, msg_len, "%s", why.c_str());
  return CP2_ERR_INVALID;
}

bool pow2(uint64_t x) { return x && !(x & (x - 1)); }

// the circuit parameters every object of one verification batch shares
struct Circuit {
  size_t md, m, cs, nf, ns, bd;
};

int circuit_of(const cp2_proof_input* p, Circuit* c, std::string* why) {
  const cp2_config& g = p->cfg;
  if (g.max_depth < 0 || g.max_depth > 64 || g.max_log2_nslots < 0 || g.max_log2_nslots > 63) {
    *why = "maxDepth must be in [0, 64] and maxLog2NSlots in [0, 63]";
    return CP2_ERR_INVALID;
  }
  if (g.cell_size == 0 || g.block_size % g.cell_size || !pow2(g.block_size / g.cell_size) || g.block_size / g.cell_size < 2) {
    *why = "blockSize / cellSize must be a power of two >= 2 (blockTreeDepth >= 1)";
    return CP2_ERR_INVALID;
  }
  c->md = (size_t)g.max_depth;
  c->m = (size_t)g.max_log2_nslots;
  c->cs = g.cell_size;
  c->nf = cp2_felts_per_bytes(g.cell_size);
  c->ns = p->n_samples;
  c->bd = (size_t)__builtin_ctzll(g.block_size / g.cell_size);
  if (c->bd > c->md) {
    *why = "blockTreeDepth exceeds maxDepth";
    return CP2_ERR_INVALID;
  }
  if (c->ns > 0xffffffffULL || c->nf > 0x7fffffffULL) {
    *why = "nSamples or cellSize out of range";
    return CP2_ERR_INVALID;
  }
  return CP2_OK;
}

// witness generation's assertions (lib/log2.circom Log2_CircomWitnessCalc_Hack and CeilingLog2, misc.circom ToBits)
bool shape_ok(const cp2_proof_input* p, const Circuit& c) {
  const uint64_t nc = p->cfg.n_cells, nsl = p->cfg.n_slots;
  if (!pow2(nc) || nc < 2 || (size_t)__builtin_ctzll(nc) > c.md) return false;   // nCells = 2^k, 1 <= k <= maxDepth
  if (nsl == 0 || ((nsl - 1) >> c.m) != 0) return false;                          // ToBits(maxLog2NSlots) of nSlots - 1
  return (p->slot_idx >> c.m) == 0;                                               // ToBits(maxLog2NSlots) of slotIndex
}

template <class F>
void parallel_for(size_t n, size_t threads, F f) {
  threads = std::max<size_t>(1, std::min(threads, n));
  if (threads == 1) {
    for (size_t i = 0; i < n; ++i) f(i);
    return;
  }
  std::vector<std::thread> th;
  for (size_t w = 0; w < threads; ++w)
    th.emplace_back([&, w] {
      for (size_t i = w; i < n; i += threads) f(i);
    });
  for (auto& t : th) t.join();
}

}  // namespace

extern "C" int cp2_proof_input_parse_json(const cp2_config* cfg, const char* text, size_t len, cp2_proof_input** out, char* msg,
                                          size_t msg_len) try {
  if (msg && msg_len) msg[0] = 0;
  if (!cfg || !out || (!text && len)) return refuse(msg, msg_len, "null argument");
  *out = nullptr;
  if (cfg->max_depth < 0 || cfg->max_log2_nslots < 0 || cfg->cell_size == 0)
    return refuse(msg, msg_len, "configuration: maxDepth, maxLog2NSlots >= 0 and cellSize > 0 required");
  cp2parse::Parsed r;
  std::string err;
  if (!cp2parse::parse_proof_input(text, len, (size_t)cfg->max_depth, (size_t)cfg->max_log2_nslots, cfg->cell_size, cfg->n_samples, r,
                                   &err))
    return refuse(msg, msg_len, err);
  std::unique_ptr<cp2_proof_input> p(new cp2_proof_input());
  p->cfg = *cfg;
  p->cfg.file_base = nullptr;
  p->cfg.n_cells = r.n_cells;
  p->cfg.n_slots = r.n_slots;
  p->cfg.n_samples = r.n_samples;
  p->slot_idx = r.slot_idx;
  std::memcpy(p->dataset_root, r.dataset_root, 32);
  std::memcpy(p->entropy, r.entropy, 32);
  std::memcpy(p->slot_root, r.slot_root, 32);
  p->slot_proof = std::move(r.slot_proof);
  p->n_samples = r.n_samples;
  const size_t ns = r.n_samples, nf = cp2_felts_per_bytes(cfg->cell_size), cs = cfg->cell_size;
  auto store = std::make_shared<BatchStore>();
  const size_t o_felts = 0, o_paths = o_felts + r.cell_felts.size(), o_cells = o_paths + r.paths.size();
  store->heap.assign(o_cells + ns * cs + 8, 0);
  uint8_t* h = store->heap.data();
  if (!r.cell_felts.empty()) std::memcpy(h + o_felts, r.cell_felts.data(), r.cell_felts.size());
  if (!r.paths.empty()) std::memcpy(h + o_paths, r.paths.data(), r.paths.size());
  bool bytes = true;   // every row the 10*-padded encoding of cellSize bytes?
  for (size_t i = 0; i < ns && bytes; ++i) bytes = cp2parse::felts_to_cell_bytes(h + o_felts + i * nf * 32, nf, cs, h + o_cells + i * cs);
  p->store = store;
  p->cell_felts = h + o_felts;
  p->paths = h + o_paths;
  p->cell_data = bytes ? h + o_cells : nullptr;
  *out = p.release();
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_proof_input_shape(const cp2_proof_input* p, uint64_t* n_cells, uint64_t* n_slots, uint64_t* slot_idx) {
  if (!p) return CP2_ERR_INVALID;
  if (n_cells) *n_cells = p->cfg.n_cells;
  if (n_slots) *n_slots = p->cfg.n_slots;
  if (slot_idx) *slot_idx = p->slot_idx;
  return CP2_OK;
}

extern "C" int cp2_proof_input_cell_felts(const cp2_proof_input* p, uint8_t* out) try {
  if (!p || (!out && p->n_samples)) return CP2_ERR_INVALID;
  const size_t nf = cp2_felts_per_bytes(p->cfg.cell_size), cs = p->cfg.cell_size;
  if (p->cell_felts) {
    std::memcpy(out, p->cell_felts, p->n_samples * nf * 32);
    return CP2_OK;
  }
  if (p->n_samples && !p->cell_data) return CP2_ERR_INVALID;
  for (size_t i = 0; i < p->n_samples; ++i) CP2_TRY(cp2_bytes_to_felts(p->cell_data + i * cs, cs, out + i * nf * 32));
  return CP2_OK;
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_proof_inputs_verify(cp2_ctx* ctx, const cp2_proof_input* const* ps, size_t n, uint32_t* status,
                                       uint8_t* sample_ok) try {
  if (!ctx) return CP2_ERR_INVALID;
  ctx->err.clear();
  CP2_REFUSE_STUCK(ctx);
  if (n == 0) return CP2_OK;
  if (!ps || !status) return CP2_ERR_INVALID;
  // every length is checked before anything is packed: a wrong input is wrong data, never a wrong read
  Circuit c{};
  for (size_t i = 0; i < n; ++i) {
    const cp2_proof_input* p = ps[i];
    if (!p) {
      ctx->err = "proof input " + std::to_string(i) + " is NULL";
      return CP2_ERR_INVALID;
    }
    Circuit ci{};
    std::string why;
    if (circuit_of(p, &ci, &why) != CP2_OK) {
      ctx->err = "proof input " + std::to_string(i) + ": " + why;
      return CP2_ERR_INVALID;
    }
    if (i == 0) {
      c = ci;
    } else if (ci.md != c.md || ci.m != c.m || ci.cs != c.cs || ci.bd != c.bd || ci.ns != c.ns) {
      ctx->err = "proof input " + std::to_string(i) + " has other circuit parameters than proof input 0";
      return CP2_ERR_INVALID;
    }
    if (p->slot_proof.size() != c.m * 32 || (p->n_samples && (!p->paths || !(p->cell_felts || p->cell_data)))) {
      ctx->err = "proof input " + std::to_string(i) + " lacks its slot proof, cells or paths";
      return CP2_ERR_INVALID;
    }
  }
  const size_t ns = c.ns, nf = c.nf, md = c.md, m = c.m;
  std::vector<uint8_t> shape(n);
  for (size_t i = 0; i < n; ++i) shape[i] = shape_ok(ps[i], c) ? 1 : 0;

  // per input: 4 parameter words, the head felts, the cell and path felts; the verdict bytes after all of them
  const size_t b_prm = 32, b_head = (3 + m) * 32, b_cells = ns * nf * 32, b_paths = ns * md * 32;
  const size_t per_input = b_prm + b_head + b_cells + b_paths + ns + 1;
  constexpr size_t CHUNK_BYTES = (size_t)256 << 20;   // device memory stays bounded whatever n is
  const size_t chunk = std::max<size_t>(1, std::min(n, CHUNK_BYTES / per_input));
  const size_t slot_bytes = chunk * per_input + 64;
  struct Slot {
    PinBuf host;
    DevBuf dev;
    Event done;                 // (after the buffers: it goes before they wait for the stream and go back to the pool)
    size_t first = 0, count = 0;
    bool busy = false;
  };
  Slot slots[2];
  const int n_slots = n > chunk ? 2 : 1;
  for (int k = 0; k < n_slots; ++k) {
    CP2_TRY(slots[k].host.alloc(ctx, slot_bytes));
    CP2_TRY(slots[k].dev.scratch(ctx, slot_bytes));
    CP2_TRY(slots[k].done.create(ctx));
  }
  // offsets inside a slot for a chunk of q inputs (all 32-byte multiples up to the verdict bytes)
  auto offs = [&](size_t q, size_t* o_head, size_t* o_cells, size_t* o_paths, size_t* o_ok) {
    *o_head = q * b_prm;
    *o_cells = *o_head + q * b_head;
    *o_paths = *o_cells + q * b_cells;
    *o_ok = *o_paths + q * b_paths;
  };
  const size_t threads = std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));

  auto harvest = [&](Slot& s) -> int {
    if (!s.busy) return CP2_OK;
    CP2_HIP(ctx, hipEventSynchronize(s.done));
    size_t o_head, o_cells, o_paths, o_ok;
    offs(s.count, &o_head, &o_cells, &o_paths, &o_ok);
    const uint8_t* ok = s.host.u8() + o_ok;
    for (size_t j = 0; j < s.count; ++j) {
      const size_t i = s.first + j;
      uint8_t* so = sample_ok ? sample_ok + i * ns : nullptr;
      if (!shape[i]) {
        status[i] = CP2_VERIFY_SHAPE;
        if (so) std::memset(so, 0, ns);
        continue;
      }
      uint32_t st = ok[s.count * ns + j] ? 0u : CP2_VERIFY_DATASET_ROOT;
      for (size_t k = 0; k < ns; ++k)
        if (!ok[j * ns + k]) st |= CP2_VERIFY_SAMPLE;
      status[i] = st;
      if (so) std::memcpy(so, ok + j * ns, ns);
    }
    s.busy = false;
    return CP2_OK;
  };

  const hipStream_t st = ctx->stream;
  size_t k = 0;
  for (size_t first = 0; first < n; first += chunk, ++k) {
    Slot& s = slots[k % n_slots];
    CP2_TRY(harvest(s));   // the chunk that used this slot two turns ago (its copies and kernel are done with the buffers)
    const size_t q = std::min(chunk, n - first);
    size_t o_head, o_cells, o_paths, o_ok;
    offs(q, &o_head, &o_cells, &o_paths, &o_ok);
    uint8_t* h = s.host.u8();
    parallel_for(q, threads, [&](size_t j) {   // the previous chunk's copies and kernel run meanwhile
      const cp2_proof_input* p = ps[first + j];
      uint64_t prm[4] = {p->cfg.n_cells, p->cfg.n_slots, p->slot_idx, shape[first + j]};
      std::memcpy(h + j * b_prm, prm, 32);
      uint8_t* hd = h + o_head + j * b_head;
      std::memcpy(hd, p->dataset_root, 32);
      std::memcpy(hd + 32, p->entropy, 32);
      std::memcpy(hd + 64, p->slot_root, 32);
      if (m) std::memcpy(hd + 96, p->slot_proof.data(), m * 32);
      if (!shape[first + j]) return;   // the kernel reads nothing else of it
      uint8_t* cf = h + o_cells + j * b_cells;
      if (p->cell_felts) std::memcpy(cf, p->cell_felts, b_cells);
      else
        for (size_t r = 0; r < ns; ++r) (void)cp2_bytes_to_felts(p->cell_data + r * c.cs, c.cs, cf + r * nf * 32);
      if (b_paths) std::memcpy(h + o_paths + j * b_paths, p->paths, b_paths);
    });
    CP2_HIP(ctx, hipMemcpyAsync(s.dev.p, h, o_ok, hipMemcpyHostToDevice, st));
    cp2k::VerifyGeom g{q, (uint32_t)ns, (uint32_t)nf, (uint32_t)md, (uint32_t)m, (uint32_t)c.bd};
    uint8_t* d = s.dev.u8();
    CP2_HIP(ctx, cp2k::launch_verify_samples(g, reinterpret_cast<const uint64_t*>(d), d + o_head, d + o_cells, d + o_paths, d + o_ok, st));
    CP2_HIP(ctx, hipMemcpyAsync(h + o_ok, d + o_ok, q * ns + q, hipMemcpyDeviceToHost, st));
    CP2_HIP(ctx, hipEventRecord(s.done, st));
    s.first = first;
    s.count = q;
    s.busy = true;
  }
  for (size_t j = 0; j < 2; ++j) CP2_TRY(harvest(slots[(k + j) % n_slots]));
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}
