// The host side every proof-input route shares: what refuses a shape the reference would assert on, slotProof, the name of an
// input.json, the malloc'ed text the text-returning calls hand out, the strided formatting fan-out and the two-stage export pipeline.
// No HIP in here: tests/host_check/proof_export_check.cpp runs it on the CPU, with stand-ins for the generate and format steps, under
// AddressSanitizer + UBSan and again under ThreadSanitizer.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/codex_p2.h"
#include "workers.hpp"

namespace cp2i {

// Why generateProofInput (gen_input/bn254.nim:35-79) would not get through with this configuration -- the reference asserts, these
// calls refuse -- or nothing when it would.  The depths are those of the trees the paths come from (a unit's tree plus the levels above
// it where slots are cut into units).  Every route asks here: the *_many calls pass the text on, the others return CP2_ERR_INVALID.
inline std::string proof_shape_refusal(const cp2_config& c, size_t slot_tree_depth, size_t dataset_tree_depth) {
  // cellIndex asserts a power of two (sample/bn254.nim:19-20) and extractLowBits asserts k > 0 bits (types/bn254.nim:48)
  if (c.n_cells == 0 || (c.n_cells & (c.n_cells - 1)) || (c.n_samples && c.n_cells < 2))
    return "nCells " + std::to_string(c.n_cells) + " is not a power of two >= 2";
  // padMerkleProof asserts that a proof is no longer than what it is padded to (types.nim:29): every merged cell proof to maxDepth
  // (gen_input/bn254.nim:63) ...
  if (c.max_depth < 0 || slot_tree_depth > (size_t)c.max_depth) return "its slot tree is deeper than maxDepth";
  // ... and slotProof to maxLog2NSlots (gen_input/bn254.nim:72)
  if (c.max_log2_nslots < 0 || dataset_tree_depth > (size_t)c.max_log2_nslots) return "its dataset tree is deeper than maxLog2NSlots";
  return std::string();
}

// slotProof = padMerkleProof(merkleProof(dsetTree, slotIdx), maxLog2NSlots), gen_input/bn254.nim:51,72: `dlayers` holds every layer of
// the dataset tree over n_slots roots, bottom first, `dsizes` their sizes; a sibling past the end of an odd layer is zero, like the padding
inline void slot_proof_of(const std::vector<uint8_t>& dlayers, const std::vector<size_t>& dsizes, size_t n_slots, size_t max_log2_nslots,
                          uint64_t slot, std::vector<uint8_t>& out) {
  out.assign(max_log2_nslots * 32, 0);
  size_t k = slot, m = n_slots, off = 0;
  for (size_t i = 0; i + 1 < dsizes.size(); ++i) {
    const size_t j = k ^ 1;
    if (j < m) std::memcpy(&out[i * 32], &dlayers[(off + j) * 32], 32);
    off += dsizes[i];
    k >>= 1;
    m = (m + 1) >> 1;
  }
}

// "<dir>/input_<slot>.json": where every export puts a slot's text
inline std::string input_json_name(const char* dir, uint64_t slot) { return std::string(dir) + "/input_" + std::to_string(slot) + ".json"; }

// a text into a malloc'ed, NUL-terminated buffer the caller releases with cp2_free_buffer; len may be NULL
inline int text_to_malloc(const std::string& s, char** text, size_t* len) {
  char* buf = (char*)std::malloc(s.size() + 1);
  if (!buf) return CP2_ERR_ALLOC;
  std::memcpy(buf, s.data(), s.size());
  buf[s.size()] = 0;
  *text = buf;
  if (len) *len = s.size();
  return CP2_OK;
}

// The formatting fan-out: f(t, i, &bytes) for i = t, t + threads, ... on thread t of `threads` (at most n of them; the calling thread
// is thread 0), every thread adding what it formatted to its own byte count.  A status other than CP2_OK is kept and the thread goes
// on (its last one counts); a task that throws ends its thread with CP2_ERR_ALLOC.  Returns the status of the lowest thread that has
// one, with *total_bytes untouched, or CP2_OK with the sum in *total_bytes (may be NULL).
template <typename F>
int format_strided(size_t n, int threads, F f, uint64_t* total_bytes) {
  if (threads < 1) threads = 1;
  if ((size_t)threads > n) threads = n ? (int)n : 1;
  std::vector<int> status(threads, CP2_OK);
  std::vector<uint64_t> bytes(threads, 0);
  auto work = [&](int t) {
    try {
      for (size_t i = (size_t)t; i < n; i += (size_t)threads) {
        const int st = f(t, i, &bytes[t]);
        if (st != CP2_OK) status[t] = st;
      }
    } catch (...) {
      status[t] = CP2_ERR_ALLOC;
    }
  };
  {
    Workers pool(threads > 1 ? threads - 1 : 1);   // joined by its destructor on every path out of this scope
    for (int t = 1; t < threads; ++t) pool.submit([&work, t] { work(t); });
    work(0);
    pool.wait_idle();
  }
  uint64_t tot = 0;
  for (int t = 0; t < threads; ++t) {
    tot += bytes[t];
    if (status[t] != CP2_OK) return status[t];
  }
  if (total_bytes) *total_bytes = tot;
  return CP2_OK;
}

// The two-stage export pipeline: proof inputs for requests [0, n) in chunks of `batch` (0: 512), chunk k + 1 generated on one
// producer thread -- generate(b0, m, out) makes the objects of requests [b0, b0 + m) or none -- while chunk k goes through
// cp2_proof_inputs_write_json_batch on `threads` host threads, request i written to path_of(i) unless that is NULL.  The objects are
// freed on every way out.  The first chunk that fails ends the export; where the formatter and the generator of the chunk after it
// both fail, the formatter's status is the one returned.  *total_bytes (may be NULL): the texts of the chunks that were formatted.
template <typename Generate, typename PathOf>
int export_in_chunks(size_t n, size_t batch, int threads, Generate generate, PathOf path_of, uint64_t* total_bytes) {
  if (batch == 0) batch = 512;
  if (batch > n) batch = n;                                  // (and b0 + batch below cannot wrap)
  if (threads < 1) threads = 1;
  uint64_t bytes = 0;
  int status = CP2_OK;
  std::vector<cp2_proof_input*> cur, next;
  struct Release {   // whatever leaves this scope, the objects are freed
    std::vector<cp2_proof_input*>& v;
    ~Release() { for (auto* p : v) cp2_proof_input_free(p); v.clear(); }
  } rel_cur{cur}, rel_next{next};
  auto make = [&](size_t b0, std::vector<cp2_proof_input*>& o) -> int {   // (runs on the producer thread: nothing may leave it but a status)
    try {
      const size_t m = std::min(batch, n - b0);
      o.assign(m, nullptr);
      return generate(b0, m, o.data());
    } catch (const std::bad_alloc&) {
      return CP2_ERR_ALLOC;
    } catch (...) {
      return CP2_ERR_INVALID;
    }
  };
  if (n) status = make(0, cur);
  for (size_t b0 = 0; status == CP2_OK && b0 < n; b0 += batch) {
    const size_t b1 = b0 + batch;
    // paths first: nothing below may throw while the producer task is in flight except into the pool's joining destructor
    std::vector<const char*> paths(cur.size());
    for (size_t i = 0; i < cur.size(); ++i) paths[i] = path_of(b0 + i);
    int gen_status = CP2_OK, st = CP2_OK;
    uint64_t got = 0;
    {
      Workers producer(1);                                   // device stage of the NEXT chunk; joined when this scope ends
      if (b1 < n) producer.submit([&] { gen_status = make(b1, next); });
      st = cp2_proof_inputs_write_json_batch(cur.data(), cur.size(), paths.data(), threads, &got);
    }
    bytes += got;
    for (auto* p : cur) cp2_proof_input_free(p);
    cur.clear();
    if (st != CP2_OK) status = st;
    else if (gen_status != CP2_OK) status = gen_status;
    cur.swap(next);
  }
  if (total_bytes) *total_bytes = bytes;
  return status;
}

}  // namespace cp2i
