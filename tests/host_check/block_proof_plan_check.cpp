// The block proofs' host logic (csrc/block_proof_plan.hpp, the header block_proofs.cpp uses) walked over random geometries and request
// sets, every answer compared with a direct restatement: the proof's length against the layer count of the tree, the sibling rows of
// both kept layouts against a brute-force layout built here (BLOCK_PROOF_NO_ROW exactly where the sibling index is past its layer's
// end), the (right?, key) schedule against a transcription of reconstructRoot (reference/nim/proof_input/src/merkle.nim:51-74) that
// records its compress calls, and both validations with the lowest offending index named.  Built with AddressSanitizer + UBSan.  No GPU.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "block_proof_plan.hpp"

using namespace cp2i;

static int failures = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      ++failures;                                     \
      if (failures < 20) {                            \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                     \
        std::printf("\n");                            \
      }                                               \
    }                                                 \
  } while (0)

// layer sizes of a tree over n leaves, bottom first; the bottom layer always gets one round (internal.hpp, layer_sizes_of)
static std::vector<uint64_t> layers(uint64_t n) {
  std::vector<uint64_t> s;
  uint64_t m = n;
  bool bottom = true;
  for (;;) {
    s.push_back(m);
    if (m == 1 && !bottom) break;
    m = (m + 1) / 2;
    bottom = false;
  }
  return s;
}

// merkle.nim:51-74, the compress calls recorded instead of made: (is the running hash the second argument?, the key)
struct Call { bool h_second; uint32_t key; };
static std::vector<Call> reconstruct_calls(uint64_t number_of_leaves, uint64_t leaf_index, size_t path_len) {
  std::vector<Call> calls;
  uint64_t m = number_of_leaves, j = leaf_index;
  uint32_t bottom_flag = 1;                               // KeyBottomLayer
  for (size_t i = 0; i < path_len; ++i) {
    if (j & 1) calls.push_back({true, bottom_flag});      // compressWithKey(bottomFlag, p, h)
    else if (j == m - 1) calls.push_back({false, bottom_flag + 2});   // compressWithKey(bottomFlag + 2, h, p)
    else calls.push_back({false, bottom_flag});           // compressWithKey(bottomFlag, h, p)
    bottom_flag = 0;                                      // KeyNone
    j >>= 1;
    m = (m + 1) >> 1;
  }
  return calls;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 20000;
  std::mt19937_64 rng(2468);
  auto U = [&](uint64_t n) { return n ? rng() % n : 0; };
  size_t n_rows = 0, n_absent = 0, n_odd_keys = 0, n_refused = 0, n_ok = 0;
  CHECK(block_proof_depth(0) == 0, "depth of no blocks");
  for (uint64_t nb : {1ULL, 2ULL, 3ULL, 5ULL, 6ULL, 7ULL, 8ULL, 128ULL, 131072ULL, (1ULL << 40)})
    CHECK(block_proof_depth(nb) == layers(nb).size() - 1, "depth of %llu blocks", (unsigned long long)nb);
  CHECK(block_proof_depth(1) == 1 && block_proof_depth(2) == 1 && block_proof_depth(5) == 3 && block_proof_depth(131072) == 17, "known depths");
  for (int r = 0; r < rounds; ++r) {
    // singletons, powers of two and odd sizes all come up
    const uint64_t nblocks = U(4) == 0 ? (1ULL << U(8)) : 1 + U(70), n_local = 1 + U(6), first = U(5), cpb = 1ULL << U(4);
    const std::vector<uint64_t> t = layers(nblocks), b = layers(cpb);
    const size_t depth = block_proof_depth(nblocks);
    CHECK(depth == t.size() - 1, "round %d: depth %zu of %llu blocks", r, depth, (unsigned long long)nblocks);
    // ---- the two layouts restated: every node kept = block-tree layers below the block roots over all blocks, then the big-tree layers
    // over all slots (layer-major); compact = the big-tree layers alone.  owner[row] = (layer, slot, node) of every big-tree row.
    struct Node { int layer; uint64_t slot, node; };
    uint64_t below = 0;
    for (size_t k = 0; k + 1 < b.size(); ++k) below += n_local * nblocks * b[k];
    std::vector<uint64_t> toff, coff;
    std::vector<Node> owner_c;
    uint64_t off = 0;
    for (size_t k = 0; k < t.size(); ++k) {
      toff.push_back(below + off);
      coff.push_back(off);
      for (uint64_t s = 0; s < n_local; ++s)
        for (uint64_t x = 0; x < t[k]; ++x) owner_c.push_back({(int)k, s, x});
      off += n_local * t[k];
    }
    for (int q = 0; q < 8; ++q) {
      const uint64_t local = U(n_local), blk = q == 0 ? nblocks - 1 : U(nblocks);
      std::vector<uint64_t> rows_f(depth), rows_c(depth);
      block_proof_rows(toff, t, local, blk, depth, rows_f.data());
      block_proof_rows(coff, t, local, blk, depth, rows_c.data());
      for (size_t l = 0; l < depth; ++l) {
        const uint64_t sib = (blk >> l) ^ 1;
        const bool absent = sib >= t[l];
        ++n_rows;
        n_absent += absent;
        CHECK((rows_c[l] == BLOCK_PROOF_NO_ROW) == absent && (rows_f[l] == BLOCK_PROOF_NO_ROW) == absent, "round %d: level %zu of block %llu / %llu: absent %d",
              r, l, (unsigned long long)blk, (unsigned long long)nblocks, (int)absent);
        if (absent) {
          // only the even last node of an odd layer (or the singleton) has no sibling
          CHECK((blk >> l) == t[l] - 1 && (t[l] & 1), "round %d: a sibling is absent inside a layer", r);
          continue;
        }
        CHECK(rows_c[l] < owner_c.size(), "round %d: compact row past the end", r);
        if (rows_c[l] < owner_c.size()) {
          const Node& o = owner_c[rows_c[l]];
          CHECK(o.layer == (int)l && o.slot == local && o.node == sib, "round %d: compact row of level %zu is (layer %d, slot %llu, node %llu)", r, l, o.layer,
                (unsigned long long)o.slot, (unsigned long long)o.node);
        }
        CHECK(rows_f[l] == rows_c[l] + below, "round %d: full row of level %zu", r, l);
      }
      // the block root's own row (repair_plan.hpp) is layer 0 of the same layouts
      CHECK(repair_row_compact(coff[0], t[0], local, blk) == coff[0] + local * nblocks + blk, "round %d: compact block-root row", r);
      CHECK(repair_row_full(below, 1, nblocks, local, blk) == toff[0] + local * t[0] + blk, "round %d: full block-root row", r);
      // ---- the schedule against reconstructRoot's calls
      const std::vector<BlockPathStep> s = block_proof_schedule(nblocks, blk);
      const std::vector<Call> want = reconstruct_calls(nblocks, blk, depth);
      CHECK(s.size() == want.size(), "round %d: schedule of %zu steps, want %zu", r, s.size(), want.size());
      for (size_t l = 0; l < s.size() && l < want.size(); ++l) {
        CHECK(s[l].right == want[l].h_second && s[l].key == want[l].key, "round %d: block %llu / %llu level %zu: (%d, %u), want (%d, %u)", r,
              (unsigned long long)blk, (unsigned long long)nblocks, l, (int)s[l].right, s[l].key, (int)want[l].h_second, want[l].key);
        // an odd key is used exactly where the path holds no sibling
        CHECK((s[l].key >= 2) == (rows_c[l] == BLOCK_PROOF_NO_ROW), "round %d: key %u at level %zu, row %llu", r, s[l].key, l, (unsigned long long)rows_c[l]);
        n_odd_keys += s[l].key >= 2;
      }
    }
    // ---- validation: ranges only, duplicates allowed, the lowest offending index named
    const size_t n = U(30);
    const uint64_t n_roots = 1 + U(5);
    std::vector<uint64_t> rb(2 * n), sb(2 * n);
    const bool spoil = U(3) == 0;
    for (size_t i = 0; i < n; ++i) {
      rb[2 * i] = U(n_roots + (spoil && U(8) == 0 ? 2 : 0));
      rb[2 * i + 1] = U(nblocks + (spoil && U(8) == 0 ? 2 : 0));
      if (i && U(4) == 0) { rb[2 * i] = rb[2 * (i - 1)]; rb[2 * i + 1] = rb[2 * (i - 1) + 1]; }   // repeats are fine
      sb[2 * i] = first + U(n_local + (spoil && U(8) == 0 ? 2 : 0));
      sb[2 * i + 1] = U(nblocks + (spoil && U(8) == 0 ? 2 : 0));
    }
    if (spoil && n && first && U(4) == 0) sb[2 * U(n)] = first - 1;   // below the range
    size_t bad_v = n, bad_p = n;
    for (size_t i = n; i-- > 0;) {
      if (rb[2 * i] >= n_roots || rb[2 * i + 1] >= nblocks) bad_v = i;
      if (sb[2 * i] < first || sb[2 * i] >= first + n_local || sb[2 * i + 1] >= nblocks) bad_p = i;
    }
    std::string err;
    const bool ok_v = block_verify_validate(rb.data(), n, n_roots, nblocks, &err);
    CHECK(ok_v == (bad_v == n), "round %d: verify validation says %d, want bad index %zu", r, (int)ok_v, bad_v);
    if (!ok_v) CHECK(err.find("request " + std::to_string(bad_v) + ":") != std::string::npos, "round %d: '%s' names not request %zu", r, err.c_str(), bad_v);
    err.clear();
    const bool ok_p = block_proofs_validate(sb.data(), n, first, n_local, nblocks, &err);
    CHECK(ok_p == (bad_p == n), "round %d: proofs validation says %d, want bad index %zu", r, (int)ok_p, bad_p);
    if (!ok_p) CHECK(err.find("request " + std::to_string(bad_p) + ":") != std::string::npos, "round %d: '%s' names not request %zu", r, err.c_str(), bad_p);
    n_refused += !ok_v + !ok_p;
    n_ok += ok_v + ok_p;
  }
  std::printf("block proof plan: %d rounds, %zu sibling rows (%zu absent), %zu odd keys, %zu request sets valid and %zu refused, %d failures\n", rounds, n_rows,
              n_absent, n_odd_keys, n_ok, n_refused, failures);
  if (failures || n_absent == 0 || n_odd_keys == 0 || n_refused == 0) return 1;
  std::printf("block proof plan ok\n");
  return 0;
}
