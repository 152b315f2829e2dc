// A fill session's host logic (csrc/fill_plan.hpp, the header fill.cpp uses) walked over random geometries, request sets and write
// failures, every answer compared with a direct restatement kept here: the compact layout against a brute-force one, destination rows
// inside layer 0 and distinct per block, validation with the lowest offending index named, NEW / DUPLICATE against a map walked in index
// order, the UNWRITTEN roll-back leaving its blocks missing, the bitmap and the ordered missing list against a std::set, the capped and
// the counting form of the list, and the finish precondition with its count and first pair.  Built with AddressSanitizer + UBSan.  No GPU.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "fill_plan.hpp"

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

typedef std::pair<uint64_t, uint64_t> Pair;

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 2000;
  std::mt19937_64 rng(20261017);
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  std::string err;

  // ---- the range check: dataset_check's rules and the power of two --------------------------------------------------------------------
  CHECK(fill_check_range(11, 0, 11, 32, 8, 512, 2048, 0, &err), "the reference default is refused: %s", err.c_str());
  CHECK(fill_check_range(11, 3, 8, 32, 8, 512, 2048, 16384, &err), "a tail range is refused");
  CHECK(!fill_check_range(11, 0, 0, 32, 8, 512, 2048, 0, &err), "n_local == 0 is accepted");
  CHECK(!fill_check_range(11, 12, 1, 32, 8, 512, 2048, 0, &err), "first_slot past the dataset is accepted");
  CHECK(!fill_check_range(11, 4, 8, 32, 8, 512, 2048, 0, &err), "a range past the dataset's end is accepted");
  CHECK(!fill_check_range(11, 1, ~0ULL, 32, 8, 512, 2048, 0, &err), "a wrapping range is accepted");
  CHECK(!fill_check_range(11, 0, 11, -1, 8, 512, 2048, 0, &err) && !fill_check_range(11, 0, 11, 32, -1, 512, 2048, 0, &err), "negative depths are accepted");
  CHECK(!fill_check_range(11, 0, 11, 32, 8, 0, 2048, 0, &err) && !fill_check_range(11, 0, 11, 32, 8, 96, 2048, 0, &err) &&
        err.find("power of two") != std::string::npos, "nCells that is not a power of two is accepted");
  CHECK(!fill_check_range(11, 0, 11, 32, 8, 512, 16385, 16384, &err) && fill_check_range(11, 0, 11, 32, 8, 512, 16385, 0, &err),
        "the slot-file cell limit applies to the wrong source");

  for (int round = 0; round < rounds; ++round) {
    const uint64_t n_blocks = round % 7 == 0 ? 1 : (round % 5 == 0 ? pick(1, 70) : (uint64_t)1 << pick(0, 6));
    const uint64_t n_local = pick(1, 5), first_slot = pick(0, 9);
    FillPlan p;
    p.init(first_slot, n_local, n_blocks);

    // ---- the compact layout: dataset_alloc_kept's, layer-major over the local slots ---------------------------------------------------
    const std::vector<uint64_t> want = layers(n_blocks);
    CHECK(p.csizes.size() == want.size() && p.coff.size() == want.size(), "%llu blocks: %zu layers, want %zu", (unsigned long long)n_blocks,
          p.csizes.size(), want.size());
    uint64_t off = 0;
    for (size_t k = 0; k < want.size() && k < p.csizes.size(); ++k) {
      CHECK(p.csizes[k] == want[k] && p.coff[k] == off, "layer %zu: size %zu at %zu, want %llu at %llu", k, p.csizes[k], p.coff[k],
            (unsigned long long)want[k], (unsigned long long)off);
      off += n_local * want[k];
    }
    CHECK(p.rows == off && p.csizes.back() == 1, "rows %zu, want %llu", p.rows, (unsigned long long)off);
    CHECK(p.total() == n_local * n_blocks && p.n_missing() == p.total() && p.bits.size() == (p.total() + 63) / 64, "a fresh session is not empty");

    // destination rows: inside layer 0, one per block, slot-major
    std::set<uint64_t> rows_seen;
    for (uint64_t s = 0; s < n_local; ++s)
      for (uint64_t b = 0; b < n_blocks; ++b) {
        const uint64_t r = p.dest_row(first_slot + s, b);
        CHECK(r == p.coff[0] + s * n_blocks + b && r < n_local * n_blocks && r < p.rows, "row of (%llu, %llu) is %llu", (unsigned long long)s,
              (unsigned long long)b, (unsigned long long)r);
        rows_seen.insert(r);
      }
    CHECK(rows_seen.size() == p.total(), "destination rows collide");

    // ---- calls until the session is full, with mismatches, repeats and failing files on the way -----------------------------------------
    std::set<Pair> present;                                         // the restatement of the bitmap
    for (int call = 0; call < 60 && present.size() < p.total(); ++call) {
      const size_t n = (size_t)pick(0, 2 * n_blocks + 3);
      std::vector<uint64_t> sb(2 * n + 2);
      std::vector<uint32_t> verdict(n + 1), status(n + 1, 77);
      for (size_t i = 0; i < n; ++i) {
        sb[2 * i] = first_slot + pick(0, n_local - 1);
        sb[2 * i + 1] = pick(0, n_blocks - 1);
        verdict[i] = pick(0, 4) == 0 ? 1 : 0;                       // the device's word: 0 proved
      }
      CHECK(p.validate(sb.data(), n, &err), "a valid call is refused: %s", err.c_str());
      // one request broken at a random index: named, and the lowest of two
      if (n) {
        const size_t bad = (size_t)pick(0, n - 1);
        std::vector<uint64_t> t(sb);
        const int how = (int)pick(0, 2);
        if (how == 0) t[2 * bad] = first_slot + n_local + pick(0, 3);
        else if (how == 1 && first_slot > 0) t[2 * bad] = first_slot - 1;
        else t[2 * bad + 1] = n_blocks + pick(0, 3);
        if (bad + 1 < n) t[2 * (n - 1) + 1] = n_blocks;             // a later one too
        CHECK(!p.validate(t.data(), n, &err) && err.find("request " + std::to_string(bad) + ":") != std::string::npos, "request %zu not named: %s", bad,
              err.c_str());
      }
      std::vector<uint64_t> local_block, dest;
      p.device_requests(sb.data(), n, &local_block, &dest);
      CHECK(local_block.size() == 2 * n && dest.size() == n, "device arrays of the wrong size");
      for (size_t i = 0; i < n; ++i)
        CHECK(local_block[2 * i] == sb[2 * i] - first_slot && local_block[2 * i] < n_local && local_block[2 * i + 1] == sb[2 * i + 1] &&
              dest[i] == p.dest_row(sb[2 * i], sb[2 * i + 1]), "device request %zu", i);

      const FillPlan before = p;
      p.resolve(sb.data(), verdict.data(), n, status.data());
      CHECK(p.bits == before.bits && p.n_present == before.n_present, "resolve changed the session");
      CHECK(status[n] == 77, "resolve wrote past its n");
      std::set<Pair> in_call;
      for (size_t i = 0; i < n; ++i) {                              // in index order: the first proved one of an absent block is NEW
        const Pair q(sb[2 * i], sb[2 * i + 1]);
        uint32_t w = FILL_MISMATCH;
        if (verdict[i] == 0) {
          w = present.count(q) || in_call.count(q) ? FILL_DUPLICATE : FILL_NEW;
          in_call.insert(q);
        }
        CHECK(status[i] == w, "request %zu of (%llu, %llu): status %u, want %u", i, (unsigned long long)q.first, (unsigned long long)q.second, status[i], w);
      }

      // the writer: files in ascending slot order, the first failing one and every later one FAILED
      std::vector<uint32_t> mask = FillPlan::write_mask(status.data(), n);
      for (size_t i = 0; i < n; ++i) CHECK(mask[i] == (status[i] == FILL_NEW ? FILL_WRITE : FILL_SKIP), "write mask of request %zu", i);
      const bool fails = pick(0, 3) == 0;
      const uint64_t failing_slot = first_slot + pick(0, n_local - 1);
      if (fails)
        for (size_t i = 0; i < n; ++i)
          if (mask[i] == FILL_WRITE && sb[2 * i] >= failing_slot) mask[i] = FILL_WRITE_FAILED;
      const std::vector<uint32_t> resolved(status);
      FillPlan::roll_back(sb.data(), mask, status.data());
      std::set<Pair> failed;
      for (size_t i = 0; i < n; ++i)
        if (mask[i] == FILL_WRITE_FAILED) failed.insert(Pair(sb[2 * i], sb[2 * i + 1]));
      size_t want_new = 0;
      for (size_t i = 0; i < n; ++i) {
        const Pair q(sb[2 * i], sb[2 * i + 1]);
        if (mask[i] == FILL_WRITE_FAILED) CHECK(status[i] == FILL_UNWRITTEN, "request %zu is not UNWRITTEN after its file failed", i);
        // a DUPLICATE of a block that failed in this call is UNWRITTEN too; every other status is as resolved
        if (resolved[i] == FILL_DUPLICATE) CHECK(status[i] == (failed.count(q) ? FILL_UNWRITTEN : FILL_DUPLICATE), "duplicate %zu after the roll-back: %u", i, status[i]);
        if (resolved[i] == FILL_MISMATCH || (resolved[i] == FILL_NEW && mask[i] == FILL_WRITE)) CHECK(status[i] == resolved[i], "the roll-back changed request %zu", i);
        if (status[i] == FILL_NEW) {
          CHECK(!present.count(q), "request %zu is NEW for a block that is present", i);
          present.insert(q);
          ++want_new;
        }
      }
      const size_t got_new = p.commit(sb.data(), status.data(), n);
      CHECK(got_new == want_new && p.n_present == present.size(), "commit set %zu bits, want %zu", got_new, want_new);
      for (size_t i = 0; i < n; ++i)
        if (status[i] == FILL_UNWRITTEN) CHECK(!p.present(sb[2 * i] - first_slot, sb[2 * i + 1]) || present.count(Pair(sb[2 * i], sb[2 * i + 1])),
                                               "an UNWRITTEN block became present");

      // the bitmap and the ordered missing list
      std::vector<Pair> absent;
      for (uint64_t s = 0; s < n_local; ++s)
        for (uint64_t b = 0; b < n_blocks; ++b) {
          const bool in = present.count(Pair(first_slot + s, b)) != 0;
          CHECK(p.present(s, b) == in, "bit of (%llu, %llu)", (unsigned long long)s, (unsigned long long)b);
          if (!in) absent.push_back(Pair(first_slot + s, b));
        }
      CHECK(p.missing(nullptr, 0) == absent.size() && p.n_missing() == absent.size(), "the counting form says %llu, want %zu",
            (unsigned long long)p.missing(nullptr, 0), absent.size());
      for (size_t cap : {(size_t)1, absent.size() / 2 + 1, absent.size(), absent.size() + 3}) {
        std::vector<uint64_t> out(2 * cap + 2, 0xabababababababULL);
        CHECK(p.missing(out.data(), cap) == absent.size(), "missing() with cap %zu returns another count", cap);
        const size_t k = std::min(cap, absent.size());
        for (size_t i = 0; i < k; ++i)
          CHECK(out[2 * i] == absent[i].first && out[2 * i + 1] == absent[i].second, "missing[%zu] with cap %zu", i, cap);
        for (size_t i = 2 * k; i < out.size(); ++i) CHECK(out[i] == 0xabababababababULL, "missing() wrote past min(cap, n_missing)");
      }

      // the finish precondition
      const bool ok = p.may_finish(&err);
      CHECK(ok == absent.empty(), "may_finish says %d with %zu missing", (int)ok, absent.size());
      if (!absent.empty())
        CHECK(err.find(std::to_string(absent.size()) + " block(s)") != std::string::npos &&
              err.find("(slot " + std::to_string(absent[0].first) + ", block " + std::to_string(absent[0].second) + ")") != std::string::npos,
              "the refusal does not name the count and the first pair: %s", err.c_str());
    }
    // whatever is left arrives in one call; then the session finishes once and refuses everything after
    std::vector<uint64_t> rest(2 * (size_t)p.n_missing() + 2);
    const size_t n_rest = (size_t)p.missing(rest.data(), (size_t)p.n_missing());
    std::vector<uint32_t> verdict(n_rest + 1, 0), status(n_rest + 1);
    p.resolve(rest.data(), verdict.data(), n_rest, status.data());
    for (size_t i = 0; i < n_rest; ++i) CHECK(status[i] == FILL_NEW, "a missing block is not NEW");
    CHECK(p.commit(rest.data(), status.data(), n_rest) == n_rest && p.n_missing() == 0 && p.may_finish(&err), "the session does not fill up");
    CHECK(p.commit(rest.data(), status.data(), n_rest) == 0, "a bit was set twice");
    p.finished = true;
    CHECK(!p.may_finish(&err) && err.find("finished") != std::string::npos, "a finished session may finish again");
    CHECK(!p.validate(rest.data(), 0, &err) && !p.validate(rest.data(), n_rest, &err) && err.find("finished") != std::string::npos,
          "a finished session takes requests");
  }
  std::printf("fill plan ok: %d rounds, %d failures\n", rounds, failures);
  return failures ? 1 : 0;
}
