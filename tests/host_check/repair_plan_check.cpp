// The block repair's host logic (csrc/repair_plan.hpp, the header repair.cpp and multi_gpu.cpp use) walked over random request sets,
// every answer compared with a direct restatement: validation (range, duplicates, the index named), the kept rows of both layouts, the
// per-file write groups, routing to units and shards, and the stamp rule.  Built with AddressSanitizer + UBSan.  No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "repair_plan.hpp"

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

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 20000;
  std::mt19937_64 rng(12345);
  auto U = [&](uint64_t n) { return n ? rng() % n : 0; };
  size_t n_dup = 0, n_range = 0, n_ok = 0, n_groups = 0, n_restamped = 0;
  for (int r = 0; r < rounds; ++r) {
    const uint64_t first = U(5), n_local = 1 + U(9), cpb = 1ULL << U(5), nblocks = 1 + U(12);
    const size_t n = U(40);
    // ---- validation against a brute-force restatement
    std::vector<uint64_t> sb(2 * n);
    const int kind = (int)U(4);                          // 0: out of range allowed, 1: duplicates allowed, else distinct and in range
    std::set<std::pair<uint64_t, uint64_t>> used;
    for (size_t i = 0; i < n; ++i) {
      sb[2 * i] = first + U(n_local + (kind == 0 && U(8) == 0 ? 2 : 0));
      sb[2 * i + 1] = U(nblocks + (kind == 0 && U(10) == 0 ? 1 : 0));
      if (kind == 1 && i && U(6) == 0) {
        const size_t j = i - 1 - U(i);
        sb[2 * i] = sb[2 * j];
        sb[2 * i + 1] = sb[2 * j + 1];
      }
      if (kind >= 2 && !used.insert({sb[2 * i], sb[2 * i + 1]}).second) {   // (n may exceed the slots x blocks there are: then it repeats)
        if (used.size() >= n_local * nblocks) break;
        --i;
      }
    }
    if (kind == 0 && U(5) == 0 && n) sb[0] = first ? first - 1 : first + n_local;   // below or past the range
    size_t want_bad = n;
    bool want_range = false;
    for (size_t i = 0; i < n && want_bad == n; ++i)
      if (sb[2 * i] < first || sb[2 * i] >= first + n_local || sb[2 * i + 1] >= nblocks) { want_bad = i; want_range = true; }
    if (want_bad == n)
      for (size_t j = 0; j < n && want_bad == n; ++j)
        for (size_t i = 0; i < j; ++i)
          if (sb[2 * i] == sb[2 * j] && sb[2 * i + 1] == sb[2 * j + 1]) { want_bad = j; break; }
    std::string err;
    const bool ok = repair_validate(sb.data(), n, first, n_local, nblocks, &err);
    CHECK(ok == (want_bad == n), "round %d: validate says %d, want bad index %zu", r, (int)ok, want_bad);
    if (!ok) {
      CHECK(err.find("request " + std::to_string(want_bad) + ":") != std::string::npos, "round %d: message '%s' names not request %zu", r, err.c_str(), want_bad);
      if (want_range) ++n_range; else ++n_dup;
      continue;
    }
    ++n_ok;
    // ---- kept rows: every node kept (block trees layer-major over n_local * nblocks blocks, then the big trees) and compact
    const std::vector<uint64_t> b = layers(cpb), t = layers(nblocks);
    uint64_t toff0 = 0;
    for (size_t k = 0; k + 1 < b.size(); ++k) toff0 += n_local * nblocks * b[k];
    std::vector<uint64_t> boff;
    uint64_t off = 0;
    for (size_t k = 0; k < b.size(); ++k) { boff.push_back(off); if (k + 1 < b.size()) off += n_local * nblocks * b[k]; }
    std::set<uint64_t> rows_full, rows_compact;
    for (size_t i = 0; i < n; ++i) {
      const uint64_t local = sb[2 * i] - first, blk = sb[2 * i + 1];
      const uint64_t rf = repair_row_full(boff.back(), b.back(), nblocks, local, blk);
      CHECK(rf == toff0 + local * t[0] + blk, "round %d: full row %llu", r, (unsigned long long)rf);
      const uint64_t rc = repair_row_compact(0, t[0], local, blk);
      CHECK(rc == local * nblocks + blk && rc < n_local * t[0], "round %d: compact row %llu", r, (unsigned long long)rc);
      rows_full.insert(rf);
      rows_compact.insert(rc);
    }
    CHECK(rows_full.size() == n && rows_compact.size() == n, "round %d: two requests share a kept row", r);
    // ---- write groups over a random matched subset
    std::vector<size_t> matched;
    for (size_t i = 0; i < n; ++i)
      if (U(3)) matched.push_back(i);
    const std::vector<WriteGroup> g = repair_write_groups(sb.data(), matched);
    std::map<size_t, int> seen;
    for (size_t k = 0; k < g.size(); ++k) {
      ++n_groups;
      CHECK(!g[k].reqs.empty(), "round %d: empty group", r);
      if (k) CHECK(g[k - 1].slot < g[k].slot, "round %d: groups out of slot order", r);
      for (size_t j = 0; j < g[k].reqs.size(); ++j) {
        const size_t i = g[k].reqs[j];
        ++seen[i];
        CHECK(sb[2 * i] == g[k].slot, "round %d: request %zu in the group of slot %llu", r, i, (unsigned long long)g[k].slot);
        if (j) CHECK(sb[2 * g[k].reqs[j - 1] + 1] < sb[2 * i + 1], "round %d: offsets not ascending in a group", r);
      }
    }
    CHECK(seen.size() == matched.size(), "round %d: %zu of %zu matched requests in a group", r, seen.size(), matched.size());
    for (size_t i : matched) CHECK(seen[i] == 1, "round %d: request %zu in %d groups", r, i, seen[i]);
    // ---- units and shards: every block of every slot lands in exactly one (unit, block of the unit), and in one shard
    const uint64_t S = 1ULL << U(3);
    if (nblocks % S == 0) {
      const uint64_t per = nblocks / S, n_units = n_local * S;
      std::vector<uint64_t> sf, sc;
      for (uint64_t a = 0; a < n_units;) {
        const uint64_t c = 1 + U(n_units - a);
        sf.push_back(a);
        sc.push_back(c);
        a += c;
      }
      std::vector<int> hit(n_units * per, 0);
      for (uint64_t s = 0; s < n_local; ++s)
        for (uint64_t blk = 0; blk < nblocks; ++blk) {
          const UnitBlock u = repair_unit_of(s, blk, S, per);
          CHECK(u.unit / S == s && u.block < per && (u.unit % S) * per + u.block == blk, "round %d: unit of (%llu, %llu)", r, (unsigned long long)s,
                (unsigned long long)blk);
          if (u.unit < n_units && u.block < per) ++hit[u.unit * per + u.block];
          const size_t k = repair_shard_of(sf, sc, u.unit);
          CHECK(k < sf.size() && u.unit >= sf[k] && u.unit < sf[k] + sc[k], "round %d: unit %llu in no shard", r, (unsigned long long)u.unit);
        }
      for (int h : hit) CHECK(h == 1, "round %d: a unit block covered %d times", r, h);
      CHECK(repair_shard_of(sf, sc, n_units) == sf.size(), "round %d: a unit past the end found a shard", r);
    }
    // ---- the stamp rule: items of units_per_slot S2; files written with a stat before and after; stamps that equalled `before`
    const uint64_t S2 = 1 + U(3), first_item = U(4), n_items = 1 + U(12);
    std::vector<uint64_t> stamps(2 * n_items);
    std::vector<FileStamp> written;
    std::map<uint64_t, FileStamp> by_slot;
    for (uint64_t slot = first_item / S2; slot <= (first_item + n_items - 1) / S2 + 1; ++slot) {
      if (U(2)) continue;
      FileStamp f;
      f.slot = slot;
      f.before[0] = 100 + U(3); f.before[1] = 1000 + U(3);
      f.after[0] = f.before[0] + U(2); f.after[1] = f.before[1] + U(3);
      written.push_back(f);
      by_slot[slot] = f;
    }
    for (uint64_t i = 0; i < n_items; ++i) { stamps[2 * i] = 100 + U(3); stamps[2 * i + 1] = 1000 + U(3); }
    const std::vector<uint64_t> old = stamps;
    const std::vector<size_t> changed = repair_restamp(stamps, first_item, S2, written);
    std::set<size_t> ch(changed.begin(), changed.end());
    CHECK(ch.size() == changed.size(), "round %d: an item restamped twice", r);
    for (uint64_t i = 0; i < n_items; ++i) {
      const auto it = by_slot.find((first_item + i) / S2);
      const bool was_valid = it != by_slot.end() && old[2 * i] == it->second.before[0] && old[2 * i + 1] == it->second.before[1];
      const bool moves = was_valid && (it->second.after[0] != old[2 * i] || it->second.after[1] != old[2 * i + 1]);
      CHECK(ch.count(i) == (moves ? 1u : 0u), "round %d: item %llu restamped %d, want %d", r, (unsigned long long)i, (int)ch.count(i), (int)moves);
      if (was_valid) CHECK(stamps[2 * i] == it->second.after[0] && stamps[2 * i + 1] == it->second.after[1], "round %d: item %llu not at the new stat", r,
                           (unsigned long long)i);
      else CHECK(stamps[2 * i] == old[2 * i] && stamps[2 * i + 1] == old[2 * i + 1], "round %d: a stale stamp of item %llu changed", r,
                 (unsigned long long)i);
    }
    n_restamped += changed.size();
  }
  std::printf("repair plan: %d rounds, %zu valid, %zu duplicate and %zu range refusals, %zu write groups, %zu stamps restamped, %d failures\n", rounds,
              n_ok, n_dup, n_range, n_groups, n_restamped, failures);
  if (failures) return 1;
  std::printf("repair plan ok\n");
  return 0;
}
