// The host side of cp2_datasets_set_roots_many (csrc/set_roots_many.cpp): how the dataset trees of one call become work for
// k_compress_layer_ragged.  The requests go in CHUNKS of consecutive requests whose trees fit a byte bound; a chunk's trees lie
// tree-major in one buffer of 32-byte rows, tree r owning set_roots_total(n_r) consecutive rows from first_row[r], its layers bottom first
// (what cp2_dataset::dlayers holds); every LEVEL k of the chunk is one launch over the trees that still have a layer k + 1, found by a
// lane through the level's prefix table.  Pure arithmetic over offsets -- no HIP in here: tests/host_check/set_roots_plan_check.cpp runs it
// on the CPU under AddressSanitizer + UBSan and tests/set_roots_many_models.py restates it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cp2i {

// layer k of a tree over n >= 1 leaves holds ceil(n / 2^k) rows (k = 0: n), and the tree has set_roots_levels(n) layers above the leaves:
// layer_sizes_of's rule, the bottom layer compressed once even for a singleton (sizes 1, 1)
inline uint64_t set_roots_layer_size(uint64_t n, uint32_t k) { return k >= 64 ? 1 : ((n - 1) >> k) + 1; }
inline uint32_t set_roots_levels(uint64_t n) {
  uint32_t d = 1;
  while (set_roots_layer_size(n, d) > 1) ++d;
  return d;
}
// row of layer k inside the tree, and the rows of the whole tree (cp2_merkle_total)
inline uint64_t set_roots_layer_off(uint64_t n, uint32_t k) {
  uint64_t off = 0;
  for (uint32_t i = 0; i < k; ++i) off += set_roots_layer_size(n, i);
  return off;
}
inline uint64_t set_roots_total(uint64_t n) { return set_roots_layer_off(n, set_roots_levels(n) + 1); }

// requests [first, first + count) of the call
struct SetRootsChunk {
  size_t first = 0, count = 0;
  uint64_t rows = 0;            // of all its trees
};

// Consecutive requests while their trees' rows x 32 bytes stay within `bound` bytes; a request larger than that is alone in its chunk.
inline std::vector<SetRootsChunk> set_roots_chunks(const uint64_t* n_slots, size_t n, uint64_t bound) {
  std::vector<SetRootsChunk> out;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t rows = set_roots_total(n_slots[i]);
    if (out.empty() || (out.back().rows + rows) * 32 > bound) out.push_back({i, 0, 0});
    out.back().count += 1;
    out.back().rows += rows;
  }
  return out;
}

// The tables of one chunk.  tree_tab (what the kernel reads): first_row and n of tree r at [2 r], [2 r + 1].  Level k: the trees with a
// layer k + 1, in tree order, are entries [level_off[k], level_off[k] + level_cnt[k]) of `tree_of` (the tree) and of `prefix` (the running
// sum of their layer k + 1 sizes, this tree's included: lane t of the launch belongs to the first entry whose prefix is > t, and is node
// t - (the entry before it, or 0) of that layer); level_work[k] is the last prefix, the lanes of the launch.
struct SetRootsPlan {
  std::vector<uint64_t> tree_tab;
  std::vector<uint64_t> prefix;
  std::vector<uint32_t> tree_of;
  std::vector<uint64_t> level_off, level_cnt, level_work;
  uint64_t rows = 0;
  size_t n_trees() const { return tree_tab.size() / 2; }
  size_t n_levels() const { return level_off.size(); }
};

inline SetRootsPlan set_roots_plan(const uint64_t* n_slots, size_t n) {
  SetRootsPlan p;
  p.tree_tab.resize(2 * n);
  uint32_t levels = 0;
  for (size_t r = 0; r < n; ++r) {
    p.tree_tab[2 * r] = p.rows;
    p.tree_tab[2 * r + 1] = n_slots[r];
    p.rows += set_roots_total(n_slots[r]);
    levels = levels < set_roots_levels(n_slots[r]) ? set_roots_levels(n_slots[r]) : levels;
  }
  for (uint32_t k = 0; k < levels; ++k) {
    p.level_off.push_back(p.prefix.size());
    uint64_t sum = 0;
    for (size_t r = 0; r < n; ++r) {
      if (set_roots_levels(n_slots[r]) <= k) continue;
      sum += set_roots_layer_size(n_slots[r], k + 1);
      p.prefix.push_back(sum);
      p.tree_of.push_back((uint32_t)r);
    }
    p.level_cnt.push_back(p.prefix.size() - p.level_off.back());
    p.level_work.push_back(sum);
  }
  return p;
}

// steps of the kernel's search over cnt entries: the smallest s with 2^s >= cnt
inline uint32_t set_roots_trips(uint64_t cnt) {
  uint32_t s = 0;
  while (s < 63 && ((uint64_t)1 << s) < cnt) ++s;
  return s;
}

// The kernel's search, as the host runs it: the entry of lane t < prefix[cnt - 1], in set_roots_trips(cnt) steps whatever t is.
inline uint32_t set_roots_find(const uint64_t* prefix, uint64_t cnt, uint64_t t) {
  uint32_t lo = 0;
  for (uint32_t s = set_roots_trips(cnt); s-- > 0;) {
    const uint64_t mid = (uint64_t)lo + ((uint64_t)1 << s);
    if (mid < cnt && prefix[mid - 1] <= t) lo = (uint32_t)mid;
  }
  return lo;
}

// Whether tables describe what the kernel may run on a buffer of `rows` rows: every tree inside it, no two overlapping, every level's
// entries ascending trees that have that level with the prefix the rule gives.  The guard in front of the launches.
inline bool set_roots_plan_ok(const SetRootsPlan& p, uint64_t rows) {
  const size_t n = p.n_trees();
  if (p.tree_of.size() != p.prefix.size() || p.level_cnt.size() != p.n_levels() || p.level_work.size() != p.n_levels()) return false;
  uint64_t at = 0;
  for (size_t r = 0; r < n; ++r) {
    const uint64_t first = p.tree_tab[2 * r], m = p.tree_tab[2 * r + 1];
    if (m == 0 || m > ((uint64_t)1 << 40) || first < at || first > rows || set_roots_total(m) > rows - first) return false;
    at = first + set_roots_total(m);
  }
  for (size_t k = 0; k < p.n_levels(); ++k) {
    const uint64_t off = p.level_off[k], cnt = p.level_cnt[k];
    if (off > p.prefix.size() || cnt > p.prefix.size() - off || cnt > 0xffffffffull) return false;
    uint64_t sum = 0;
    for (uint64_t a = 0; a < cnt; ++a) {
      const uint32_t r = p.tree_of[off + a];
      if (r >= n || (a && r <= p.tree_of[off + a - 1]) || set_roots_levels(p.tree_tab[2 * r + 1]) <= k) return false;
      sum += set_roots_layer_size(p.tree_tab[2 * r + 1], (uint32_t)k + 1);
      if (p.prefix[off + a] != sum) return false;
    }
    if (p.level_work[k] != sum) return false;
  }
  return true;
}

}  // namespace cp2i
