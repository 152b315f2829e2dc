// csrc/set_roots_plan.hpp on the CPU, under AddressSanitizer + UBSan (tests/test_set_roots_many_cpu.py compiles and drives this): no HIP,
// no device.  It reads one call described as text (tests/set_roots_many_models.py: describe -- "bound B" and "n n_slots ...") and prints
// what the plan makes of it, for the Python model to compare with: per chunk "chunk first count rows R levels L", "trees first:n ..." and
// per level "level k off O cnt C work W trips T entries tree:prefix ...".  On the way every lane of every level is searched
// (set_roots_find) and held against a walk of the table, the sizes against the arithmetic of the layer offsets, and the plan against its
// own guard (set_roots_plan_ok), which must also refuse the plan with one tree grown by a leaf: any disagreement ends the run with 1.
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "set_roots_plan.hpp"

using namespace cp2i;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  uint64_t bound = 0;
  std::vector<uint64_t> n_slots;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream s(line);
    std::string tag;
    s >> tag;
    if (tag == "bound") s >> bound;
    else if (tag == "n") { uint64_t v; while (s >> v) n_slots.push_back(v); }
  }
  size_t next = 0;
  for (const SetRootsChunk& c : set_roots_chunks(n_slots.data(), n_slots.size(), bound)) {
    if (c.first != next || c.count == 0) { std::printf("chunks do not tile the requests\n"); return 1; }
    next = c.first + c.count;
    const std::vector<uint64_t> mine(n_slots.begin() + (long)c.first, n_slots.begin() + (long)next);   // exactly the chunk's: one too many is a sanitizer report
    const SetRootsPlan p = set_roots_plan(mine.data(), mine.size());
    if (p.rows != c.rows || !set_roots_plan_ok(p, p.rows) || set_roots_plan_ok(p, p.rows - 1)) { std::printf("plan refused\n"); return 1; }
    {
      SetRootsPlan q = p;
      q.tree_tab[1] += q.tree_tab[1];                        // the first tree twice as large as planned: it overlaps the next or leaves the buffer
      if (set_roots_plan_ok(q, q.rows)) { std::printf("a grown tree was accepted\n"); return 1; }
    }
    std::printf("chunk %zu %zu rows %" PRIu64 " levels %zu\ntrees", c.first, c.count, c.rows, p.n_levels());
    for (size_t r = 0; r < p.n_trees(); ++r) {
      const uint64_t n = p.tree_tab[2 * r + 1];
      std::printf(" %" PRIu64 ":%" PRIu64, p.tree_tab[2 * r], n);
      uint64_t at = 0;
      for (uint32_t k = 0; k <= set_roots_levels(n); ++k) {
        if (set_roots_layer_off(n, k) != at || (k && set_roots_layer_size(n, k) != (set_roots_layer_size(n, k - 1) + 1) / 2)) {
          std::printf("\nlayer arithmetic disagrees\n");
          return 1;
        }
        at += set_roots_layer_size(n, k);
      }
      if (at != set_roots_total(n) || set_roots_layer_size(n, set_roots_levels(n)) != 1) { std::printf("\nlayer arithmetic disagrees\n"); return 1; }
    }
    std::printf("\n");
    for (size_t k = 0; k < p.n_levels(); ++k) {
      const uint64_t off = p.level_off[k], cnt = p.level_cnt[k];
      std::printf("level %zu off %" PRIu64 " cnt %" PRIu64 " work %" PRIu64 " trips %u entries", k, off, cnt, p.level_work[k], set_roots_trips(cnt));
      for (uint64_t a = 0; a < cnt; ++a) std::printf(" %u:%" PRIu64, p.tree_of[off + a], p.prefix[off + a]);
      std::printf("\n");
      const std::vector<uint64_t> pre(p.prefix.begin() + (long)off, p.prefix.begin() + (long)(off + cnt));   // the level's own entries only
      uint64_t e = 0;
      for (uint64_t t = 0; t < p.level_work[k]; ++t) {
        while (pre[e] <= t) ++e;
        if (set_roots_find(pre.data(), cnt, t) != e) { std::printf("find disagrees\n"); return 1; }
      }
    }
  }
  if (next != n_slots.size()) { std::printf("chunks do not tile the requests\n"); return 1; }
  return 0;
}
