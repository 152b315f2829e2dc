// Stand-alone check of csrc/fill_finish_plan.hpp (no HIP, no device): reads a scenario -- a world of sessions in stated states and calls
// that list them -- and prints, per call, the refusal with its index or the tables, a running sum over every lane of every level, the
// verdict index turned back into (fills index, local slot), the text of a mismatch, and the order of saves, objects and hand-overs with a
// failing save injected at every k and a failing allocation in the middle.  tests/test_fill_finish_many_cpu.py builds it with
// AddressSanitizer + UBSan and compares the output line by line with tests/fill_finish_many_models.py.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fill_finish_plan.hpp"

using namespace cp2i;

struct Session {
  FillPlan plan;
  bool other = false;
};

static void commit_line(const char* what, long at, size_t n, const std::vector<int>& has_path, long fail_at, long alloc_fail_at) {
  std::vector<std::string> ev;
  size_t saved = 0;
  const int st = fill_finish_commit(
      n, [&](size_t k) { return has_path[k] != 0; },
      [&](size_t k) {
        ev.push_back("save " + std::to_string(k));
        return (long)k == fail_at ? -5 : 0;
      },
      [&](size_t k) {
        ev.push_back("make " + std::to_string(k));
        return (long)k != alloc_fail_at;
      },
      [&](size_t k) { ev.push_back("hand " + std::to_string(k)); }, -3, &saved);
  std::string line;
  for (size_t i = 0; i < ev.size(); ++i) line += (i ? ", " : "") + ev[i];
  std::printf("commit %s %s status %d saved %zu: %s\n", what, at < 0 ? "none" : std::to_string(at).c_str(), st, saved, line.c_str());
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  std::string line, word;
  std::vector<Session> world;
  std::vector<long> fills;
  std::vector<int> has_path;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    in >> word;
    if (word == "world") {
      size_t n = 0;
      in >> n;
      world.reserve(n);            // (the calls keep addresses of the sessions)
    } else if (word == "session") {
      uint64_t n = 0, nl = 0, first = 0;
      std::string state;
      in >> n >> nl >> first >> state;
      world.emplace_back();
      Session& s = world.back();
      s.plan.init(first, nl, n);
      for (uint64_t g = 0; g < n * nl; ++g) s.plan.bits[(size_t)(g >> 6)] |= (uint64_t)1 << (g & 63);
      s.plan.n_present = n * nl;
      s.other = state == "other";
      s.plan.finished = state == "finished";
      uint64_t g = 0;
      while (state == "missing" && in >> g) {
        s.plan.bits[(size_t)(g >> 6)] &= ~((uint64_t)1 << (g & 63));
        --s.plan.n_present;
      }
    } else if (word == "call") {
      size_t m = 0;
      in >> m;
      fills.assign(m, -1);
      for (size_t k = 0; k < m; ++k) in >> fills[k];
    } else if (word == "paths") {
      has_path.assign(fills.size(), 0);
      for (size_t k = 0; k < fills.size(); ++k) in >> has_path[k];
    } else if (word == "bad") {
      size_t nb = 0;
      in >> nb;
      std::vector<uint64_t> bad(nb);
      for (size_t i = 0; i < nb; ++i) in >> bad[i];
      const size_t n = fills.size();
      std::vector<const void*> ptrs(n);
      std::vector<FillFinishIn> fin(n);
      for (size_t k = 0; k < n; ++k) {
        if (fills[k] < 0) continue;
        Session& s = world[(size_t)fills[k]];
        ptrs[k] = &s;
        fin[k] = {&s.plan, !s.other, 0x1000 * (uint64_t)(fills[k] + 1), 0x100 * (uint64_t)(fills[k] + 1)};
      }
      FillFinishRefusal why;
      if (!fill_finish_check(ptrs.data(), fin.data(), n, &why)) {
        std::printf("refused %zu %s\n", why.index, why.text.c_str());
        continue;
      }
      FillFinishPlan p;
      p.tables(fin.data(), n);
      std::printf("voff");
      for (uint64_t v : p.voff) std::printf(" %llu", (unsigned long long)v);
      std::printf("\n");
      for (size_t l = 0; l < p.n_levels(); ++l) {
        std::printf("level %zu off %llu cnt %llu work %llu trips %u entries", l, (unsigned long long)p.level_off[l], (unsigned long long)p.level_cnt[l],
                    (unsigned long long)p.level_work[l], FillFinishPlan::trips(p.level_cnt[l]));
        for (uint64_t a = p.level_off[l]; a < p.level_off[l] + p.level_cnt[l]; ++a)
          std::printf(" %u:%llu", p.sess_of[a], (unsigned long long)p.prefix[a]);
        std::printf("\n");
      }
      std::printf("rows_built %llu launches %zu\n", (unsigned long long)p.rows_built, p.launches);
      for (size_t k = 0; k < n; ++k) {                 // the descriptors say what the sessions are
        const FillManyDesc& d = p.table[k];
        const FillPlan& sp = *fin[k].plan;
        if (d.tree != fin[k].tree || d.slot_roots != fin[k].slot_roots || d.n_rows != sp.rows || d.n_local != sp.n_local || d.n_blocks != sp.n_blocks ||
            d.depth != sp.depth() || d.layer_tab != 0 || d.reserved != 0) {
          std::printf("descriptor %zu is wrong\n", k);
          return 1;
        }
      }
      for (size_t l = 0; l < p.n_levels(); ++l) {
        uint64_t acc = 0;
        for (uint64_t t = 0; t < p.level_work[l]; ++t) {
          const FillFinishPlan::Lane x = p.lane(l, t);
          const FillPlan& sp = *fin[x.session].plan;   // the closed form against the session's own layout
          if (x.src != sp.coff[l] + x.slot * sp.csizes[l] + 2 * x.node || x.dst != sp.coff[l + 1] + x.slot * sp.csizes[l + 1] + x.node || x.dst >= sp.rows) {
            std::printf("level %zu lane %llu: rows off the session's layout\n", l, (unsigned long long)t);
            return 1;
          }
          const unsigned __int128 next = (unsigned __int128)acc * 1000003u + x.session * 7ull + x.slot * 11 + x.node * 13 + x.src * 17 + x.dst * 19 +
                                         (x.pair ? 23 : 0) + (x.last ? 29 : 0);
          acc = (uint64_t)(next % ((unsigned __int128)1 << 61));
        }
        std::printf("lanes %zu count %llu sum %llu\n", l, (unsigned long long)p.level_work[l], (unsigned long long)acc);
      }
      std::printf("where");
      for (uint64_t v = 0; v < p.n_verdicts(); ++v) {
        size_t k = 0;
        uint64_t local = 0;
        p.where(v, &k, &local);
        std::printf(" %zu:%llu", k, (unsigned long long)local);
      }
      std::printf("\n");
      std::vector<uint32_t> verdict((size_t)p.n_verdicts(), 0);
      for (uint64_t v : bad) verdict[(size_t)v] = 1 + (uint32_t)(v % 3);
      if (p.first_mismatch(verdict.data(), fin.data(), &why)) std::printf("mismatch %zu %s\n", why.index, why.text.c_str());
      std::fill(verdict.begin(), verdict.end(), 0u);
      std::printf("clean %s\n", p.first_mismatch(verdict.data(), fin.data(), &why) ? "mismatch" : "none");
      for (long k = 0; k <= (long)n; ++k) commit_line("fail", k < (long)n ? k : -1, n, has_path, k < (long)n ? k : -1, -1);
      commit_line("alloc", (long)(n / 2), n, has_path, -1, (long)(n / 2));
    }
  }
  std::printf("fill finish many ok\n");
  return 0;
}
