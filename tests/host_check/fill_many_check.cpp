// Host check of csrc/fill_many_plan.hpp (cp2_fills_add_many) for tests/test_fill_many_cpu.py: a stand-alone program, built there with
// -fsanitize=address,undefined.  It reads a scenario (tests/fill_many_models.py: scenario_text) from the file named on its command line --
// sessions of several shapes on FillPlans of their own, then calls, each with its `fills`, its interleaved requests and the verdict label of
// every request -- runs the plan exactly as csrc/fill_many.cpp does (listed twice, group, validate, tables, the per-chunk maxima, apply
// per session with a writer that fails where the scenario says a file cannot be written) and prints the grouping, the tables, every
// session's statuses, presence, known rows and n_new, and every refusal with its index.  The Python side compares the output line by
// line with its model, which composes tests/fill_session_model.py per session.  No HIP, no device.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "fill_many_plan.hpp"

using namespace cp2i;

namespace {

struct Sess {
  FillPlan plan;
  bool files = false;
};

void print_states(const std::vector<std::unique_ptr<Sess>>& s) {
  for (size_t j = 0; j < s.size(); ++j) {
    const FillPlan& p = s[j]->plan;
    std::string bits, known;
    for (uint64_t l = 0; l < p.n_local; ++l)
      for (uint64_t b = 0; b < p.n_blocks; ++b) bits += p.present(l, b) ? '1' : '0';
    for (uint64_t r = 0; r < p.rows; ++r)
      if (p.is_known(r)) known += (known.empty() ? "" : " ") + std::to_string(r);
    std::printf("state %zu: keeps %d finished %d present %s known %s\n", j, (int)p.keeps_nodes, (int)p.finished, bits.c_str(),
                known.empty() ? "-" : known.c_str());
  }
}

template <class T>
std::string joined(const std::vector<T>& v) {
  std::string s;
  for (const T& x : v) s += (s.empty() ? "" : " ") + std::to_string(x);
  return s.empty() ? "-" : s;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  size_t n_sessions = 0, n_steps = 0;
  if (!(in >> n_sessions >> n_steps)) return 2;
  std::vector<std::unique_ptr<Sess>> sess;
  for (size_t j = 0; j < n_sessions; ++j) {
    uint64_t nb, first, n_local;
    int keep, files;
    in >> nb >> first >> n_local >> keep >> files;
    sess.emplace_back(new Sess());
    sess.back()->plan.init(first, n_local, nb);
    sess.back()->files = files != 0;
    if (keep) {
      sess.back()->plan.derive_from_presence();
      sess.back()->plan.keeps_nodes = true;
    }
  }
  print_states(sess);
  for (size_t step = 0; step < n_steps; ++step) {
    int kind = 0;
    in >> kind;
    if (kind == 1 || kind == 2) {
      size_t j = 0;
      in >> j;
      FillPlan& p = sess[j]->plan;
      if (kind == 1 && !p.keeps_nodes) {                 // cp2_fill_keep_nodes' host side
        p.derive_from_presence();
        p.keeps_nodes = true;
      }
      if (kind == 2) p.finished = true;
      std::printf("%s %zu\n", kind == 1 ? "keep" : "finish", j);
      print_states(sess);
      continue;
    }
    size_t n_fills = 0, n = 0;
    int have_levels = 0, have_paths = 0;
    in >> n_fills >> n >> have_levels >> have_paths;
    std::vector<size_t> which(n_fills);
    std::vector<long long> fail(n_fills);
    for (size_t k = 0; k < n_fills; ++k) in >> which[k] >> fail[k];
    std::vector<uint64_t> req(3 * n);
    std::vector<uint32_t> levels(n), label(n);
    for (size_t i = 0; i < n; ++i) in >> req[3 * i] >> req[3 * i + 1] >> req[3 * i + 2] >> levels[i] >> label[i];
    if (!in) return 2;
    std::printf("call: %zu session(s), %zu request(s), %s\n", n_fills, n, have_levels ? "levels" : "whole paths");
    // ---- as cp2_fills_add_many: listed twice, group, validate -- and nothing of any session touched by a refusal
    std::vector<const void*> fills(n_fills);
    std::vector<FillManyIn> ins(n_fills);
    for (size_t k = 0; k < n_fills; ++k) {
      fills[k] = sess[which[k]].get();
      ins[k] = {&sess[which[k]]->plan, 0x1000 * (k + 1), 0x100000 * (k + 1), sess[which[k]]->plan.keeps_nodes ? 0x10000000 * (uint64_t)(k + 1) : 0};
    }
    FillManyPlan mp;
    FillManyRefusal why;
    const size_t twice = fill_many_listed_twice(fills.data(), n_fills);
    bool ok = twice == n_fills;
    if (!ok) why = {false, twice, "fills: fills[" + std::to_string(twice) + "] is listed twice"};
    ok = ok && mp.group(req.data(), n, n_fills, &why) && mp.validate(ins.data(), have_levels ? levels.data() : nullptr, have_paths != 0, &why);
    if (!ok) {
      if (why.text.find(std::to_string(why.index)) == std::string::npos) {
        std::printf("the refusal's text does not name its index: %s\n", why.text.c_str());
        return 1;
      }
      std::printf("refused %s %zu\n", why.request ? "request" : "fills", why.index);
      print_states(sess);
      continue;
    }
    mp.tables(ins.data(), req.data());
    for (size_t k = 0; k < n_fills; ++k) {
      std::vector<size_t> g(mp.rows_of(k), mp.rows_of(k) + mp.count(k));
      std::printf("group %zu: %s\n", k, joined(g).c_str());
    }
    for (size_t k = 0; k < n_fills; ++k) {
      const FillManyDesc& d = mp.table[k];
      if (d.tree != ins[k].tree || d.slot_roots != ins[k].slot_roots || d.layer_tab != ins[k].layer_tab || d.reserved != 0) {
        std::printf("descriptor %zu does not carry its session's addresses\n", k);
        return 1;
      }
      std::printf("session %zu: rows %llu local %llu keeps %d blocks %llu depth %u\n", k, (unsigned long long)d.n_rows, (unsigned long long)d.n_local,
                  d.layer_tab != 0, (unsigned long long)d.n_blocks, d.depth);
    }
    for (size_t i = 0; i < n; ++i) {
      const std::string anchor = mp.anchor_row[i] == FillPlan::ANCHOR_SLOT_ROOT ? "root" : std::to_string(mp.anchor_row[i]);
      std::printf("req %zu: session %llu local %llu block %llu level %u off %llu dest %llu anchor %s\n", i, (unsigned long long)mp.session_of[i],
                  (unsigned long long)mp.local_block[2 * i], (unsigned long long)mp.local_block[2 * i + 1], mp.levels[i],
                  (unsigned long long)mp.path_off[i], (unsigned long long)mp.dest[i], anchor.c_str());
    }
    std::printf("paths %llu\n", (unsigned long long)mp.path_off[n]);
    std::vector<size_t> chunks = {1, 3, 64, n ? n : 1};
    std::sort(chunks.begin(), chunks.end());
    chunks.erase(std::unique(chunks.begin(), chunks.end()), chunks.end());
    for (size_t c : chunks) std::printf("chunk %zu: most %llu\n", c, (unsigned long long)mp.most_path_rows(c));
    // ---- the verdicts are the scenario's labels; the writer fails where the scenario says so (repair_write's contract: the failing file's
    // blocks and those of every later file)
    std::vector<uint32_t> status(n, 99);
    std::vector<size_t> n_new(n_fills);
    int result = 0;
    for (size_t k = 0; k < n_fills; ++k) {
      auto write = [&](size_t kk, std::vector<uint32_t>& w) {
        if (fail[kk] < 0) return;
        const uint64_t* sb = mp.pairs_of(kk);
        bool failing = false;
        for (size_t j = 0; j < w.size(); ++j) failing = failing || (w[j] == FILL_WRITE && sb[2 * j] == (uint64_t)fail[kk]);
        if (!failing) return;
        for (size_t j = 0; j < w.size(); ++j)
          if (w[j] == FILL_WRITE && sb[2 * j] >= (uint64_t)fail[kk]) w[j] = FILL_WRITE_FAILED;
        if (result == 0) result = -5;
      };
      n_new[k] = mp.apply(k, sess[which[k]]->plan, label.data(), sess[which[k]]->files, write, status.data());
    }
    for (size_t k = 0; k < n_fills; ++k) {
      std::vector<uint32_t> sub;
      for (size_t j = 0; j < mp.count(k); ++j) sub.push_back(status[mp.rows_of(k)[j]]);
      std::printf("status %zu: %s\n", k, joined(sub).c_str());
    }
    std::printf("result %d: status %s n_new %s\n", result, joined(status).c_str(), joined(n_new).c_str());
    print_states(sess);
  }
  std::printf("fill many ok\n");
  return 0;
}
