// A whole fill session replayed on the product's own host plans (csrc/fill_plan.hpp, adopt_plan.hpp, block_proof_plan.hpp,
// fill_checkpoint.hpp), in the order csrc/fill.cpp calls them, from a list of operations in a file: tests/test_fill_session_model_cpu.py
// writes the list from tests/fill_session_model.py's generator and compares what this prints, line by line, with the model.
//
// What the device and the file system decide is input here, derived by the test from the model's labels, exactly as adopt_plan_check.cpp
// stands in for compression: per add request whether its walk matches, per call the slot whose file cannot be written, per resume and
// adopt how many whole blocks each slot file covers and whether each block on disk is the true one ('T'), another ('D') or not covered ('-').
// Compression is the injective stand-in of adopt_plan_check.cpp.
//
//   init <first> <n_local> <n_blocks> <files 0|1>
//   add <n> <fail_slot|-1> n x (<slot> <block> <bad 0|1>)        anchored <n> <fail_slot|-1> n x (<slot> <block> <level> <bad 0|1>)
//   keep | save | finish | nop                                  resume <trust 0|1> <whole blocks per local slot ...> <labels>
//   anchors <n> n x (<slot> <block>) | proofs <n> ... | missing <cap>
//   adopt <s0> <ns> <no_read 0|1> <whole blocks per local slot ...> <labels>
//
// After every operation: "R <status> <results ...>", then the presence bits (P), the known rows (K), the remembered candidates (H), the
// anchor and the proof status of every pair (A, S) and "F <keeps nodes> <finished>".  Built with AddressSanitizer + UBSan.  No GPU.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "adopt_plan.hpp"
#include "block_proof_plan.hpp"
#include "fill_checkpoint.hpp"
#include "fill_plan.hpp"

using namespace cp2i;

typedef uint64_t V;
static std::map<std::tuple<V, V, uint32_t>, V> interned;
static V next_value = 1;
static V fresh() { return next_value++; }
static V compress(const V& l, const V& r, uint32_t key) {
  auto it = interned.find(std::make_tuple(l, r, key));
  if (it != interned.end()) return it->second;
  const V v = fresh();
  interned[std::make_tuple(l, r, key)] = v;
  return v;
}

struct Replay {
  FillPlan plan;
  bool files = true;
  std::vector<V> truth, roots;
  std::vector<uint64_t> have, saved;                    // adopt_have; the bitmap of the last checkpoint
  std::vector<V> adopt_roots;                           // per global block: the candidate root a reading adopt kept
  bool has_saved = false;

  void init(uint64_t first, uint64_t n_local, uint64_t nb, bool from_file) {
    files = from_file;
    plan.init(first, n_local, nb);
    truth.assign(plan.rows, 0);
    for (uint64_t s = 0; s < n_local; ++s) {
      for (uint64_t b = 0; b < nb; ++b) truth[plan.node_row(0, s, b)] = fresh();
      for (size_t l = 0; l < plan.depth(); ++l)
        for (uint64_t j = 0; j < plan.csizes[l + 1]; ++j) {
          const bool pair = 2 * j + 1 < plan.csizes[l];
          truth[plan.node_row(l + 1, s, j)] =
              compress(truth[plan.node_row(l, s, 2 * j)], pair ? truth[plan.node_row(l, s, 2 * j + 1)] : 0, (l == 0 ? 1 : 0) + (pair ? 0 : 2));
        }
    }
    roots.resize(n_local);
    for (uint64_t s = 0; s < n_local; ++s) roots[s] = truth[plan.node_row(plan.depth(), s, 0)];
    adopt_roots.assign(plan.total(), 0);
    have.assign(plan.bits.size(), 0);
  }

  // the writer's stand-in (repair_write): files in ascending slot order, the first that fails stops the writing
  int write(const uint64_t* sb, std::vector<uint32_t>* w, int64_t fail_slot) {
    std::vector<size_t> todo;
    for (size_t i = 0; i < w->size(); ++i)
      if ((*w)[i] == FILL_WRITE) todo.push_back(i);
    bool failed = false;
    for (const WriteGroup& g : repair_write_groups(sb, todo)) {
      if (fail_slot >= 0 && g.slot == (uint64_t)fail_slot) failed = true;
      if (failed)
        for (size_t i : g.reqs) (*w)[i] = FILL_WRITE_FAILED;
    }
    return failed ? -5 : 0;
  }

  // fill_add_checked after the device has spoken
  void settle(const std::vector<uint64_t>& sb, const std::vector<uint32_t>& verdict, int64_t fail_slot) {
    const size_t n = verdict.size();
    std::vector<uint32_t> st(n);
    plan.resolve(sb.data(), verdict.data(), n, st.data());
    int r = 0;
    if (files) {
      std::vector<uint32_t> w = FillPlan::write_mask(st.data(), n);
      r = write(sb.data(), &w, fail_slot);
      FillPlan::roll_back(sb.data(), w, st.data());
    }
    const size_t set = plan.commit(sb.data(), st.data(), n);
    std::printf("R %d", r);
    for (uint32_t s : st) std::printf(" %u", s);
    std::printf(" %zu\n", set);
  }

  void state() const {
    std::string p, k, h, a, s;
    for (uint64_t g = 0; g < plan.total(); ++g) {
      p += plan.present(g / plan.n_blocks, g % plan.n_blocks) ? '1' : '0';
      h += adopt_bit(have, g) ? '1' : '0';
      a += " " + std::to_string(plan.anchor_level(g / plan.n_blocks, g % plan.n_blocks));
      s += " " + std::to_string(plan.proof_status(g / plan.n_blocks, g % plan.n_blocks));
    }
    for (uint64_t r = 0; r < plan.rows; ++r) k += plan.is_known(r) ? '1' : '0';
    std::printf("P %s\nK %s\nH %s\nA%s\nS%s\nF %d %d\n", p.c_str(), k.c_str(), h.c_str(), a.c_str(), s.c_str(), (int)plan.keeps_nodes, (int)plan.finished);
  }
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  Replay R;
  std::string line, err;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string op;
    if (!(ls >> op)) continue;
    FillPlan& plan = R.plan;
    if (op == "init") {
      uint64_t first, n_local, nb;
      int files;
      ls >> first >> n_local >> nb >> files;
      R.init(first, n_local, nb, files != 0);
      continue;
    }
    if (op == "add" || op == "anchored") {
      const bool anchored = op == "anchored";
      size_t n;
      int64_t fail;
      ls >> n >> fail;
      std::vector<uint64_t> sb(2 * n);
      std::vector<uint32_t> levels(n), verdict(n);
      for (size_t i = 0; i < n; ++i) {
        ls >> sb[2 * i] >> sb[2 * i + 1];
        if (anchored) ls >> levels[i];
        ls >> verdict[i];
      }
      if (anchored ? !plan.validate_anchored(sb.data(), levels.data(), n, &err) : !plan.validate(sb.data(), n, &err)) {
        std::printf("R -1\n");
      } else {
        if (anchored) plan.mark_proved_anchored(sb.data(), levels.data(), verdict.data(), n);
        else if (plan.keeps_nodes) plan.mark_proved(sb.data(), verdict.data(), n);
        R.settle(sb, verdict, fail);
      }
    } else if (op == "keep") {                          // cp2_fill_keep_nodes
      if (plan.finished) std::printf("R -1\n");
      else {
        if (!plan.keeps_nodes) {
          plan.derive_from_presence();
          plan.keeps_nodes = true;
        }
        std::printf("R 0\n");
      }
    } else if (op == "save") {                          // cp2_fill_save: the presence bitmap (and layer 0, which no plan reads)
      if (plan.finished) std::printf("R -1\n");
      else {
        R.saved = plan.bits;
        R.has_saved = true;
        std::printf("R 0\n");
      }
    } else if (op == "resume") {                        // cp2_fill_free, cp2_fill_resume
      int trust;
      ls >> trust;
      std::vector<uint64_t> whole(plan.n_local);
      for (uint64_t& x : whole) ls >> x;
      std::string labels;
      ls >> labels;
      if (!R.has_saved || labels.size() != plan.total()) return 3;
      std::vector<uint64_t> bits = R.saved, dropped;
      std::vector<uint8_t> layer0(plan.total() * 32, 1);
      if (!trust && R.files) fill_ckpt_drop_short(whole, plan.n_blocks, &bits, &layer0, &dropped);
      const uint64_t first = plan.first_slot, n_local = plan.n_local, nb = plan.n_blocks;
      plan.init(first, n_local, nb);                    // session_open: a plan of its own, no nodes kept
      R.have.assign(plan.bits.size(), 0);
      if (!plan.restore(bits)) return 3;
      if (!trust && R.files) {                          // recheck_present: the device's verdict per block read
        const FillReadPlan rp = fill_read_plan(plan.bits, plan.total(), plan.n_blocks, 7);
        std::vector<uint64_t> changed;
        for (uint64_t g : rp.g)
          if (labels[g] != 'T') changed.push_back(g);
        (void)plan.drop(changed.data(), changed.size());
        dropped.insert(dropped.end(), changed.begin(), changed.end());
      }
      std::printf("R 0 %zu\n", dropped.size());
    } else if (op == "anchors" || op == "proofs") {
      size_t n;
      ls >> n;
      std::vector<uint64_t> sb(2 * n);
      for (uint64_t& x : sb) ls >> x;
      const bool refused = plan.finished || (op == "proofs" && !plan.keeps_nodes) ||
                           !block_proofs_validate(sb.data(), n, plan.first_slot, plan.n_local, plan.n_blocks, &err);
      if (refused) std::printf("R -1\n");
      else {
        std::printf("R 0");
        for (size_t i = 0; i < n; ++i)
          std::printf(" %u", op == "anchors" ? (uint32_t)plan.anchor_level(sb[2 * i] - plan.first_slot, sb[2 * i + 1])
                                              : plan.proof_status(sb[2 * i] - plan.first_slot, sb[2 * i + 1]));
        std::printf("\n");
      }
    } else if (op == "missing") {
      size_t cap;
      ls >> cap;
      cap = std::min<size_t>(cap, (size_t)plan.total());
      std::vector<uint64_t> out(2 * cap + 2);
      const uint64_t n = plan.missing(out.data(), cap);
      std::printf("R 0 %llu", (unsigned long long)n);
      for (size_t i = 0; i < 2 * std::min<uint64_t>(cap, n); ++i) std::printf(" %llu", (unsigned long long)out[i]);
      std::printf("\n");
    } else if (op == "adopt") {                         // cp2_fill_adopt
      uint64_t s0, ns;
      int no_read;
      ls >> s0 >> ns >> no_read;
      std::vector<uint64_t> whole_all(plan.n_local);
      for (uint64_t& x : whole_all) ls >> x;
      std::string labels;
      ls >> labels;
      if (labels.size() != plan.total()) return 3;
      if (plan.finished || !plan.keeps_nodes || !R.files) std::printf("R -1\n");
      else {
        uint64_t read = 0;
        if (!no_read) {
          const std::vector<uint64_t> whole(whole_all.begin() + (long)s0, whole_all.begin() + (long)(s0 + ns));
          const std::vector<uint64_t> read_bits = adopt_read_bits(plan, s0, ns, whole);
          const FillReadPlan rp = fill_read_plan(read_bits, plan.total(), plan.n_blocks, 5);
          read = rp.g.size();
          for (uint64_t g : rp.g) {
            if (labels[g] == '-') return 4;             // the read set must lie inside what the files cover
            R.adopt_roots[g] = labels[g] == 'T' ? R.truth[g] : fresh();
          }
          adopt_remember(plan, s0, ns, read_bits, &R.have);
        }
        uint64_t n_cand = 0;
        std::vector<uint8_t> flags = adopt_flags(plan, s0, ns, &R.have, &n_cand);
        AdoptVerdict verdict;
        verdict.adopted.resize((size_t)ns);
        if (n_cand) {
          std::vector<V> kept(plan.rows), cand(plan.rows, 0);
          for (uint64_t r = 0; r < plan.rows; ++r) kept[r] = plan.is_known(r) ? R.truth[r] : fresh();
          for (uint64_t g = 0; g < plan.total(); ++g) cand[g] = R.adopt_roots[g];   // (coff[0] == 0: layer 0 comes first)
          adopt_model_layers(plan, s0, ns, kept, R.roots, (V)0, &cand, &flags, compress);
          verdict = adopt_apply(&plan, s0, ns, adopt_model_resolve(plan, s0, ns, kept, cand, flags));
        }
        uint64_t adopted = 0;
        for (uint64_t i = 0; i < ns; ++i) adopted += adopt_commit(&plan, verdict.adopted[(size_t)i]);
        std::printf("R 0 %llu %llu\n", (unsigned long long)read, (unsigned long long)adopted);
      }
    } else if (op == "finish") {                        // cp2_fill_finish
      if (!plan.may_finish(&err)) std::printf("R -1\n");
      else {
        plan.finished = true;
        std::printf("R 0\n");
      }
    } else if (op == "nop") {                           // the sequence touched the files: nothing of the session changes
      std::printf("R 0\n");
    } else {
      return 2;
    }
    R.state();
  }
  return 0;
}
