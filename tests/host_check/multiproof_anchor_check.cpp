// The host side of multiproofs against what a fill session knows (csrc/multiproof_anchor_plan.hpp) on the CPU, with its own main: compiled
// with -fsanitize=address,undefined and run as a process by tests/test_multiproof_anchor_cpu.py, never loaded into Python.  It reads a
// scenario file of commands and prints what the plan makes of each, one line per fact; the test compares the output with the model's
// (tests/multiproof_anchor_models.py) line by line.  A known set is written "<count> <level> <index> ...".
//   want <n_blocks> <k> <blocks...> <known>                          -> "want <level>:<index> ..."
//   plan <n_groups> then per group "<n_blocks> <count> <blocks...> <known>"
//                                                                   -> the table sizes, every level, every job, every row, every top,
//                                                                      top_off and the commit list
//   counts <n_groups> <count...>                                    -> a plan over counts alone (no block list): "refused <text>"
//   places <first> <n_local> <n_blocks> <n> then per place "<slot> <level> <index>"
//                                                                   -> "ok" or "refused <text>"
//   fill <n_blocks> <first> <n_local> <n_calls> then per call "<n_groups>" and per group "<slot> <verdict> <count> <blocks...>"
//                                                                   -> per call, on one FillPlan that keeps nodes: "rows <per group>" (the
//                                                                      want lists against the session as it stands) and the known bitmap
//                                                                      after FillPlan::mark_proved_multi over the commit list, which must
//                                                                      equal, bit for bit, the one mark_proved_anchored leaves over the same
//                                                                      requests at their lowest anchors (anchor_level)
//   validate <first> <n_local> <n_blocks> <n_rows or -1> <n_groups> then per group "<slot> <count>", then "<n> <blocks...>", then per group
//   <known>                                                         -> "ok rows <r>" or "refused <text>": the add's refusals in their order
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "fill_plan.hpp"
#include "multiproof_anchor_plan.hpp"

using namespace cp2i;

using Known = std::set<std::pair<uint64_t, uint64_t>>;

static Known read_known(std::istream& in) {
  size_t k;
  in >> k;
  Known out;
  for (size_t j = 0; j < k; ++j) {
    uint64_t l, i;
    in >> l >> i;
    out.insert({l, i});
  }
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string cmd;
  while (in >> cmd) {
    if (cmd == "want") {
      uint64_t n_blocks;
      size_t k;
      in >> n_blocks >> k;
      std::vector<uint64_t> b(k), li;
      for (auto& x : b) in >> x;
      const Known known = read_known(in);
      const auto fn = [&](size_t l, uint64_t i) { return known.count({l, i}) != 0; };
      const size_t rows = multiproof_want(n_blocks, b.data(), k, fn, &li);
      if (rows != li.size() / 2 || rows != multiproof_want(n_blocks, b.data(), k, fn, nullptr)) return 3;
      std::printf("want");
      for (size_t r = 0; r < rows; ++r) std::printf(" %" PRIu64 ":%" PRIu64, li[2 * r], li[2 * r + 1]);
      std::printf("\n");
    } else if (cmd == "plan") {
      size_t ng;
      in >> ng;
      std::vector<uint64_t> counts(ng), nb(ng), blocks;
      std::vector<Known> known(ng);
      for (size_t g = 0; g < ng; ++g) {
        in >> nb[g] >> counts[g];
        for (uint64_t j = 0; j < counts[g]; ++j) {
          uint64_t b;
          in >> b;
          blocks.push_back(b);
        }
        known[g] = read_known(in);
      }
      MultiproofAnchorPlan p;
      std::string err;
      if (!multiproof_anchor_plan(
              counts.data(), nb.data(), ng, blocks.data(), [&](size_t g, size_t l, uint64_t i) { return known[g].count({l, i}) != 0; }, &p, &err)) {
        std::printf("refused %s\n", err.c_str());
        continue;
      }
      std::printf("plan n %zu n_rows %zu n_kept %zu n_work %zu levels %zu computed %zu tops %zu\n", p.n, p.n_rows, p.n_kept, p.n_work, p.levels(),
                  p.computed(), p.n_tops());
      for (size_t l = 0; l < p.levels(); ++l) {
        std::printf("level %zu base %" PRIu64 " jobs %" PRIu64 "\n", l, p.level_base[l], p.level_off[l + 1] - p.level_off[l]);
        for (uint64_t k = p.level_off[l]; k < p.level_off[l + 1]; ++k)
          std::printf("job %u %u %u %u\n", p.jobs[k].left, p.jobs[k].right, p.jobs[k].key_last, p.jobs[k].group);
      }
      if (p.row_group.size() != p.n_work || p.row_level.size() != p.n_work || p.row_index.size() != p.n_work) return 5;
      for (size_t r = 0; r < p.n_work; ++r) std::printf("row %zu %u %u %" PRIu64 "\n", r, p.row_group[r], p.row_level[r], p.row_index[r]);
      if (p.top_group.size() != p.n_tops() || p.top_level.size() != p.n_tops() || p.top_index.size() != p.n_tops() || p.top_off.size() != ng + 1) return 5;
      for (size_t t = 0; t < p.n_tops(); ++t) std::printf("top %u %u %u %" PRIu64 "\n", p.top_row[t], p.top_group[t], p.top_level[t], p.top_index[t]);
      std::printf("top_off");
      for (uint64_t x : p.top_off) std::printf(" %" PRIu64, x);
      std::printf("\ncommit");
      for (uint32_t r : p.commit) std::printf(" %u", r);
      std::printf("\n");
    } else if (cmd == "counts") {
      size_t ng;
      in >> ng;
      std::vector<uint64_t> counts(ng), nb(ng, 2);
      for (auto& x : counts) in >> x;
      MultiproofAnchorPlan p;
      std::string err;
      if (multiproof_anchor_plan(counts.data(), nb.data(), ng, nullptr, [](size_t, size_t, uint64_t) { return false; }, &p, &err))
        return 6;   // (only refusals come this way: nothing reads a block)
      std::printf("refused %s\n", err.c_str());
    } else if (cmd == "validate") {
      uint64_t first, n_local, n_blocks;
      int64_t n_rows;
      size_t ng, n;
      in >> first >> n_local >> n_blocks >> n_rows >> ng;
      std::vector<uint64_t> groups(2 * ng);
      for (auto& x : groups) in >> x;
      in >> n;
      std::vector<uint64_t> blocks(n);
      for (auto& x : blocks) in >> x;
      std::vector<Known> known(ng);
      for (auto& k : known) k = read_known(in);
      size_t counted = 0;
      if (!multiproof_count(groups.data(), ng, &counted) || counted != n) return 4;
      std::string err;
      uint64_t rows = 0;
      if (multiproof_anchor_validate(
              "fill multi anchored", groups.data(), ng, blocks.data(), first, n_local, n_blocks,
              [&](size_t g, size_t l, uint64_t i) { return known[g].count({l, i}) != 0; }, n_rows >= 0, (uint64_t)n_rows, &rows, nullptr, nullptr, &err))
        std::printf("ok rows %" PRIu64 "\n", rows);
      else
        std::printf("refused %s\n", err.c_str());
    } else if (cmd == "places") {
      uint64_t first, n_local, n_blocks;
      size_t n;
      in >> first >> n_local >> n_blocks >> n;
      std::vector<uint64_t> places(3 * n);
      for (auto& x : places) in >> x;
      FillPlan plan;
      plan.init(first, n_local, n_blocks);
      std::string err;
      if (tree_places_validate("tree rows", places.data(), n, first, n_local, plan.csizes, &err)) std::printf("ok\n");
      else std::printf("refused %s\n", err.c_str());
    } else if (cmd == "fill") {
      uint64_t n_blocks, first, n_local;
      size_t n_calls;
      in >> n_blocks >> first >> n_local >> n_calls;
      FillPlan multi, anchored;
      multi.init(first, n_local, n_blocks);
      anchored.init(first, n_local, n_blocks);
      multi.keeps_nodes = anchored.keeps_nodes = true;
      for (size_t c = 0; c < n_calls; ++c) {
        size_t ng;
        in >> ng;
        std::vector<uint64_t> counts(ng), nb(ng, n_blocks), local(ng), blocks, slot_block;
        std::vector<uint32_t> gv(ng), verdict, levels;
        for (size_t g = 0; g < ng; ++g) {
          uint64_t slot;
          in >> slot >> gv[g] >> counts[g];
          local[g] = slot - first;
          for (uint64_t j = 0; j < counts[g]; ++j) {
            uint64_t b;
            in >> b;
            blocks.push_back(b);
            slot_block.push_back(slot);
            slot_block.push_back(b);
            verdict.push_back(gv[g]);
            levels.push_back((uint32_t)anchored.anchor_level(local[g], b));
          }
        }
        std::printf("rows");
        size_t at = 0;
        for (size_t g = 0; g < ng; ++g) {
          std::printf(" %zu", multiproof_want(
                                  n_blocks, blocks.data() + at, (size_t)counts[g],
                                  [&](size_t l, uint64_t i) { return multi.is_known(multi.node_row(l, local[g], i)); }, nullptr));
          at += (size_t)counts[g];
        }
        std::printf("\n");
        MultiproofAnchorPlan p;
        std::string err;
        if (!multiproof_anchor_plan(
                counts.data(), nb.data(), ng, blocks.data(), [&](size_t g, size_t l, uint64_t i) { return multi.is_known(multi.node_row(l, local[g], i)); },
                &p, &err))
          return 8;
        std::vector<uint32_t> c_group, c_level;
        std::vector<uint64_t> c_index;
        for (uint32_t r : p.commit) {
          if (multi.is_known(multi.node_row(p.row_level[r], local[p.row_group[r]], p.row_index[r]))) return 10;   // a known row is never written
          c_group.push_back(p.row_group[r]);
          c_level.push_back(p.row_level[r]);
          c_index.push_back(p.row_index[r]);
        }
        std::string why;
        if (!anchored.validate_anchored(slot_block.data(), levels.data(), levels.size(), &why)) return 11;
        multi.mark_proved_multi(c_group.data(), c_level.data(), c_index.data(), c_group.size(), local.data(), gv.data());
        anchored.mark_proved_anchored(slot_block.data(), levels.data(), verdict.data(), verdict.size());
        if (multi.known != anchored.known) return 9;
        std::printf("known");
        for (uint64_t w : multi.known) std::printf(" %" PRIx64, w);
        std::printf("\n");
      }
    } else {
      return 7;
    }
  }
  std::printf("multiproof anchor plan ok\n");
  return 0;
}
