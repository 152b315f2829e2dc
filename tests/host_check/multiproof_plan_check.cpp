// The host side of block multiproofs (csrc/multiproof_plan.hpp) on the CPU, with its own main: compiled with -fsanitize=address,undefined
// and run as a process by tests/test_multiproof_cpu.py, never loaded into Python.  It reads a scenario file of commands and prints what
// the plan makes of each, one line per fact; the test compares the output with the model's (tests/multiproof_models.py) line by line.
//   layout <n_blocks> <k> <blocks...>                               -> "layout <level>:<index> ..."
//   validate <call> <what> <first> <n_local> <n_blocks> <n_rows or -1> <n_groups> then per group "<slot> <count>", then "<n> <blocks...>"
//                                                                   -> "ok rows <r>" or "refused <text>"
//   plan <n_groups> then per group "<n_blocks> <count> <blocks...>" -> the table sizes, every level, every job, every row
//   counts <n_groups> <count...>                                    -> a plan over counts alone (no block list): "refused <text>"
//   fit <rows> <more>                                               -> "fit 0" or "fit 1"
//   mark <n_blocks> <first_slot> <n_local> <n_groups> then per group "<slot> <verdict> <count> <blocks...>"
//                                                                   -> the commit list of a session that keeps nodes ("commit <work row>
//                                                                      <row of the compact layout> <group>") and the known bitmap after
//                                                                      FillPlan::mark_proved_multi, which must equal, bit for bit, the one
//                                                                      FillPlan::mark_proved leaves over the same blocks with whole paths
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "fill_plan.hpp"
#include "multiproof_plan.hpp"

using namespace cp2i;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string cmd;
  while (in >> cmd) {
    if (cmd == "layout") {
      uint64_t n_blocks;
      size_t k;
      in >> n_blocks >> k;
      std::vector<uint64_t> b(k), li;
      for (auto& x : b) in >> x;
      if (!multiproof_list_ok(n_blocks, b.data(), k)) {
        std::printf("layout refused\n");
        continue;
      }
      const size_t rows = multiproof_layout(n_blocks, b.data(), k, &li);
      if (rows != li.size() / 2 || rows != multiproof_layout(n_blocks, b.data(), k, nullptr)) return 3;
      std::printf("layout");
      for (size_t r = 0; r < rows; ++r) std::printf(" %" PRIu64 ":%" PRIu64, li[2 * r], li[2 * r + 1]);
      std::printf("\n");
    } else if (cmd == "validate") {
      std::string call, what;
      uint64_t first, n_local, n_blocks;
      int64_t n_rows;
      size_t ng, n;
      in >> call >> what >> first >> n_local >> n_blocks >> n_rows >> ng;
      std::vector<uint64_t> groups(2 * ng);
      for (auto& x : groups) in >> x;
      in >> n;
      std::vector<uint64_t> blocks(n);
      for (auto& x : blocks) in >> x;
      size_t counted = 0;
      if (!multiproof_count(groups.data(), ng, &counted) || counted != n) return 4;
      std::string err;
      uint64_t rows = 0;
      if (multiproof_validate(call.c_str(), what.c_str(), groups.data(), ng, blocks.data(), first, n_local, n_blocks, n_rows >= 0, (uint64_t)n_rows, &rows, &err))
        std::printf("ok rows %" PRIu64 "\n", rows);
      else
        std::printf("refused %s\n", err.c_str());
    } else if (cmd == "plan") {
      size_t ng;
      in >> ng;
      std::vector<uint64_t> counts(ng), nb(ng), blocks;
      for (size_t g = 0; g < ng; ++g) {
        in >> nb[g] >> counts[g];
        for (uint64_t j = 0; j < counts[g]; ++j) {
          uint64_t b;
          in >> b;
          blocks.push_back(b);
        }
      }
      MultiproofPlan p;
      std::string err;
      if (!multiproof_plan(counts.data(), nb.data(), ng, blocks.data(), &p, &err)) {
        std::printf("refused %s\n", err.c_str());
        continue;
      }
      std::printf("plan n %zu n_rows %zu n_work %zu levels %zu computed %zu\n", p.n, p.n_rows, p.n_work, p.levels(), p.computed());
      for (size_t l = 0; l < p.levels(); ++l) {
        std::printf("level %zu base %" PRIu64 " jobs %" PRIu64 "\n", l, p.level_base[l], p.level_off[l + 1] - p.level_off[l]);
        for (uint64_t k = p.level_off[l]; k < p.level_off[l + 1]; ++k)
          std::printf("job %u %u %u %u\n", p.jobs[k].left, p.jobs[k].right, p.jobs[k].key_last, p.jobs[k].group);
      }
      if (p.row_group.size() != p.n_work || p.row_level.size() != p.n_work || p.row_index.size() != p.n_work) return 5;
      for (size_t r = 0; r < p.n_work; ++r) std::printf("row %zu %u %u %" PRIu64 "\n", r, p.row_group[r], p.row_level[r], p.row_index[r]);
    } else if (cmd == "counts") {
      size_t ng;
      in >> ng;
      std::vector<uint64_t> counts(ng), nb(ng, 2);
      for (auto& x : counts) in >> x;
      MultiproofPlan p;
      std::string err;
      if (multiproof_plan(counts.data(), nb.data(), ng, nullptr, &p, &err)) return 6;   // (only refusals come this way: nothing reads a block)
      std::printf("refused %s\n", err.c_str());
    } else if (cmd == "fit") {
      uint64_t rows, more;
      in >> rows >> more;
      std::printf("fit %d\n", multiproof_rows_fit(rows, more) ? 1 : 0);
    } else if (cmd == "mark") {
      uint64_t n_blocks, first, n_local;
      size_t ng;
      in >> n_blocks >> first >> n_local >> ng;
      std::vector<uint64_t> counts(ng), nb(ng, n_blocks), local(ng), blocks, slot_block;
      std::vector<uint32_t> gv(ng), verdict;
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
        }
      }
      MultiproofPlan p;
      std::string err;
      if (!multiproof_plan(counts.data(), nb.data(), ng, blocks.data(), &p, &err)) return 8;
      FillPlan multi, whole;
      multi.init(first, n_local, n_blocks);
      whole.init(first, n_local, n_blocks);
      for (size_t r = 0; r < p.n_work; ++r)
        std::printf("commit %zu %" PRIu64 " %u\n", r, multi.node_row(p.row_level[r], local[p.row_group[r]], p.row_index[r]), p.row_group[r]);
      multi.mark_proved_multi(p.row_group.data(), p.row_level.data(), p.row_index.data(), p.n_work, local.data(), gv.data());
      whole.mark_proved(slot_block.data(), verdict.data(), verdict.size());
      if (multi.known != whole.known) return 9;
      std::printf("known");
      for (uint64_t w : multi.known) std::printf(" %" PRIx64, w);
      std::printf("\n");
    } else {
      return 7;
    }
  }
  std::printf("multiproof plan ok\n");
  return 0;
}
