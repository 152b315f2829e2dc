// csrc/build_many_plan.hpp on the CPU, under AddressSanitizer + UBSan (tests/test_build_many_cpu.py compiles and drives this): no HIP, no
// device.  It reads one call described as text (tests/build_many_models.py: describe) and prints what the plan makes of it, for the
// Python model to compare with:
//   build_many_plan_check plan FILE      "fake ...", then per class "class", "items", "layers" and per batch "batch ... src ..." and
//                                        "table ..." (the address table of that batch; "table refused" when a row leaves its buffer,
//                                        which a "shrink i" line brings about: request i then has one slot fewer than planned)
//   build_many_plan_check refusal n_slots first_slot n_local max_depth max_log2 cell_size block_size n_cells from_file
//                                        "refusal <text>" ("refusal -": nothing to name)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "build_many_plan.hpp"

using namespace cp2i;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string what = argv[1];
  if (what == "refusal") {
    if (argc < 11) return 2;
    uint64_t v[9];
    for (int i = 0; i < 9; ++i) v[i] = (uint64_t)std::strtoll(argv[2 + i], nullptr, 10);
    const std::string r = build_many_refusal(v[0], v[1], v[2], (int)(int64_t)v[3], (int)(int64_t)v[4], v[5], v[6], v[7], v[8] != 0, 16384);
    std::printf("refusal %s\n", r.empty() ? "-" : r.c_str());
    return 0;
  }
  if (what != "plan") return 2;
  std::ifstream in(argv[2]);
  if (!in) return 2;
  size_t stage = 0;
  int mode = 2;
  std::vector<BuildRequest> req;
  std::vector<uint64_t> base;
  std::vector<size_t> shrink;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream s(line);
    std::string tag;
    s >> tag;
    if (tag == "stage") s >> stage;
    else if (tag == "mode") s >> mode;
    else if (tag == "shrink") { size_t i; s >> i; shrink.push_back(i); }
    else if (tag == "R") {
      BuildRequest r;
      int from_file;
      uint64_t b;
      s >> r.cell_size >> r.block_size >> r.n_cells >> r.first_slot >> r.n_local >> from_file >> b;
      r.from_file = from_file != 0;
      req.push_back(r);
      base.push_back(b);
    }
  }
  const BuildPlan p = build_many_plan(req, stage);
  for (size_t i : shrink) --req[i].n_local;      // "shrink i": request i's buffer is one slot smaller than what was planned for it
  std::printf("fake");
  for (size_t i : p.fake) std::printf(" %zu", i);
  std::printf("\n");
  size_t items = 0, batches = 0;
  for (size_t c = 0; c < p.classes.size(); ++c) {
    const BuildClass& k = p.classes[c];
    const BuildLayers L = build_many_layers(k.cell_size, k.block_size, k.n_cells, mode);
    std::printf("class %zu %zu %zu %" PRIu64 " batch %zu item_rows %" PRIu64 " kept_rows %" PRIu64 "\n", c, k.cell_size, k.block_size, k.n_cells, k.batch,
                L.item_rows, L.kept_rows);
    std::printf("items");
    for (size_t j = 0; j < k.n_items(); ++j) std::printf(" %zu:%" PRIu64, k.request[j], k.local[j]);
    std::printf("\nlayers");
    for (size_t l = 0; l < L.n(); ++l) std::printf(" %" PRIu64 "/%" PRIu64 "/%" PRIu64, L.rows[l], L.src_prefix[l], L.dst_prefix[l]);
    std::printf("\n");
    size_t kb = 0;
    for (size_t i0 = 0; i0 < k.n_items(); i0 += k.batch, ++kb) {
      const size_t n = std::min(k.batch, k.n_items() - i0);
      std::printf("batch %zu %zu %zu src", kb, i0, n);
      for (size_t l = 0; l < L.n(); ++l) std::printf(" %" PRIu64, build_many_src_row(L, l, n));
      std::printf("\n");
      std::vector<uint64_t> table(L.n() * n);      // exactly the batch's entries: an entry too many is a sanitizer report
      if (!build_many_addr_table(k, L, req, base.data(), i0, n, table.data())) {
        std::printf("table refused\n");
        continue;
      }
      std::printf("table");
      for (uint64_t a : table) std::printf(" %" PRIu64, a);
      std::printf("\n");
    }
    items += k.n_items();
    batches += kb;
  }
  if (items != p.n_items || batches != p.n_batches) { std::printf("totals disagree\n"); return 1; }
  return 0;
}
