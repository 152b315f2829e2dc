// csrc/read_blocks_plan.hpp on the CPU, under AddressSanitizer + UBSan (tests/test_read_blocks_cpu.py compiles and drives this): no HIP,
// no device.  It reads one call described as text (tests/read_blocks_models.py: describe) and prints what the plan makes of it, for the
// Python model to compare with:
//   read_blocks_check plan FILE         "refused <message>", or the read plan ("chunk", "group <ds> <slot> <requests...>"), "path_off ..."
//                                       and "addr ..." lines
//   read_blocks_check read FILE OUT     runs the reader of every chunk against the slot files the datasets name, request i into row i of
//                                       OUT (n x block_size bytes); "read ok", or "error <slot_file_error's message>"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "read_blocks_plan.hpp"

using namespace cp2i;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  std::ifstream in(argv[2]);
  if (!in) return 2;
  ReadArgs a;
  std::vector<ReadDataset> ds;
  std::vector<uint64_t> req;
  size_t chunk = 1;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream s(line);
    std::string tag;
    s >> tag;
    if (tag == "args") {
      int v[6];
      for (int& x : v) s >> x;
      a.ds = v[0]; a.req = v[1]; a.data = v[2]; a.paths = v[3]; a.path_off = v[4]; a.status = v[5];
      s >> a.n_ds >> a.flags;
    } else if (tag == "D") {
      ReadDataset d;
      int null, foreign, whole, from_file;
      size_t layers;
      s >> null >> foreign >> d.same_as >> d.cell_size >> d.block_size >> d.n_cells >> d.first_slot >> d.n_local >> d.mode >> whole >> from_file >> d.seed >>
          d.nodes >> d.root_off >> d.root_size >> d.base >> layers;
      d.null = null; d.foreign = foreign; d.whole = whole; d.from_file = from_file;
      d.offs.resize(layers);
      d.sizes.resize(layers);
      for (auto& x : d.offs) s >> x;
      for (auto& x : d.sizes) s >> x;
      ds.push_back(d);
    } else if (tag == "chunk") {
      s >> chunk;
    } else if (tag == "R") {
      uint64_t k, sl, b;
      s >> k >> sl >> b;
      req.push_back(k); req.push_back(sl); req.push_back(b);
    }
  }
  const size_t n = req.size() / 3;
  a.n = n;
  std::string err;
  if (!read_blocks_validate(a, ds, req.data(), &err)) {
    std::printf("refused %s\n", err.c_str());
    return 0;
  }
  const ReadPlan p = read_blocks_plan(ds, req.data(), n, chunk);
  if (mode == "plan") {
    for (size_t k = 0; k < p.n_chunks(); ++k) {
      std::printf("chunk %zu %zu\n", p.chunk_begin(k), p.chunk_end(k));
      for (size_t g = p.first_group[k]; g < p.first_group[k + 1]; ++g) {
        std::printf("group %zu %" PRIu64, p.groups[g].ds, p.groups[g].slot);
        for (size_t q = p.groups[g].begin; q < p.groups[g].end; ++q) std::printf(" %zu", p.order[q]);
        std::printf("\n");
      }
    }
    const std::vector<uint64_t> off = read_blocks_path_off(ds, req.data(), n);
    std::printf("path_off");
    for (uint64_t x : off) std::printf(" %" PRIu64, x);
    std::printf("\naddr");
    for (uint64_t x : read_blocks_addr_table(ds, req.data(), n, off)) std::printf(" %" PRIu64, x);
    std::printf("\nchunk_of %zu\n", n ? read_blocks_chunk((size_t)1 << 20, ds[0].block_size, n) : 0);
    return 0;
  }
  if (mode != "read" || argc < 4) return 2;
  const size_t bs = n ? ds[0].block_size : 0;
  // each row in an allocation of its own size, so that a write past a row is a sanitizer report; 0xA5 where nothing was read
  std::vector<std::vector<uint8_t>> rows(n, std::vector<uint8_t>(bs, 0xA5));
  for (size_t k = 0; k < p.n_chunks(); ++k) {
    std::string bad;
    int e = 0;
    if (!read_blocks_read_chunk(p, k, ds, req.data(), bs, [&](size_t i) { return rows[i].data(); }, 3, &bad, &e)) {
      std::printf("error %s\n", slot_file_error(bad, e).c_str());
      return 0;
    }
  }
  std::ofstream out(argv[3], std::ios::binary);
  for (auto& r : rows) out.write(reinterpret_cast<const char*>(r.data()), (std::streamsize)r.size());
  std::printf("read ok %zu\n", n);
  return 0;
}
