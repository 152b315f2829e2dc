// Stand-alone check of csrc/repair_many_plan.hpp (no HIP, no device), two modes.
//   plan <scenario>                  datasets as the plan sees them and `call` lines; prints the refusal, or the descriptor table, the most
//                                    path rows a chunk stages, the write groups of a verdict pattern and what the call makes of a writer
//                                    whose every fourth file (1, 5, ...) fails.
//   write <scenario> <dir> <threads> the one call of the scenario, its base names under <dir>, written for real on <threads> threads: prints
//                                    the files, the fdatasync calls counted (this program's own fdatasync stands in front of libc's),
//                                    which worker took which file, what stopped each file, and the settled statuses, count and stamps.
//                                    The test laid the files out (some present, some missing, some directories) and reads them back.
// tests/test_repair_many_cpu.py builds it with AddressSanitizer + UBSan (and the write mode with ThreadSanitizer) and compares the output
// line by line with tests/repair_many_models.py.
#include <sys/stat.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "repair_many_plan.hpp"

using namespace cp2i;

static std::atomic<size_t> g_syncs{0};
extern "C" int fdatasync(int fd) {   // counted, then the system call itself
  ++g_syncs;
  return (int)syscall(SYS_fdatasync, fd);
}

struct Scenario {
  std::vector<ReadDataset> ds;
  RepairManyArgs a;
  size_t chunk = 1;
  std::vector<uint64_t> req, path_off;
};

static ReadDataset parse_ds(std::istringstream& in, const std::string& prefix) {
  ReadDataset d;
  std::string kind;
  int whole = 0, from_file = 0;
  size_t n_layers = 0;
  in >> kind >> d.cell_size >> d.block_size >> d.n_cells >> d.first_slot >> d.n_local >> d.mode >> whole >> from_file >> d.base >> d.nodes >> d.roots >>
      d.root_off >> d.root_size >> n_layers >> d.same_as;
  d.null = kind == "null";
  d.foreign = kind == "foreign";
  d.whole = whole != 0;
  d.from_file = from_file != 0;
  d.base = prefix + d.base;
  // the layers of the tree over a slot's block roots, as many as the line says (only their number matters to the plan)
  uint64_t m = d.n_blocks(), off = d.root_off;
  for (size_t l = 0; l < n_layers; ++l) {
    d.offs.push_back(off);
    d.sizes.push_back(m);
    off += d.n_local * m;
    m = (m + 1) / 2;
  }
  return d;
}

static void parse_call(std::istringstream& in, Scenario* s) {
  int ds, req, data, paths, path_off, status;
  size_t n_off = 0;
  in >> s->a.flags >> ds >> req >> data >> paths >> path_off >> status >> s->a.n_ds >> s->a.n >> s->chunk >> n_off;
  s->a.ds = ds; s->a.req = req; s->a.data = data; s->a.paths = paths; s->a.path_off = path_off; s->a.status = status;
  s->req.assign(3 * s->a.n, 0);
  for (auto& x : s->req) in >> x;
  s->path_off.assign(n_off, 0);
  for (auto& x : s->path_off) in >> x;
}

static void print_settled(const Scenario& s, const std::vector<RepairManyFile>& groups, const std::vector<WriteOutcome>& out, std::vector<uint32_t> status) {
  size_t n_written = 0;
  std::vector<std::vector<FileStamp>> written;
  const size_t bad = repair_many_settle(s.ds, s.req.data(), groups, out, 2, status.data(), &n_written, &written);
  std::printf("settled bad %zu written %zu status", bad, n_written);
  for (uint32_t x : status) std::printf(" %u", x);
  std::printf("\n");
  for (size_t k = 0; k < written.size(); ++k) {
    std::printf("stamps %zu:", k);
    for (const FileStamp& f : written[k]) std::printf(" %llu", (unsigned long long)f.slot);
    std::printf("\n");
  }
}

static int plan_mode(const char* path) {
  std::ifstream f(path);
  std::string line, word;
  Scenario s;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    in >> word;
    if (word == "reset") {
      s = Scenario();
    } else if (word == "ds") {
      s.ds.push_back(parse_ds(in, ""));
    } else if (word == "call") {
      parse_call(in, &s);
      const uint64_t* po = s.a.path_off ? s.path_off.data() : nullptr;
      std::string err;
      if (!repair_many_validate(s.a, s.ds, s.req.data(), po, &err)) {
        std::printf("refused: %s\n", err.c_str());
        continue;
      }
      const size_t n = s.a.n;
      std::printf("accepted n %zu most %llu\n", n, (unsigned long long)repair_many_most_path_rows(po, n, s.chunk));
      const std::vector<RepairManyDesc> t = repair_many_table(s.ds, s.req.data(), po, n, s.chunk);
      for (size_t i = 0; i < n; ++i)
        std::printf("desc %zu %llu %llu %llu %llu %u\n", i, (unsigned long long)t[i].want, (unsigned long long)t[i].blk, (unsigned long long)t[i].n_blocks,
                    (unsigned long long)t[i].path_at, t[i].len);
      std::vector<uint32_t> status(n);
      for (size_t i = 0; i < n; ++i) status[i] = i % 3 == 1 ? 1 : 0;
      const std::vector<RepairManyFile> groups = repair_many_write_groups(s.ds, s.req.data(), status.data(), n, 0);
      std::vector<WriteOutcome> out(groups.size());
      for (size_t j = 0; j < groups.size(); ++j) {
        std::printf("file %zu/%llu %s:", groups[j].ds, (unsigned long long)groups[j].slot, groups[j].name.c_str());
        for (size_t q = 0; q < groups[j].reqs.size(); ++q) std::printf("%s%zu", q ? "," : " ", groups[j].reqs[q]);
        std::printf("\n");
        out[j].what = j % 4 == 1 ? 5 : 0;
      }
      print_settled(s, groups, out, status);
    }
  }
  std::printf("repair many ok\n");
  return 0;
}

static uint8_t row_byte(size_t i, size_t j) { return (uint8_t)(i * 37 + j * 11 + (j >> 8)); }

static int write_mode(const char* path, const std::string& dir, int threads) {
  std::ifstream f(path);
  std::string line, word;
  Scenario s;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    in >> word;
    if (word == "ds") s.ds.push_back(parse_ds(in, dir + "/"));
    else if (word == "call") parse_call(in, &s);
  }
  const size_t n = s.a.n, bs = s.ds[0].block_size;
  std::vector<uint8_t> data(n * bs);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < bs; ++j) data[i * bs + j] = row_byte(i, j);
  std::vector<uint32_t> status(n);
  for (size_t i = 0; i < n; ++i) status[i] = i % 3 == 1 ? 1 : 0;
  const std::vector<RepairManyFile> groups = repair_many_write_groups(s.ds, s.req.data(), status.data(), n, 0);
  std::vector<WriteFile> files(groups.size());
  std::vector<FileStamp> before(groups.size());
  for (size_t j = 0; j < groups.size(); ++j) {
    files[j].name = groups[j].name;
    for (size_t i : groups[j].reqs) files[j].rows.push_back({s.req[3 * i + 2] * (uint64_t)bs, data.data() + i * bs});
    (void)repair_stat_stamp(groups[j].name, before[j].before);
  }
  const std::vector<WriteOutcome> out = write_files_threaded(files, bs, threads);
  std::printf("files %zu syncs %zu\n", files.size(), g_syncs.load());
  std::printf("workers");
  for (const WriteOutcome& o : out) std::printf(" %d", o.worker);
  std::printf("\n");
  for (size_t j = 0; j < groups.size(); ++j) {
    uint64_t now[2];
    (void)repair_stat_stamp(groups[j].name, now);
    const bool same_before = out[j].before[0] == before[j].before[0] && out[j].before[1] == before[j].before[1];
    const bool same_after = out[j].what || (out[j].after[0] == now[0] && out[j].after[1] == now[1]);
    std::printf("file %s: %d%s\n", groups[j].name.substr(dir.size() + 1).c_str(), out[j].what, same_before && same_after ? "" : " STAMPS DIFFER");
  }
  print_settled(s, groups, out, status);
  std::printf("repair many ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  if (mode == "plan") return plan_mode(argv[2]);
  if (mode == "write" && argc == 5) return write_mode(argv[2], argv[3], std::atoi(argv[4]));
  return 2;
}
