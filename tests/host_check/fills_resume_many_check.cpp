// Stand-alone check of csrc/fills_resume_plan.hpp (no HIP, no device), three modes.
//   plan <scenario>   entries (bitmap, n_blocks, range, source, base, seed, buffer address, and how many whole blocks each slot file
//                     holds) and `plan` lines; prints the short-file drops, the request list, the owners, the address table, the seeds
//                     and first cells, the groups of every chunk, every verdict index turned back, and the drop lists of a verdict pattern.
//   args <scenario>   calls as the argument checks see them and per-entry findings; prints the refusal (index, status, text) or "accepted".
//   read <dir> <threads>   writes real slot files into <dir>, reads a three-chunk plan over file and fake entries on <threads> threads and
//                     compares every row with the file bytes (zeros past a file's end); then makes files unreadable and expects the first
//                     failing file in plan order.
// tests/test_fills_resume_many_cpu.py builds it with AddressSanitizer + UBSan (and the read mode with ThreadSanitizer) and compares the
// output line by line with tests/fills_resume_many_models.py.
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fills_resume_plan.hpp"

using namespace cp2i;

static uint64_t seed_stub(uint64_t seed, uint64_t slot) { return seed * 1000003ull + slot; }   // (cp2_slot_seed is the library's)

static void list(const char* name, const std::vector<uint64_t>& v) {
  std::printf("%s", name);
  for (uint64_t x : v) std::printf(" %llu", (unsigned long long)x);
  std::printf("\n");
}

static int plan_mode(const char* path) {
  std::ifstream f(path);
  std::string line, word;
  std::vector<ResumeManySession> s;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    in >> word;
    if (word == "reset") {
      s.clear();
    } else if (word == "entry") {
      ResumeManySession e;
      std::string src;
      size_t nw = 0, nwhole = 0;
      in >> e.n_blocks >> e.first_slot >> e.n_local >> src >> e.base >> e.seed >> e.layer0 >> nw;
      e.from_file = src == "file";
      if (!e.from_file) e.base.clear();
      e.bits.resize(nw);
      for (auto& w : e.bits) in >> w;
      in >> nwhole;
      std::vector<uint64_t> whole(nwhole), dropped;
      for (auto& w : whole) in >> w;
      if (nwhole) {
        std::vector<uint8_t> layer0((size_t)(e.n_local * e.n_blocks) * 32, 0xEE);
        fill_ckpt_drop_short(whole, e.n_blocks, &e.bits, &layer0, &dropped);
        for (uint64_t g = 0; g < e.n_local * e.n_blocks; ++g) {            // a dropped row is zeroed, every other row is left
          const bool was = std::find(dropped.begin(), dropped.end(), g) != dropped.end();
          for (int b = 0; b < 32; ++b)
            if (layer0[(size_t)g * 32 + b] != (was ? 0 : 0xEE)) { std::printf("entry %zu: layer 0 row %llu is wrong\n", s.size(), (unsigned long long)g); return 1; }
        }
      }
      std::printf("dropped %zu:", s.size());
      for (uint64_t g : dropped) std::printf(" %llu", (unsigned long long)g);
      std::printf("\n");
      s.push_back(e);
    } else if (word == "plan") {
      size_t cell = 0, block = 0, chunk = 0;
      in >> cell >> block >> chunk;
      FillsResumePlan p;
      p.build(s, cell, block, seed_stub);
      std::printf("n %zu file %llu\n", p.n(), (unsigned long long)p.n_file);
      list("req", p.req);
      list("first", p.first);
      list("g", p.g);
      list("addr", p.addr);
      std::printf("same_as");
      for (const ReadDataset& d : p.owners) std::printf(" %zu", d.same_as);
      std::printf("\n");
      if (p.fake.empty()) {
        std::printf("fake none\n");
      } else {
        std::printf("fake");
        for (uint8_t x : p.fake) std::printf(" %u", x);
        std::printf("\n");
        list("seeds", p.seeds);
        list("firsts", p.firsts);
      }
      const ReadPlan rp = p.read_plan(chunk);
      for (size_t k = 0; k < rp.n_chunks(); ++k) {
        std::printf("chunk %zu [%zu,%zu):", k, rp.chunk_begin(k), rp.chunk_end(k));
        for (size_t gi = rp.first_group[k]; gi < rp.first_group[k + 1]; ++gi) {
          const ReadGroup& g = rp.groups[gi];
          std::printf(" %zu/%llu=", g.ds, (unsigned long long)g.slot);
          for (size_t q = g.begin; q < g.end; ++q) std::printf("%s%zu", q > g.begin ? "," : "", rp.order[q]);
        }
        std::printf("\n");
      }
      std::printf("where");
      for (size_t i = 0; i < p.n(); ++i) {
        size_t k = 0;
        uint64_t g = 0;
        p.where(i, &k, &g);
        std::printf(" %zu:%llu", k, (unsigned long long)g);
      }
      std::printf("\n");
      std::vector<uint32_t> verdict(p.n());
      for (size_t i = 0; i < p.n(); ++i) verdict[i] = i % 3 == 1 ? 1 + (uint32_t)(i % 2) : 0;
      const auto d = p.drops(verdict.data());
      for (size_t k = 0; k < d.size(); ++k) {
        std::printf("drops %zu:", k);
        for (uint64_t g : d[k]) std::printf(" %llu", (unsigned long long)g);
        std::printf("\n");
      }
    } else if (word == "cuts") {
      size_t piece = 0, ns = 0;
      in >> piece >> ns;
      std::vector<size_t> sizes(ns);
      for (auto& x : sizes) in >> x;
      std::printf("cuts");
      for (const ResumeManyCut& c : fills_resume_cuts(sizes, piece)) std::printf(" %zu:%zu+%zu@%zu%s", c.seg, c.off, c.len, c.at, c.flush ? "!" : "");
      std::printf("\n");
    }
  }
  std::printf("fills resume many ok\n");
  return 0;
}

static int args_mode(const char* path) {
  std::ifstream f(path);
  std::string line, word;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    in >> word;
    if (word == "call") {
      ResumeManyArgs a;
      int cfgs, ranges, roots, paths, out;
      in >> a.flags >> cfgs >> ranges >> roots >> paths >> out >> a.n_fills;
      a.cfgs = cfgs; a.ranges = ranges; a.slot_roots = roots; a.paths = paths; a.out = out;
      std::vector<ResumeManyEntry> e(a.n_fills);
      std::vector<int> begin(a.n_fills);
      for (size_t k = 0; k < a.n_fills; ++k) {
        int c, r, p;
        in >> c >> r >> p >> e[k].cell_size >> e[k].block_size >> begin[k];
        e[k].cfg = c; e[k].slot_roots = r; e[k].path = p;
      }
      ResumeManyRefusal why;
      size_t asked = 0;
      const bool ok = fills_resume_check_args(a, e.data(), [&](size_t k, std::string* text) {
        ++asked;
        if (!e[k].cfg || !e[k].slot_roots || !e[k].path) { std::printf("begin asked of an entry with a NULL\n"); std::exit(1); }
        if (begin[k]) *text = "fill: stub refusal of " + std::to_string(k);
        return begin[k] != 0;
      }, &why);
      if (ok) std::printf("accepted asked %zu\n", asked);
      else std::printf("refused %zu status %d asked %zu: %s\n", why.index, why.status, asked, why.text.c_str());
    } else if (word == "found") {
      size_t n = 0;
      in >> n;
      std::vector<ResumeManyFound> found(n);
      for (size_t k = 0; k < n; ++k) {
        in >> found[k].status;
        if (found[k].status) found[k].text = "finding of " + std::to_string(k);
      }
      ResumeManyRefusal why;
      if (fills_resume_first_failed(found, &why)) std::printf("failed %zu status %d: %s\n", why.index, why.status, why.text.c_str());
      else std::printf("failed none\n");
    } else if (word == "describes") {
      // two metas that differ in one named field (or none): cp2_fill_resume's words
      std::string field;
      in >> field;
      FillCkptMeta got, want;
      for (FillCkptMeta* m : {&got, &want}) {
        m->cell_size = 128; m->block_size = 4096; m->n_cells = 64; m->n_slots = 4; m->first_slot = 1; m->n_local = 2; m->src = FILL_SRC_FILE; m->seed = 7;
        m->file_base = "/x/s";
        m->roots.assign(64, 9);
      }
      if (field == "n_cells") got.n_cells = 128;
      if (field == "first_slot") got.first_slot = 0;
      if (field == "source") got.src = FILL_SRC_FAKE;
      if (field == "base") got.file_base = "/y/s";
      if (field == "root") got.roots[40] = 1;
      const ResumeManyFound r = fills_resume_describes(got, want, "/ck/p");
      std::printf("describes %s: %d %s\n", field.c_str(), r.status, r.text.c_str());
    }
  }
  std::printf("fills resume many ok\n");
  return 0;
}

// ---- the reader against real files -----------------------------------------------------------------------------------------------------------
static uint8_t byte_of(int base, uint64_t slot, uint64_t off) { return (uint8_t)(base * 131 + slot * 31 + off * 7 + (off >> 8) * 3); }

static bool write_file(const std::string& name, int base, uint64_t slot, size_t bytes) {
  std::vector<uint8_t> v(bytes);
  for (size_t i = 0; i < bytes; ++i) v[i] = byte_of(base, slot, i);
  std::ofstream o(name, std::ios::binary);
  o.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)bytes);
  return (bool)o;
}

static int read_mode(const std::string& dir, int threads) {
  const size_t bs = 512, cell = 64;
  const std::string a = dir + "/a", b = dir + "/b";
  // a2, a3, a4 whole (4, 4 and 8 blocks); b0 whole (2 blocks), b1 ends in the middle of its second block
  if (!write_file(fill_slot_file_name(a, 2), 0, 2, 4 * bs) || !write_file(fill_slot_file_name(a, 3), 0, 3, 8 * bs) ||
      !write_file(fill_slot_file_name(a, 4), 0, 4, 8 * bs) || !write_file(fill_slot_file_name(b, 0), 1, 0, 2 * bs) ||
      !write_file(fill_slot_file_name(b, 1), 1, 1, bs + 100)) {
    std::printf("cannot write the slot files\n");
    return 1;
  }
  std::vector<ResumeManySession> s(5);
  s[0].n_blocks = 4; s[0].first_slot = 2; s[0].n_local = 2; s[0].from_file = true; s[0].base = a; s[0].bits = {0xB7};          // 6 of 8
  s[1].n_blocks = 2; s[1].first_slot = 0; s[1].n_local = 1; s[1].seed = 5; s[1].bits = {3};                                      // fake, full
  s[2].n_blocks = 8; s[2].first_slot = 3; s[2].n_local = 2; s[2].from_file = true; s[2].base = a; s[2].bits = {0xFFFF};          // over a3, a4: full
  s[3].n_blocks = 2; s[3].first_slot = 0; s[3].n_local = 2; s[3].from_file = true; s[3].base = b; s[3].bits = {0xF};             // b1's last block is short
  s[4].n_blocks = 1; s[4].first_slot = 0; s[4].n_local = 1; s[4].from_file = true; s[4].base = b; s[4].bits = {0};               // empty
  for (size_t k = 0; k < s.size(); ++k) s[k].layer0 = 0x10000 * (k + 1);
  const int base_of[5] = {0, -1, 0, 1, 1};
  FillsResumePlan p;
  p.build(s, cell, bs, seed_stub);
  const size_t n = p.n(), chunk = (n + 2) / 3;
  const ReadPlan rp = p.read_plan(chunk);
  if (rp.n_chunks() != 3) { std::printf("%zu chunks\n", rp.n_chunks()); return 1; }
  std::vector<uint8_t> rows(n * bs, 0xCD);
  size_t checked = 0;
  for (size_t k = 0; k < rp.n_chunks(); ++k) {
    std::string bad;
    int err = 0;
    if (!p.read_chunk(rp, k, [&](size_t i) { return rows.data() + i * bs; }, threads, &bad, &err)) {
      std::printf("chunk %zu: %s\n", k, slot_file_error(bad, err).c_str());
      return 1;
    }
  }
  for (size_t i = 0; i < n; ++i) {
    const size_t k = (size_t)p.req[3 * i];
    const uint64_t slot = p.req[3 * i + 1], blk = p.req[3 * i + 2];
    const bool fake = !p.fake.empty() && p.fake[i];
    if (fake != !s[k].from_file) { std::printf("request %zu: wrong source\n", i); return 1; }
    struct stat sb;
    size_t size = 0;
    if (!fake && stat(fill_slot_file_name(s[k].base, slot).c_str(), &sb) == 0) size = (size_t)sb.st_size;
    for (size_t j = 0; j < bs; ++j) {
      const uint64_t off = blk * bs + j;
      const uint8_t want = fake ? 0xCD : off < size ? byte_of(base_of[k], slot, off) : 0;   // fake rows are not the reader's; zeros past the end
      if (rows[i * bs + j] != want) { std::printf("request %zu byte %zu: %u, the file has %u\n", i, j, rows[i * bs + j], want); return 1; }
    }
    ++checked;
  }
  std::printf("reader ok: %zu rows, %zu chunks, %llu from files\n", checked, rp.n_chunks(), (unsigned long long)p.n_file);
  // a file that is a directory fails its first read; a file that is gone cannot be opened: the first of the chunk's groups is named
  const std::string gone = fill_slot_file_name(a, 4), dirfile = fill_slot_file_name(a, 3);
  if (unlink(gone.c_str()) != 0 || unlink(dirfile.c_str()) != 0 || mkdir(dirfile.c_str(), 0700) != 0) { std::printf("cannot damage the files\n"); return 1; }
  for (size_t k = 0; k < rp.n_chunks(); ++k) {
    std::string bad;
    int err = -1;
    const bool ok = p.read_chunk(rp, k, [&](size_t i) { return rows.data() + i * bs; }, threads, &bad, &err);
    // what the plan's order says: the first group of the chunk over a3 (a directory) or a4 (gone)
    std::string want;
    int want_err = -1;
    for (size_t gi = rp.first_group[k]; gi < rp.first_group[k + 1] && want.empty(); ++gi) {
      const std::string name = fill_slot_file_name(s[rp.groups[gi].ds].base, rp.groups[gi].slot);
      if (name == gone) { want = name; want_err = 0; }
      if (name == dirfile) { want = name; want_err = EISDIR; }
    }
    if (ok != want.empty() || (!ok && (bad != want || err != want_err))) {
      std::printf("chunk %zu: %s / %d where the plan's first failing file is %s / %d\n", k, ok ? "fine" : bad.c_str(), err, want.c_str(), want_err);
      return 1;
    }
    std::printf("chunk %zu fails: %s\n", k, ok ? "no" : slot_file_error(bad.substr(dir.size() + 1), err == 0 ? 0 : EISDIR).c_str());
  }
  std::printf("fills resume many ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  if (mode == "plan") return plan_mode(argv[2]);
  if (mode == "args") return args_mode(argv[2]);
  if (mode == "read" && argc == 4) return read_mode(argv[2], std::atoi(argv[3]));
  return 2;
}
