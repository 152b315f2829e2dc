// A fill checkpoint's host logic (csrc/fill_checkpoint.hpp, the header fill.cpp uses, and FillPlan::drop / restore of csrc/fill_plan.hpp)
// walked over random sessions, every answer compared with a direct restatement kept here: the layout's offsets and size, the round trip
// (1 block per slot, bitmaps that are no multiple of 64 bits, empty and full sessions, absent rows zeroed whatever they held), every
// truncation point and every single flipped byte of a small file refused, each differing field named, the blocks a short or missing file
// drops, and the read plan (each present block once, ascending per file, chunks of the stated size).  Then the two readers the re-check and
// cp2_fill_adopt share, against REAL slot files in a scratch directory: fill_slot_files_cover (absent, empty, whole and ragged files; a path
// component that is a file; a name too long to stat) and fill_read_chunk (every chunk of a random plan byte for byte, into a buffer of
// exactly a chunk; files removed, replaced by a directory or cut short after the plan was made).  Built with AddressSanitizer + UBSan.  No GPU.
//   g++ -std=c++17 -pthread -fsanitize=address,undefined -I<csrc> fill_checkpoint_check.cpp -o check && ./check <sessions> <scratch dir>
#include <sys/stat.h>
#include <unistd.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "fill_checkpoint.hpp"
#include "fill_plan.hpp"

using namespace cp2i;

static int failures = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      ++failures;                                     \
      if (failures < 20) {                            \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                     \
        std::printf("\n");                            \
      }                                               \
    }                                                 \
  } while (0)

static std::mt19937_64 rng(20261017);
static uint64_t pick(uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); }

// a random session: fill = 0 empty, 1 full, 2 random
static FillCheckpoint random_checkpoint(uint64_t n_local, uint64_t n_blocks, int fill, bool file) {
  FillCheckpoint c;
  FillCkptMeta& m = c.meta;
  m.cell_size = 64 << pick(0, 3);
  const uint64_t cpb = 1ULL << pick(0, 4);
  m.block_size = m.cell_size * cpb;
  m.n_cells = n_blocks * cpb;
  m.first_slot = pick(0, 6);
  m.n_local = n_local;
  m.n_slots = m.first_slot + n_local + pick(0, 3);
  m.src = file ? FILL_SRC_FILE : FILL_SRC_FAKE;
  m.seed = rng();
  if (file) {
    const size_t len = (size_t)pick(0, 19);
    for (size_t i = 0; i < len; ++i) m.file_base.push_back((char)('a' + pick(0, 25)));
  }
  m.roots.resize(n_local * 32);
  for (auto& b : m.roots) b = (uint8_t)rng();
  const uint64_t total = n_local * n_blocks;
  c.bits.assign((total + 63) / 64, 0);
  c.layer0.resize(total * 32);
  for (auto& b : c.layer0) b = (uint8_t)(rng() | 1);            // never zero: an absent row must come back as zeros all the same
  for (uint64_t g = 0; g < total; ++g)
    if (fill == 1 || (fill == 2 && (rng() & 1))) c.bits[g >> 6] |= 1ULL << (g & 63);
  return c;
}

static bool same_meta(const FillCkptMeta& a, const FillCkptMeta& b) {
  return a.cell_size == b.cell_size && a.block_size == b.block_size && a.n_cells == b.n_cells && a.n_slots == b.n_slots && a.first_slot == b.first_slot &&
         a.n_local == b.n_local && a.src == b.src && a.seed == b.seed && a.file_base == b.file_base && a.roots == b.roots;
}

// ---- the two readers against real files ---------------------------------------------------------------------------------------------------
static void put_file(const std::string& name, const std::vector<uint8_t>& bytes) {
  FILE* fh = std::fopen(name.c_str(), "wb");
  CHECK(fh && (bytes.empty() || std::fwrite(bytes.data(), 1, bytes.size(), fh) == bytes.size()), "cannot write %s", name.c_str());
  if (fh) std::fclose(fh);
}

static void slot_files_check(const std::string& dir, int rounds) {
  for (int round = 0; round < rounds; ++round) {
    const size_t bs = (size_t)pick(1, 64);
    const uint64_t n_blocks = pick(1, 9), n_local = pick(1, 6), first = pick(0, 6), total = n_local * n_blocks;
    const std::string base = dir + "/slot";
    // each file: absent, empty, a whole number of blocks, or that and a partial tail
    std::vector<std::vector<uint8_t>> bytes(n_local);
    std::vector<bool> there(n_local);
    std::vector<uint64_t> want(n_local), whole;
    for (uint64_t s = 0; s < n_local; ++s) {
      const int kind = (int)pick(0, 3);
      there[s] = kind != 0;
      size_t size = kind < 2 ? 0 : (size_t)pick(1, n_blocks) * bs;
      if (kind == 3 && bs > 1) size = size - bs + (size_t)pick(1, bs - 1);       // 0 .. n_blocks - 1 whole blocks and a tail
      bytes[s].resize(size);
      for (auto& b : bytes[s]) b = (uint8_t)rng();
      want[s] = size / bs;
      if (there[s]) put_file(fill_slot_file_name(base, first + s), bytes[s]);
    }
    std::string bad;
    CHECK(fill_slot_files_cover(base, first, n_local, bs, &whole, &bad) && whole == want, "round %d: the whole blocks of the files", round);

    // a presence bitmap of what the files cover, every chunk byte for byte; the buffer is exactly a chunk, so an overrun is ASan's
    std::vector<uint64_t> bits((total + 63) / 64, 0);
    for (uint64_t g = 0; g < total; ++g)
      if (g % n_blocks < whole[g / n_blocks] && (rng() & 1)) bits[g >> 6] |= 1ULL << (g & 63);
    const size_t chunk = (size_t)pick(1, 9);
    const FillReadPlan rp = fill_read_plan(bits, total, n_blocks, chunk);
    std::unique_ptr<uint8_t[]> host(new uint8_t[chunk * bs]);
    for (size_t k = 0; k < rp.n_chunks(); ++k) {
      std::memset(host.get(), 0xA5, chunk * bs);
      int e = -1;
      CHECK(fill_read_chunk(rp, k, base, first, bs, host.get(), &bad, &e), "round %d: chunk %zu cannot be read: %s", round, k, slot_file_error(bad, e).c_str());
      for (size_t i = rp.chunk_begin(k); i < rp.chunk_end(k); ++i)
        CHECK(std::memcmp(host.get() + (i - rp.chunk_begin(k)) * bs, &bytes[rp.g[i] / n_blocks][(rp.g[i] % n_blocks) * bs], bs) == 0,
              "round %d: chunk %zu: entry %zu holds other bytes", round, k, i);
    }

    // after the plan was made.  A file removed cannot be opened; a directory in its place opens and fails to read (EISDIR); the lowest such
    // file of the chunk is the one named.  A file cut short reads as the read rule has it: zeros from its end on, and no error -- the device
    // then finds another root.
    if (rp.n_chunks()) {
      const size_t k = (size_t)pick(0, rp.n_chunks() - 1);
      const std::vector<FillReadPlan::Run> runs = rp.runs(k);
      const FillReadPlan::Run& cut = runs[(size_t)pick(0, runs.size() - 1)];
      const std::string cut_name = fill_slot_file_name(base, first + cut.local);
      const size_t keep = (size_t)(rp.g[cut.i0] % n_blocks) * bs + (size_t)pick(0, bs - 1);      // inside the run's first block
      CHECK(truncate(cut_name.c_str(), (off_t)keep) == 0, "round %d: cannot cut %s", round, cut_name.c_str());
      int e = -1;
      CHECK(fill_read_chunk(rp, k, base, first, bs, host.get(), &bad, &e), "round %d: a file cut short is an error", round);
      for (size_t i = cut.i0; i < cut.i1; ++i)
        for (size_t j = 0; j < bs; ++j) {
          const size_t at = (size_t)(rp.g[i] % n_blocks) * bs + j;
          CHECK(host[(i - rp.chunk_begin(k)) * bs + j] == (at < keep ? bytes[cut.local][at] : 0), "round %d: chunk %zu: byte %zu of a file cut at %zu", round, k, at, keep);
        }
      const size_t lo = (size_t)pick(0, runs.size() - 1), hi = (size_t)pick(lo, runs.size() - 1);  // two files fail (or one): the lower is named
      const bool dir_lo = rng() & 1;
      for (size_t r : std::set<size_t>{lo, hi}) {
        const std::string name = fill_slot_file_name(base, first + runs[r].local);
        CHECK(unlink(name.c_str()) == 0, "round %d: cannot remove %s", round, name.c_str());
        there[runs[r].local] = false;
      }
      const std::string lo_name = fill_slot_file_name(base, first + runs[lo].local);
      if (dir_lo) CHECK(mkdir(lo_name.c_str(), 0700) == 0, "round %d: cannot make the directory %s", round, lo_name.c_str());
      e = -1;
      bad.clear();
      CHECK(!fill_read_chunk(rp, k, base, first, bs, host.get(), &bad, &e) && bad == lo_name && e == (dir_lo ? EISDIR : 0),
            "round %d: chunk %zu: '%s' errno %d reported, '%s' %s expected", round, k, bad.c_str(), e, lo_name.c_str(), dir_lo ? "EISDIR" : "not opened");
      if (dir_lo) rmdir(lo_name.c_str());
    }
    for (uint64_t s = 0; s < n_local; ++s)
      if (there[s]) unlink(fill_slot_file_name(base, first + s).c_str());
  }
  // a path component that is a regular file: ENOTDIR, absent like ENOENT; a name no stat takes: an error that names the first file
  std::vector<uint64_t> whole;
  std::string bad;
  put_file(dir + "/plain", {1, 2, 3});
  CHECK(fill_slot_files_cover(dir + "/plain/slot", 3, 4, 1, &whole, &bad) && whole == std::vector<uint64_t>(4, 0), "files under a regular file are not absent");
  unlink((dir + "/plain").c_str());
  const std::string longer = dir + "/" + std::string(PATH_MAX, 'x');
  CHECK(!fill_slot_files_cover(longer, 3, 4, 1, &whole, &bad) && bad == fill_slot_file_name(longer, 3), "a name longer than PATH_MAX: '%zu' bytes reported", bad.size());
  CHECK(slot_file_error(bad, 0) == "cannot open " + bad, "the text of a file that cannot be looked at");
}

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: fill_checkpoint_check <sessions> <scratch dir>\n"); return 2; }
  const int rounds = std::atoi(argv[1]);
  std::string err;

  // ---- round trips ------------------------------------------------------------------------------------------------------------------------
  for (int round = 0; round < rounds; ++round) {
    const uint64_t n_blocks = round % 7 == 0 ? 1 : (round % 5 == 0 ? pick(1, 70) : (uint64_t)1 << pick(0, 6));
    const uint64_t n_local = round % 11 == 0 ? 1 : pick(1, 5);
    const int fill = round % 3;
    const FillCheckpoint c = random_checkpoint(n_local, n_blocks, fill, round & 1);
    const uint64_t total = n_local * n_blocks;
    std::vector<uint8_t> buf, again;
    CHECK(fill_ckpt_serialise(c, &buf) && fill_ckpt_serialise(c, &again) && buf == again, "round %d: serialise fails or is not deterministic", round);
    // the layout, restated
    const size_t base_pad = (c.meta.file_base.size() + 7) / 8 * 8;
    const size_t want = 88 + base_pad + n_local * 32 + (total + 63) / 64 * 8 + total * 32 + 8;
    CHECK(buf.size() == want, "round %d: %zu bytes, expected %zu", round, buf.size(), want);
    CHECK(std::memcmp(buf.data(), "CP2FILL1", 8) == 0 && fill_ckpt_word(&buf[8 + 72]) == n_blocks, "round %d: magic or n_blocks", round);
    FillCheckpoint back;
    err.clear();
    CHECK(fill_ckpt_parse(buf.data(), buf.size(), &back, &err), "round %d: the file does not parse: %s", round, err.c_str());
    CHECK(same_meta(back.meta, c.meta) && back.bits == c.bits, "round %d: meta or bitmap changed", round);
    CHECK(back.layer0.size() == c.layer0.size(), "round %d: layer 0 size", round);
    uint64_t present = 0;
    for (uint64_t g = 0; g < total && back.layer0.size() == c.layer0.size(); ++g) {
      const bool p = (c.bits[g >> 6] >> (g & 63)) & 1;
      present += p;
      bool zero = true, equal = true;
      for (int k = 0; k < 32; ++k) {
        zero = zero && back.layer0[g * 32 + k] == 0;
        equal = equal && back.layer0[g * 32 + k] == c.layer0[g * 32 + k];
      }
      CHECK(p ? equal : zero, "round %d: row %llu is %s", round, (unsigned long long)g, p ? "changed" : "not zeroed");
    }
    CHECK(fill == 2 || present == (fill ? total : 0), "round %d: the empty / full session is not", round);
    CHECK(fill_ckpt_differs(back.meta, c.meta).empty(), "round %d: a checkpoint differs from its own session", round);

    // FillPlan takes the bitmap over and gives blocks back
    FillPlan plan;
    plan.init(c.meta.first_slot, n_local, n_blocks);
    CHECK(plan.restore(back.bits) && plan.n_present == present && plan.n_missing() == total - present, "round %d: restore", round);
    std::vector<uint64_t> wrong(back.bits);
    wrong.push_back(0);
    CHECK(!plan.restore(wrong), "round %d: a bitmap of another size is taken", round);
    if (total & 63) {
      wrong = back.bits;
      wrong.back() |= 1ULL << 63;
      CHECK(!plan.restore(wrong), "round %d: a bit past the last block is taken", round);
    }
    std::vector<uint64_t> give;
    std::set<uint64_t> gone;
    for (uint64_t g = 0; g < total; ++g)
      if (rng() % 3 == 0) { give.push_back(g); if ((c.bits[g >> 6] >> (g & 63)) & 1) gone.insert(g); }
    give.push_back(total);                                     // out of range: ignored
    if (!give.empty()) give.push_back(give[0]);                // twice: counted once
    CHECK(plan.drop(give.data(), give.size()) == gone.size() && plan.n_present == present - gone.size(), "round %d: drop counts", round);
    for (uint64_t g = 0; g < total; ++g) {
      const bool want_p = ((c.bits[g >> 6] >> (g & 63)) & 1) && !gone.count(g);
      CHECK(plan.present(g / n_blocks, g % n_blocks) == want_p, "round %d: bit %llu after drop", round, (unsigned long long)g);
    }
    std::vector<uint64_t> miss(2 * total);
    CHECK(plan.missing(miss.data(), total) == total - present + gone.size(), "round %d: missing after drop", round);

    // ---- the read plan ------------------------------------------------------------------------------------------------------------------
    const size_t chunk = (size_t)pick(1, 9);
    const FillReadPlan rp = fill_read_plan(c.bits, total, n_blocks, chunk);
    CHECK(rp.g.size() == present, "round %d: the plan holds %zu blocks of %llu", round, rp.g.size(), (unsigned long long)present);
    for (size_t i = 0; i < rp.g.size(); ++i) {
      CHECK(rp.g[i] < total && ((c.bits[rp.g[i] >> 6] >> (rp.g[i] & 63)) & 1), "round %d: entry %zu is not a present block", round, i);
      CHECK(i == 0 || rp.g[i - 1] < rp.g[i], "round %d: entry %zu is not above the one before", round, i);
    }
    CHECK(rp.n_chunks() == (present + chunk - 1) / chunk, "round %d: chunk count", round);
    size_t next = 0;
    for (size_t k = 0; k < rp.n_chunks(); ++k) {
      CHECK(rp.chunk_begin(k) == next && rp.chunk_end(k) - rp.chunk_begin(k) == (k + 1 < rp.n_chunks() ? chunk : present - k * chunk), "round %d: chunk %zu", round, k);
      size_t at = rp.chunk_begin(k);
      uint64_t last_local = ~0ULL;
      for (const FillReadPlan::Run& r : rp.runs(k)) {
        CHECK(r.i0 == at && r.i1 > r.i0 && r.i1 <= rp.chunk_end(k), "round %d: chunk %zu: a run does not follow the one before", round, k);
        CHECK(last_local == ~0ULL || r.local > last_local, "round %d: chunk %zu: files not ascending", round, k);
        for (size_t i = r.i0; i < r.i1; ++i) CHECK(rp.g[i] / n_blocks == r.local, "round %d: chunk %zu: entry %zu in the wrong file", round, k, i);
        last_local = r.local;
        at = r.i1;
      }
      CHECK(at == rp.chunk_end(k), "round %d: chunk %zu: its runs end at %zu", round, k, at);
      next = rp.chunk_end(k);
    }
    CHECK(next == present, "round %d: the chunks cover %zu of %llu", round, next, (unsigned long long)present);

    // ---- short and missing files ----------------------------------------------------------------------------------------------------------
    std::vector<uint64_t> whole(n_local), bits2(c.bits), dropped;
    std::vector<uint8_t> l0(back.layer0);
    for (auto& w : whole) w = rng() % 3 == 0 ? 0 : pick(0, n_blocks);
    fill_ckpt_drop_short(whole, n_blocks, &bits2, &l0, &dropped);
    size_t k = 0;
    for (uint64_t g = 0; g < total; ++g) {
      const bool was = (c.bits[g >> 6] >> (g & 63)) & 1, backed = g % n_blocks < whole[g / n_blocks], now = (bits2[g >> 6] >> (g & 63)) & 1;
      CHECK(now == (was && backed), "round %d: block %llu after the short files", round, (unsigned long long)g);
      if (was && !backed) {
        CHECK(k < dropped.size() && dropped[k] == g, "round %d: the dropped list misses %llu", round, (unsigned long long)g);
        ++k;
        bool zero = true;
        for (int j = 0; j < 32; ++j) zero = zero && l0[g * 32 + j] == 0;
        CHECK(zero, "round %d: the row of dropped block %llu stays", round, (unsigned long long)g);
      } else {
        CHECK(std::memcmp(&l0[g * 32], &back.layer0[g * 32], 32) == 0, "round %d: the row of block %llu changed", round, (unsigned long long)g);
      }
    }
    CHECK(k == dropped.size(), "round %d: %zu dropped, %zu expected", round, dropped.size(), k);
  }

  // ---- every truncation point, every flipped byte, bytes appended: a small file with a base name and 70 blocks (not a multiple of 64) ------
  {
    const FillCheckpoint c = random_checkpoint(2, 35, 2, true);
    std::vector<uint8_t> buf;
    CHECK(fill_ckpt_serialise(c, &buf), "the small file does not serialise");
    FillCheckpoint back;
    for (size_t n = 0; n < buf.size(); ++n) {
      std::vector<uint8_t> cut(buf.begin(), buf.begin() + (long)n);            // its own allocation: a read past n is caught
      err.clear();
      CHECK(!fill_ckpt_parse(cut.data(), n, &back, &err) && !err.empty(), "a file cut to %zu of %zu bytes parses", n, buf.size());
    }
    for (size_t i = 0; i < buf.size(); ++i) {
      std::vector<uint8_t> bad(buf);
      bad[i] ^= (uint8_t)(1u << (i % 8));
      err.clear();
      CHECK(!fill_ckpt_parse(bad.data(), bad.size(), &back, &err) && !err.empty(), "byte %zu flipped and the file parses", i);
    }
    std::vector<uint8_t> longer(buf);
    longer.push_back(0);
    CHECK(!fill_ckpt_parse(longer.data(), longer.size(), &back, &err), "a file with a byte appended parses");
    // sizes that would wrap or exhaust memory are refused from the header alone
    for (int word : {5, 9, 8}) {
      std::vector<uint8_t> bad(buf);
      fill_ckpt_put(&bad[8 + 8 * (size_t)word], ~0ULL >> (word == 8 ? 0 : 3));
      CHECK(!fill_ckpt_parse(bad.data(), bad.size(), &back, &err), "header word %d out of bounds and the file parses", word);
    }
    CHECK(fill_ckpt_parse(buf.data(), buf.size(), &back, &err), "the intact file no longer parses: %s", err.c_str());
  }

  // ---- each field that differs is named, in the stated order -------------------------------------------------------------------------------
  for (int file = 0; file < 2; ++file) {
    const FillCheckpoint c = random_checkpoint(3, 8, 2, file);
    struct Case { const char* name; void (*change)(FillCkptMeta&); };
    const Case cases[] = {
        {"cell_size", [](FillCkptMeta& m) { m.cell_size *= 2; }},   {"block_size", [](FillCkptMeta& m) { m.block_size *= 2; }},
        {"n_cells", [](FillCkptMeta& m) { m.n_cells *= 2; }},       {"n_slots", [](FillCkptMeta& m) { m.n_slots += 1; }},
        {"first_slot", [](FillCkptMeta& m) { m.first_slot += 1; }}, {"n_local", [](FillCkptMeta& m) { m.n_local -= 1; m.roots.resize(m.n_local * 32); }},
        {"source", [](FillCkptMeta& m) { m.src ^= 1; }},
        {file ? "file base name" : "seed", file ? +[](FillCkptMeta& m) { m.file_base += "x"; } : +[](FillCkptMeta& m) { m.seed += 1; }},
        {"stated root of slot", [](FillCkptMeta& m) { m.roots[5] ^= 1; }}};
    const size_t n_cases = sizeof cases / sizeof cases[0];
    for (size_t i = 0; i < n_cases; ++i) {
      FillCkptMeta want = c.meta;
      for (size_t j = i; j < n_cases; ++j) cases[j].change(want);          // this field and every later one differ: the first is named
      const std::string d = fill_ckpt_differs(c.meta, want);
      CHECK(d.find(cases[i].name) == 0, "source %d: changed from '%s' on, named '%s'", file, cases[i].name, d.c_str());
    }
    FillCkptMeta want = c.meta;
    want.roots[32 * 1] ^= 0x80;
    CHECK(fill_ckpt_differs(c.meta, want) == "stated root of slot " + std::to_string(c.meta.first_slot + 1) + " differs", "the slot of a differing root");
    want = c.meta;                                                           // what does not describe the session is not compared
    if (file) want.seed += 1; else want.file_base = "elsewhere";
    CHECK(fill_ckpt_differs(c.meta, want).empty(), "source %d: a field of the other source is compared", file);
  }

  slot_files_check(argv[2], rounds);

  std::printf("fill checkpoint ok: %d sessions, %d failures\n", rounds, failures);
  return failures ? 1 : 0;
}
