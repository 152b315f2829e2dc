// A fill checkpoint's host logic (csrc/fill_checkpoint.hpp, the header fill.cpp uses, and FillPlan::drop / restore of csrc/fill_plan.hpp)
// walked over random sessions, every answer compared with a direct restatement kept here: the layout's offsets and size, the round trip
// (1 block per slot, bitmaps that are no multiple of 64 bits, empty and full sessions, absent rows zeroed whatever they held), every
// truncation point and every single flipped byte of a small file refused, each differing field named, the blocks a short or missing file
// drops, and the read plan (each present block once, ascending per file, chunks of the stated size).  Built with AddressSanitizer + UBSan.
// No GPU.
#include <cstdio>
#include <cstdlib>
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

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 500;
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

  std::printf("fill checkpoint ok: %d sessions, %d failures\n", rounds, failures);
  return failures ? 1 : 0;
}
