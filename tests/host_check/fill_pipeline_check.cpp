// CPU check of the ingestion pipe's HOST side (csrc/fill_pipeline.hpp: the very class IngestPipe uses): real slot files in a scratch
// directory, turns cut by csrc/ingest_turns.hpp, fills posted TWO TURNS DEEP on several threads into a ring of exactly-sized heap
// buffers, every turn's bytes compared with the reference's own way of reading a cell (slot.nim:57-68: seek cellSize * idx, read
// cellSize bytes, what the file does not hold is zero) -- short files, a missing file (reported by name, the lowest slot first),
// slots cut into units, O_DIRECT requested, and the host-array source (memcpy).  Then the read rule (fill_pipeline.hpp) through an
// injected reader (slot_file_read): EIO on a piece's first read, after a partial read, in a turn's last grain, in two slots at once
// (the lowest named); EIO / EINVAL from O_DIRECT reads (the buffered reads finish the piece); EINTR; 1-byte reads -- and a real
// directory in place of a slot file; the same cases through the per-cell reader (read_file_cell).  Built twice by the CPU suite: with
// -fsanitize=address,undefined (a byte outside a ring buffer, a use after a turn was joined) and with -fsanitize=thread (the grain
// counter, the completion count, the error slot: workers run on into the next turn while the building thread joins this one).
//   g++ -std=c++17 -pthread -fsanitize=... -I<csrc> fill_pipeline_check.cpp -o check && ./check <scratch dir> [shapes]
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "fill_pipeline.hpp"

using namespace cp2i;

static uint64_t rng_state = 0x853c49e6748fea9bULL;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// byte x of slot file `slot` as written below: a function of (slot, x), never zero, so that zero-fill is distinguishable
static uint8_t file_byte(uint64_t slot, size_t x) { return (uint8_t)(1 + ((slot * 131 + x * 7 + (x >> 9)) % 251)); }

constexpr size_t MISSING = (size_t)-1, DIRECTORY = (size_t)-2;

struct Dataset {
  std::string base;
  std::vector<size_t> file_bytes;   // per slot; MISSING: the file does not exist, DIRECTORY: a directory of that name is there
};

// ---- the injected reader (fill_pipeline.hpp: slot_file_read).  Set up before the fill threads start; read-only while they run.
struct Fault {
  enum Kind { NONE, FAIL, PARTIAL_THEN_FAIL, DIRECT_FAIL, INTR_ONCE, INTR_MANY, SHORT1 } kind = NONE;
  int n_rules = 0;                       // FAIL: reads of slot[i] that cover file byte at[i] fail with `err`, after delay_ms[i]
  uint64_t slot[2] = {~0ULL, ~0ULL}, at[2] = {0, 0};
  int grain[2] = {-2, -2};               // FAIL: >= -1: at[i] / slot[i] are set to the middle of grain grain[i] of turn 0 (-1: its last)
  unsigned delay_ms[2] = {0, 0};
  int err = EIO;                         // FAIL; DIRECT_FAIL: EIO (after some whole blocks) or EINVAL (at once)
};
static Fault fault;
static std::vector<ino_t> slot_inode;   // slot -> inode of its file (0: none)
static std::atomic<long> injected{0};   // reads the injection changed: a case where nothing was injected proves nothing
static std::atomic<uint64_t> partial_end{~0ULL};
static std::atomic<bool> intr_done{false};

static long slot_of(int fd) {
  struct stat sb;
  if (fstat(fd, &sb) != 0) return -1;
  for (size_t s = 0; s < slot_inode.size(); ++s)
    if (slot_inode[s] && slot_inode[s] == sb.st_ino) return (long)s;
  return -1;
}

static ssize_t injected_pread(int fd, void* buf, size_t n, off_t off) {
  const Fault& f = fault;
  if (f.kind == Fault::NONE) return ::pread(fd, buf, n, off);
  const long slot = slot_of(fd);
  const bool direct = (fcntl(fd, F_GETFL) & O_DIRECT) != 0;
  switch (f.kind) {
    case Fault::FAIL:
      for (int i = 0; i < f.n_rules; ++i)
        if (slot >= 0 && (uint64_t)slot == f.slot[i] && (uint64_t)off <= f.at[i] && f.at[i] < (uint64_t)off + n) {
          if (f.delay_ms[i]) std::this_thread::sleep_for(std::chrono::milliseconds(f.delay_ms[i]));
          ++injected;
          errno = f.err;
          return -1;
        }
      break;
    case Fault::PARTIAL_THEN_FAIL:   // the first read of the file's first piece returns half of what it asked for, the next one fails
      if (slot >= 0 && (uint64_t)slot == f.slot[0]) {
        if (off == 0 && n >= 2) {
          const ssize_t r = ::pread(fd, buf, n / 2, 0);
          if (r > 0) { partial_end.store((uint64_t)r); ++injected; }
          return r;
        }
        if ((uint64_t)off == partial_end.load()) { ++injected; errno = EIO; return -1; }
      }
      break;
    case Fault::DIRECT_FAIL:
      if (direct) {
        if (f.err == EIO && n > FillPipeline::DIRECT_ALIGN) return ::pread(fd, buf, FillPipeline::DIRECT_ALIGN, off);   // whole blocks first ...
        ++injected;                                                                                                 // ... then a failure
        errno = f.err;
        return -1;
      }
      break;
    case Fault::INTR_ONCE:
      if (slot >= 0 && (uint64_t)slot == f.slot[0] && !intr_done.exchange(true)) { ++injected; errno = EINTR; return -1; }
      break;
    case Fault::INTR_MANY: {         // every read is interrupted three times before it goes through
      static thread_local unsigned k = 0;
      if (k++ % 4 != 3) { ++injected; errno = EINTR; return -1; }
      break;
    }
    case Fault::SHORT1:
      if (n > 1) { ++injected; n = 1; }
      break;
    default:
      break;
  }
  return ::pread(fd, buf, n, off);
}

static void write_files(Dataset& d, size_t n_slots, size_t slot_bytes, int short_every, int missing_slot, int dir_slot = -1) {
  d.file_bytes.assign(n_slots, 0);
  slot_inode.assign(n_slots, 0);
  for (size_t s = 0; s < n_slots; ++s) {
    const std::string name = fill_slot_file_name(d.base, s);
    if ((int)s == missing_slot) { unlink(name.c_str()); d.file_bytes[s] = MISSING; continue; }
    if ((int)s == dir_slot) {
      unlink(name.c_str());
      if (mkdir(name.c_str(), 0700) != 0) { std::printf("FAILED: cannot make directory %s\n", name.c_str()); std::exit(2); }
      d.file_bytes[s] = DIRECTORY;
      continue;
    }
    size_t len = slot_bytes;
    if (short_every && s % (size_t)short_every == 1) len = slot_bytes / 2 + (rnd() % 7);     // a file that ends early, not on a cell boundary
    std::vector<uint8_t> v(len);
    for (size_t x = 0; x < len; ++x) v[x] = file_byte(s, x);
    FILE* f = std::fopen(name.c_str(), "wb");
    if (!f || std::fwrite(v.data(), 1, len, f) != len) { std::printf("FAILED: cannot write %s\n", name.c_str()); std::exit(2); }
    std::fclose(f);
    d.file_bytes[s] = len;
    struct stat sb;
    if (stat(name.c_str(), &sb) == 0) slot_inode[s] = sb.st_ino;
  }
}

// the reference's read of one cell of a slot (slot.nim:57-68), from what the files hold
static void reference_cell(const Dataset& d, uint64_t slot, size_t cell_in_slot, size_t cell_size, uint8_t* out) {
  const size_t have = (d.file_bytes[slot] == MISSING || d.file_bytes[slot] == DIRECTORY) ? 0 : d.file_bytes[slot];
  for (size_t b = 0; b < cell_size; ++b) {
    const size_t x = cell_in_slot * cell_size + b;
    out[b] = x < have ? file_byte(slot, x) : 0;
  }
}

static long check_shape(const std::string& dir, size_t n_slots_files, size_t cells_per_slot, size_t cell_size, uint64_t units_per_slot, size_t chunk_bytes,
                        int threads, int ring, bool direct, int short_every, int missing_slot, uint64_t first_unit, size_t n_units, long* bytes,
                        int dir_slot = -1, long* reported = nullptr) {
  Dataset d;
  d.base = dir + "/s";
  write_files(d, n_slots_files, cells_per_slot * cell_size, short_every, missing_slot, dir_slot);
  IngestGeom g;
  g.n_units = n_units; g.n_cells = cells_per_slot / units_per_slot; g.cell_size = cell_size; g.first_unit = first_unit; g.units_per_slot = units_per_slot;
  const size_t total = g.total_cells();
  const size_t chunk = ingest_chunk_cells(chunk_bytes, cell_size, total);
  const size_t cell_multiple = direct ? [&] { size_t a = cell_size, h = 4096; while (h) { size_t r = a % h; a = h; h = r; } return (size_t)4096 / a; }() : 1;
  auto fail = [&](const char* what, size_t turn, size_t at) {
    std::printf("FAILED: %s (files %zu x %zu cells of %zu B, units/slot %llu, first unit %llu, %zu units, chunk %zu B, threads %d, ring %d, direct %d, short every %d, missing %d, directory %d, fault %d: turn %zu, byte %zu)\n",
                what, n_slots_files, cells_per_slot, cell_size, (unsigned long long)units_per_slot, (unsigned long long)first_unit, n_units, chunk_bytes, threads, ring, (int)direct,
                short_every, missing_slot, dir_slot, (int)fault.kind, turn, at);
    std::exit(1);
  };
  // a rule placed in a grain of turn 0: the middle byte of that grain, as a (slot, file byte) pair
  for (int i = 0; i < fault.n_rules; ++i) {
    if (fault.grain[i] < -1) continue;
    const size_t m0 = ingest_turn_cells(g, chunk, cell_multiple, 0, 0), nb = m0 * cell_size, ng = ingest_grain_count(nb, INGEST_FILL_GRAIN);
    size_t a = 0, b = 0;
    ingest_grain(nb, INGEST_FILL_GRAIN, fault.grain[i] < 0 ? ng - 1 : (size_t)fault.grain[i], &a, &b);
    const size_t x = a + (b - a) / 2, cell = x / cell_size, unit = cell / g.n_cells;
    const uint64_t u = g.first_unit + unit;
    fault.slot[i] = u / g.units_per_slot;
    fault.at[i] = ((u % g.units_per_slot) * g.n_cells + cell % g.n_cells) * cell_size + x % cell_size;
    if (ng < 2) fail("a grain case on a turn of one grain", 0, 0);
  }
  const bool rule_fault = fault.kind == Fault::FAIL || fault.kind == Fault::PARTIAL_THEN_FAIL;
  // which slot a missing-file report must name: the lowest missing slot among the files a turn touches
  // ring buffers of EXACTLY a turn's size (ASan sees a byte beyond it), 4 KiB aligned like the pinned ring: O_DIRECT reads happen
  struct Buf {
    uint8_t* p = nullptr;
    ~Buf() { std::free(p); }
    uint8_t* data() { return p; }
    void assign(size_t n, uint8_t v) {
      std::free(p);
      p = nullptr;
      if (posix_memalign(reinterpret_cast<void**>(&p), FillPipeline::DIRECT_ALIGN, n) != 0) { std::printf("FAILED: out of memory\n"); std::exit(2); }
      std::memset(p, v, n);
    }
  };
  std::vector<Buf> bufs((size_t)ring);
  struct Posted { size_t c0, m; int b; };
  std::deque<Posted> posted;
  long turns = 0;
  {
    FillPipeline fill(threads);
    size_t c_next = 0, turn_posted = 0;
    auto post = [&] {
      const size_t m = ingest_turn_cells(g, chunk, cell_multiple, turn_posted, c_next);
      if (m == 0 || m > chunk || c_next + m > total) fail("turn outside the batch or its buffer", turn_posted, 0);
      const int b = (int)(turn_posted % (size_t)ring);
      bufs[(size_t)b].assign(m * cell_size, 0xEE);
      fill.begin(g, d.base, c_next, m, bufs[(size_t)b].data(), direct);
      posted.push_back({c_next, m, b});
      c_next += m;
      ++turn_posted;
    };
    post();
    while (!posted.empty()) {
      if (c_next < total && (int)posted.size() < ring && posted.size() < 2) post();   // two turns deep, like the builder (and never into a buffer still posted)
      const Posted p = posted.front();
      posted.pop_front();
      std::string bad;
      int err = -1;
      const bool ok = fill.join(&bad, &err);
      // what the reference reads for these cells; which slot the turn must report (missing file, directory, failing read), and how
      std::vector<uint8_t> want(cell_size);
      bool touches_missing = false;
      uint64_t lowest_missing = ~0ULL;
      int want_err = 0;
      std::vector<uint64_t> read_failed;   // slots whose reads fail in this turn: their bytes are not the reference's (nor used)
      for (size_t c = 0; c < p.m; ++c) {
        const size_t cell = p.c0 + c, unit = cell / g.n_cells, in_unit = cell % g.n_cells;
        const uint64_t u = g.first_unit + unit, slot = u / g.units_per_slot;
        const size_t cell_in_slot = (size_t)(u % g.units_per_slot) * g.n_cells + in_unit;
        int e = -1;
        if (d.file_bytes[slot] == MISSING) e = 0;
        else if (d.file_bytes[slot] == DIRECTORY) e = EISDIR;
        else if (rule_fault)
          for (int i = 0; i < std::max(1, fault.n_rules); ++i)
            if (slot == fault.slot[i] && cell_in_slot == (fault.kind == Fault::FAIL ? fault.at[i] / cell_size : 0)) {
              e = fault.kind == Fault::FAIL ? fault.err : EIO;
              read_failed.push_back(slot);
            }
        if (e >= 0) { touches_missing = true; if (slot < lowest_missing) { lowest_missing = slot; want_err = e; } }
      }
      for (size_t c = 0; c < p.m; ++c) {
        const size_t cell = p.c0 + c, unit = cell / g.n_cells, in_unit = cell % g.n_cells;
        const uint64_t u = g.first_unit + unit, slot = u / g.units_per_slot;
        const size_t cell_in_slot = (size_t)(u % g.units_per_slot) * g.n_cells + in_unit;
        if (std::find(read_failed.begin(), read_failed.end(), slot) != read_failed.end()) continue;
        reference_cell(d, slot, cell_in_slot, cell_size, want.data());
        if (std::memcmp(want.data(), bufs[(size_t)p.b].data() + c * cell_size, cell_size) != 0) fail("a cell's bytes differ from the reference's read of the slot file", (size_t)turns, c * cell_size);
      }
      if (ok == touches_missing) fail(ok ? "a turn that touches a missing file, a directory or a failing read was not reported" : "a turn reported a file it does not touch or reads fine", (size_t)turns, 0);
      if (!ok && bad != fill_slot_file_name(d.base, lowest_missing)) fail("the file reported is not the one of the lowest slot", (size_t)turns, 0);
      if (!ok && err != want_err) fail("the error reported is not the one met (0: cannot open, else the errno of the read)", (size_t)turns, (size_t)err);
      if (!ok && reported) ++*reported;
      *bytes += (long)(p.m * cell_size);
      ++turns;
    }
    if (!fill.idle()) fail("fills left posted", (size_t)turns, 0);
  }
  for (size_t s = 0; s < n_slots_files; ++s) (d.file_bytes[s] == DIRECTORY ? rmdir : unlink)(fill_slot_file_name(d.base, s).c_str());
  return turns;
}

// O_DIRECT cases only reach the O_DIRECT reads where the scratch file system takes O_DIRECT (tmpfs does not)
static bool direct_supported(const std::string& dir) {
  const std::string name = dir + "/direct_probe";
  FILE* f = std::fopen(name.c_str(), "wb");
  if (!f) return false;
  std::fclose(f);
  const int fd = open(name.c_str(), O_RDONLY | O_DIRECT);
  if (fd >= 0) close(fd);
  unlink(name.c_str());
  return fd >= 0;
}

// The read rule through the pipe: one case per way a read goes wrong (or right after all).  Returns the number of cases.
static long check_read_faults(const std::string& dir, long* turns, long* bytes, long* reported) {
  const bool can_direct = direct_supported(dir);
  const size_t big = ((size_t)8 << 20) / 4096 + 1;                 // cells of 4 KiB per file: 8 MiB + 4 KiB, a 13 MiB turn is 4 grains
  struct Case {
    const char* name;
    Fault f;
    size_t files, cells, cs, chunk;
    int threads, ring;
    bool direct, expect_report;
  };
  auto rule = [](uint64_t slot, uint64_t at, int grain = -2, unsigned delay = 0) { Fault f; f.kind = Fault::FAIL; f.n_rules = 1; f.slot[0] = slot; f.at[0] = at; f.grain[0] = grain; f.delay_ms[0] = delay; return f; };
  auto kind = [](Fault::Kind k, uint64_t slot = ~0ULL, int err = EIO) { Fault f; f.kind = k; f.slot[0] = slot; f.err = err; return f; };
  Fault two = rule(0, 0, 0, 30);                                   // slot of grain 0 fails late, slot of the last grain at once
  two.n_rules = 2; two.grain[1] = -1;
  const Case cases[] = {
    {"EIO on the first read of a piece", rule(3, 0), 7, 64, 256, 3 * 64 * 256 + 1000, 4, 3, false, true},
    {"EIO on the first read, several slots a turn", rule(5, 0), 12, 32, 100, 5 * 32 * 100, 1, 2, false, true},
    {"EIO after a partial read mid-piece", kind(Fault::PARTIAL_THEN_FAIL, 4), 9, 128, 64, 4 * 128 * 64 + 64, 3, 2, false, true},
    {"EIO in a turn's last grain", rule(0, 0, -1), 3, big, 4096, (size_t)13 << 20, 4, 2, false, true},
    {"EIO in two slots on different threads", two, 3, big, 4096, (size_t)13 << 20, 4, 2, false, true},
    {"EIO from O_DIRECT, buffered retry", kind(Fault::DIRECT_FAIL, ~0ULL, EIO), 5, 64, 4096, 3 * 64 * 4096, 3, 3, true, false},
    {"EINVAL from O_DIRECT, buffered fallback", kind(Fault::DIRECT_FAIL, ~0ULL, EINVAL), 5, 64, 2048, 2 * 64 * 2048, 2, 2, true, false},
    {"EINTR once", kind(Fault::INTR_ONCE, 2), 6, 64, 256, 2 * 64 * 256, 3, 2, false, false},
    {"EINTR repeatedly", kind(Fault::INTR_MANY), 6, 64, 256, 2 * 64 * 256 + 512, 5, 3, true, false},
    {"1-byte short reads", kind(Fault::SHORT1), 4, 16, 100, 3 * 16 * 100, 3, 2, false, false},
  };
  long n = 0;
  for (const Case& c : cases) {
    fault = c.f;
    injected = 0;
    partial_end = ~0ULL;
    intr_done = false;
    long rep = 0;
    *turns += check_shape(dir, c.files, c.cells, c.cs, 1, c.chunk, c.threads, c.ring, c.direct, 0, -1, 0, c.files, bytes, -1, &rep);
    const bool direct_case = c.f.kind == Fault::DIRECT_FAIL;
    if (injected.load() == 0 && !(direct_case && !can_direct)) { std::printf("FAILED: %s: nothing was injected\n", c.name); std::exit(1); }
    if ((rep > 0) != c.expect_report) { std::printf("FAILED: %s: %ld turn(s) reported\n", c.name, rep); std::exit(1); }
    *reported += rep;
    ++n;
  }
  fault = Fault();
  // no injection: a real DIRECTORY in place of a slot file -- open() succeeds, every read fails with EISDIR
  for (int direct = 0; direct < 2; ++direct)
    for (int dir_slot : {0, 2, 5}) {
      long rep = 0;
      *turns += check_shape(dir, 6, 64, 2048, 1, (size_t)3 * 64 * 2048 / 2, 1 + dir_slot % 4, 2 + direct, direct != 0, 0, -1, 0, 6, bytes, dir_slot, &rep);
      if (rep == 0) { std::printf("FAILED: a directory in place of slot %d was not reported\n", dir_slot); std::exit(1); }
      *reported += rep;
      ++n;
    }
  return n;
}

// The same rule through the per-cell reader the proof-input paths use (read_file_cell): cell after cell of one file of 5.5 cells.
static long check_cell_reader(const std::string& dir) {
  const size_t cs = 100, n_cells = 7;
  Dataset d;
  d.base = dir + "/c";
  write_files(d, 1, 5 * cs + cs / 2, 0, -1);
  const std::string name = fill_slot_file_name(d.base, 0);
  struct Case { const char* name; Fault f; int want_err; };   // want_err: the errno cell 0 must return (0: every cell reads right)
  auto mk = [](Fault::Kind k, int n_rules = 0) { Fault f; f.kind = k; f.n_rules = n_rules; f.slot[0] = 0; f.at[0] = 0; return f; };
  const Case cases[] = {
    {"clean", mk(Fault::NONE), 0},
    {"EIO on the first read", mk(Fault::FAIL, 1), EIO},
    {"EIO after a partial read", mk(Fault::PARTIAL_THEN_FAIL), EIO},
    {"EINTR once", mk(Fault::INTR_ONCE), 0},
    {"EINTR repeatedly", mk(Fault::INTR_MANY), 0},
    {"1-byte short reads", mk(Fault::SHORT1), 0},
  };
  long n = 0;
  std::vector<uint8_t> got(cs), want(cs);
  for (const Case& c : cases) {
    fault = c.f;
    injected = 0;
    partial_end = ~0ULL;
    intr_done = false;
    const int fd = open(name.c_str(), O_RDONLY);
    if (fd < 0) { std::printf("FAILED: cannot open %s\n", name.c_str()); std::exit(2); }
    for (size_t cell = 0; cell < n_cells; ++cell) {
      std::memset(got.data(), 0xEE, cs);
      const int err = read_file_cell(fd, cs, cell, got.data());
      const int want_err = cell == 0 ? c.want_err : 0;
      if (err != want_err) { std::printf("FAILED: cell reader, %s: cell %zu returned %d, not %d\n", c.name, cell, err, want_err); std::exit(1); }
      reference_cell(d, 0, cell, cs, want.data());
      if (!err && got != want) { std::printf("FAILED: cell reader, %s: cell %zu differs from the reference's read\n", c.name, cell); std::exit(1); }
    }
    close(fd);
    if (c.f.kind != Fault::NONE && injected.load() == 0) { std::printf("FAILED: cell reader, %s: nothing was injected\n", c.name); std::exit(1); }
    ++n;
  }
  fault = Fault();
  const std::string text = slot_file_error(name, EIO);
  if (text != "cannot read " + name + ": " + std::strerror(EIO) || slot_file_error(name, 0) != "cannot open " + name) {
    std::printf("FAILED: the error text is \"%s\"\n", text.c_str());
    std::exit(1);
  }
  unlink(name.c_str());
  // a directory: open() succeeds, the read fails with EISDIR -- an error, not a cell of zeros
  if (mkdir(name.c_str(), 0700) != 0) { std::printf("FAILED: cannot make directory %s\n", name.c_str()); std::exit(2); }
  const int fd = open(name.c_str(), O_RDONLY);
  const int err = fd >= 0 ? read_file_cell(fd, cs, 0, got.data()) : -1;
  if (fd >= 0) close(fd);
  rmdir(name.c_str());
  if (err != EISDIR) { std::printf("FAILED: cell reader on a directory returned %d, not EISDIR\n", err); std::exit(1); }
  return n + 1;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: fill_pipeline_check <scratch dir> [shapes]\n"); return 2; }
  const std::string dir = argv[1];
  const long want = argc > 2 ? std::atol(argv[2]) : 300;
  long shapes = 0, turns = 0, bytes = 0, with_missing = 0, with_units = 0, multi_file = 0;
  const size_t cell_sizes[] = {31, 64, 100, 256, 2048, 4096};
  while (shapes < want) {
    const size_t cs = cell_sizes[rnd() % 6];
    const uint64_t ups = (rnd() % 4 == 0) ? (uint64_t)1 << (1 + rnd() % 2) : 1;
    size_t cells_per_slot = ((size_t)1 << (rnd() % 9)) * ups;                  // 1 .. 256 cells per unit
    const size_t n_files = 1 + rnd() % 24;
    const size_t all_units = n_files * ups;
    const uint64_t first_unit = (rnd() % 3 == 0) ? rnd() % all_units : 0;
    const size_t n_units = 1 + rnd() % (all_units - first_unit);
    const size_t data = n_units * (cells_per_slot / ups) * cs;
    // chunk sizes from a fraction of a unit to several files; grains are 4 MiB in the product, so most turns here are ONE grain:
    // every sixth shape is made large enough for several grains per turn (8 ... 40 MiB of data)
    size_t chunk_bytes = std::max<size_t>(cs, data / (1 + rnd() % 9));
    if (shapes % 6 == 5) { cells_per_slot = (((size_t)8 << 20) / cs / ups + 1) * ups; chunk_bytes = (size_t)13 << 20; }
    const int threads = 1 + (int)(rnd() % 8), ring = 2 + (int)(rnd() % 3);
    const bool direct = rnd() % 3 == 0;
    const int short_every = (rnd() % 3 == 0) ? 2 + (int)(rnd() % 3) : 0;
    const int missing = (rnd() % 5 == 0) ? (int)(rnd() % n_files) : -1;
    size_t units_now = n_units, first_now = (size_t)first_unit;
    if (shapes % 6 == 5) { units_now = std::min<size_t>(n_units, 3 * ups); first_now = 0; }
    turns += check_shape(dir, n_files, cells_per_slot, cs, ups, chunk_bytes, threads, ring, direct, short_every, missing, first_now, units_now, &bytes);
    ++shapes;
    with_missing += missing >= 0;
    with_units += ups > 1;
    multi_file += chunk_bytes >= 2 * (cells_per_slot / ups) * cs;
  }
  // the host-array source: memcpy from a caller's array, turns two deep
  {
    const size_t cs = 2048, n = 9000;
    std::vector<uint8_t> src(n * cs);
    for (size_t x = 0; x < src.size(); ++x) src[x] = (uint8_t)(x * 31 + (x >> 11));
    IngestGeom g;
    g.n_units = 1; g.n_cells = n; g.cell_size = cs;
    const size_t chunk = ingest_chunk_cells((size_t)5 << 20, cs, n);
    FillPipeline fill(6);
    std::vector<uint8_t> out(src.size(), 0), b0, b1;
    size_t c0 = 0, turn = 0;
    size_t m = ingest_turn_cells(g, chunk, 1, turn, c0);
    b0.assign(m * cs, 0);
    fill.begin(g, "", c0, m, b0.data(), false, src.data());
    while (c0 < n) {
      const size_t c1 = c0 + m;
      size_t m_next = 0;
      std::vector<uint8_t>& cur = (turn & 1) ? b1 : b0;
      std::vector<uint8_t>& nxt = (turn & 1) ? b0 : b1;
      if (c1 < n) {
        m_next = ingest_turn_cells(g, chunk, 1, turn + 1, c1);
        nxt.assign(m_next * cs, 0);
        fill.begin(g, "", c1, m_next, nxt.data(), false, src.data() + c1 * cs);
      }
      if (!fill.join(nullptr)) { std::printf("FAILED: host-array fill reported a file\n"); return 1; }
      std::memcpy(out.data() + c0 * cs, cur.data(), m * cs);
      c0 = c1; m = m_next; ++turn;
    }
    if (out != src) { std::printf("FAILED: host-array turns do not reproduce the array\n"); return 1; }
    bytes += (long)src.size();
  }
  if (!with_missing || !with_units || !multi_file) { std::printf("FAILED: the walk missed a case (missing %ld, units %ld, multi-file %ld)\n", with_missing, with_units, multi_file); return 1; }
  // the read rule, through the injected reader
  slot_file_read = injected_pread;
  long reported = 0;
  const long fault_cases = check_read_faults(dir, &turns, &bytes, &reported);
  const long cell_cases = check_cell_reader(dir);
  slot_file_read = ::pread;
  std::printf("fill pipeline ok: %ld shapes, %ld turns, %ld bytes compared with the reference's reads; %ld shapes with a missing file, %ld cut into units, %ld with turns of several files; host-array source reproduced\n",
              shapes, turns, bytes, with_missing, with_units, multi_file);
  std::printf("read rule ok: %ld pipe cases (%ld failing turns reported with the file of the lowest slot and its errno), %ld cell-reader cases\n", fault_cases, reported, cell_cases);
  return 0;
}
