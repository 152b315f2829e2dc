// CPU check of the ingestion pipe's host side filling turns from a NAME TABLE (csrc/fill_pipeline.hpp: FillPipeline::begin with
// `names`; what trees_build_file_list hands it): unit i of a batch is the whole file names[i], whatever it is called and wherever it
// lies.  Real temporary files of unequal lengths in a scratch directory -- short (ends early, not on a cell boundary), exact, long
// (bytes past the unit, never read) and missing -- under names that share no base and are listed in shuffled order, some files listed
// twice; turns cut by csrc/ingest_turns.hpp exactly as the builder cuts them for a listed batch (first unit 0, one unit per file),
// posted two turns deep on several threads into ring buffers of exactly a turn's size, O_DIRECT requested or not.  Every buffer is
// compared with a PLAIN READ of the listed file (open, pread at cell * cell_size, zeros past the end: slot.nim:57-68).  A short file
// reads as zeros past its end; a turn that touches a missing file fails its join and names that file -- the one of the lowest unit
// when it touches several.  Built twice by the CPU suite: -fsanitize=address,undefined and -fsanitize=thread.
//   g++ -std=c++17 -pthread -fsanitize=... -I<csrc> fill_names_check.cpp -o check && ./check <scratch dir> [shapes]
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "fill_pipeline.hpp"

using namespace cp2i;

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// byte x of file f: never zero, so that zero-fill is distinguishable
static uint8_t file_byte(size_t f, size_t x) { return (uint8_t)(1 + ((f * 197 + x * 11 + (x >> 7)) % 251)); }

[[noreturn]] static void die(const char* what, size_t shape, size_t turn, size_t at) {
  std::printf("FAILED: %s (shape %zu, turn %zu, at %zu)\n", what, shape, turn, at);
  std::exit(1);
}

// the plain read: cell `cell` of the file `name`, zeros where the file does not reach
static bool plain_read_cell(const std::string& name, size_t cell, size_t cell_size, uint8_t* out) {
  std::memset(out, 0, cell_size);
  const int fd = open(name.c_str(), O_RDONLY);
  if (fd < 0) return false;
  size_t pos = 0;
  while (pos < cell_size) {
    const ssize_t r = ::pread(fd, out + pos, cell_size - pos, (off_t)(cell * cell_size + pos));
    if (r <= 0) break;
    pos += (size_t)r;
  }
  close(fd);
  return true;
}

struct Buf {
  uint8_t* p = nullptr;
  ~Buf() { std::free(p); }
  void assign(size_t n, uint8_t v) {
    std::free(p);
    p = nullptr;
    if (posix_memalign(reinterpret_cast<void**>(&p), FillPipeline::DIRECT_ALIGN, n) != 0) { std::printf("FAILED: out of memory\n"); std::exit(2); }
    std::memset(p, v, n);
  }
};

// one shape: n_files files, a table of n_units names over them; returns the turns walked
static long check_shape(const std::string& dir, size_t shape, size_t n_files, size_t n_units, size_t n_cells, size_t cell_size, size_t chunk_bytes,
                        int threads, int ring, bool direct, long* bytes, long* reported, long* short_cells) {
  const size_t unit_bytes = n_cells * cell_size;
  // the files: kind by index -- 0 exact, 1 short, 2 long, 3 missing (one in four or so), names with nothing in common but the directory
  std::vector<std::string> file_name(n_files);
  std::vector<long> file_len(n_files);   // -1: missing
  for (size_t f = 0; f < n_files; ++f) {
    const char* stem[] = {"alpha_", "b", "slot-of-dataset-", "x.y.z."};
    file_name[f] = dir + "/" + stem[rnd() % 4] + std::to_string(shape) + "_" + std::to_string(rnd() % 1000000) + "_" + std::to_string(f) + (f % 2 ? ".dat" : ".bin");
    const unsigned kind = n_files >= 4 ? (unsigned)(f % 4) : (unsigned)(rnd() % 3);
    size_t len = unit_bytes;
    if (kind == 1) len = unit_bytes / 2 + (size_t)(rnd() % 7);
    if (kind == 2) len = unit_bytes + 1 + (size_t)(rnd() % 300);
    if (kind == 3 && rnd() % 2) { unlink(file_name[f].c_str()); file_len[f] = -1; continue; }
    std::vector<uint8_t> v(len);
    for (size_t x = 0; x < len; ++x) v[x] = file_byte(f, x);
    FILE* fp = std::fopen(file_name[f].c_str(), "wb");
    if (!fp || std::fwrite(v.data(), 1, len, fp) != len) { std::printf("FAILED: cannot write %s\n", file_name[f].c_str()); std::exit(2); }
    std::fclose(fp);
    file_len[f] = (long)len;
  }
  // the table: shuffled, with repeats when there are more units than files
  std::vector<size_t> unit_file(n_units);
  for (size_t i = 0; i < n_units; ++i) unit_file[i] = i < n_files ? i : (size_t)(rnd() % n_files);
  for (size_t i = n_units; i > 1; --i) std::swap(unit_file[i - 1], unit_file[rnd() % i]);
  std::vector<std::string> names(n_units);
  for (size_t i = 0; i < n_units; ++i) names[i] = file_name[unit_file[i]];

  IngestGeom g;
  g.n_units = n_units; g.n_cells = n_cells; g.cell_size = cell_size; g.first_unit = 0; g.units_per_slot = 1;
  const size_t total = g.total_cells();
  const size_t chunk = ingest_chunk_cells(chunk_bytes, cell_size, total);
  const size_t cell_multiple = direct ? [&] { size_t a = cell_size, h = 4096; while (h) { size_t r = a % h; a = h; h = r; } return (size_t)4096 / a; }() : 1;
  std::vector<Buf> bufs((size_t)ring);
  struct Posted { size_t c0, m; int b; };
  std::deque<Posted> posted;
  long turns = 0;
  {
    FillPipeline fill(threads);
    const std::string no_base = "/nonexistent/base/that/must/never/be/used";
    size_t c_next = 0, turn_posted = 0;
    auto post = [&] {
      const size_t m = ingest_turn_cells(g, chunk, cell_multiple, turn_posted, c_next);
      if (m == 0 || m > chunk || c_next + m > total) die("turn outside the batch or its buffer", shape, turn_posted, 0);
      const int b = (int)(turn_posted % (size_t)ring);
      bufs[(size_t)b].assign(m * cell_size, 0xEE);
      fill.begin(g, no_base, c_next, m, bufs[(size_t)b].p, direct, nullptr, names.data());
      posted.push_back({c_next, m, b});
      c_next += m;
      ++turn_posted;
    };
    post();
    std::vector<uint8_t> want(cell_size);
    while (!posted.empty()) {
      if (c_next < total && (int)posted.size() < ring && posted.size() < 2) post();
      const Posted p = posted.front();
      posted.pop_front();
      std::string bad;
      int err = -1;
      const bool ok = fill.join(&bad, &err);
      size_t lowest_missing = (size_t)-1;
      for (size_t c = 0; c < p.m; ++c) {
        const size_t cell = p.c0 + c, unit = cell / n_cells, in_unit = cell % n_cells;
        const bool there = plain_read_cell(names[unit], in_unit, cell_size, want.data());
        if (!there && unit < lowest_missing) lowest_missing = unit;
        if (std::memcmp(want.data(), bufs[(size_t)p.b].p + c * cell_size, cell_size) != 0) die("a cell's bytes differ from a plain read of the listed file", shape, (size_t)turns, c * cell_size);
        // (what a short file must give, stated without the file system: its own bytes, then zeros)
        const long len = file_len[unit_file[unit]];
        for (size_t b = 0; b < cell_size; ++b) {
          const size_t x = in_unit * cell_size + b;
          const uint8_t w = len >= 0 && x < (size_t)len ? file_byte(unit_file[unit], x) : 0;
          if (bufs[(size_t)p.b].p[c * cell_size + b] != w) die("a byte is neither the file's nor the zero past its end", shape, (size_t)turns, c * cell_size + b);
        }
        if (len >= 0 && (in_unit + 1) * cell_size > (size_t)len) ++*short_cells;
      }
      const bool touches_missing = lowest_missing != (size_t)-1;
      if (ok == touches_missing) die(ok ? "a turn that touches a missing file was not reported" : "a turn reported a file that is there", shape, (size_t)turns, 0);
      if (!ok && bad != names[lowest_missing]) die("the file named is not the one of the lowest unit that is missing", shape, (size_t)turns, lowest_missing);
      if (!ok && err != 0) die("a missing file must be reported as not opened (errno 0)", shape, (size_t)turns, (size_t)err);
      if (!ok && slot_file_error(bad, err).find(names[lowest_missing]) == std::string::npos) die("the message does not name the file", shape, (size_t)turns, 0);
      if (!ok) ++*reported;
      *bytes += (long)(p.m * cell_size);
      ++turns;
    }
    if (!fill.idle()) die("fills left posted", shape, (size_t)turns, 0);
  }
  for (size_t f = 0; f < n_files; ++f) unlink(file_name[f].c_str());
  return turns;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s <scratch dir> [shapes]\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  const long shapes = argc > 2 ? std::atol(argv[2]) : 60;
  long turns = 0, bytes = 0, reported = 0, short_cells = 0;
  for (long s = 0; s < shapes; ++s) {
    // small files many to a turn, files larger than a turn, and a turn of several grains (> 4 MiB) every eighth shape
    const bool big = s % 8 == 7;
    static const size_t small_cells[5] = {64, 100, 512, 2048, 31};
    const size_t cell_size = big ? 4096 : small_cells[rnd() % 5];
    const size_t n_cells = big ? 520 + rnd() % 9 : 1 + rnd() % 40;
    const size_t n_files = big ? 3 + rnd() % 3 : 1 + rnd() % 12;
    const size_t n_units = n_files + rnd() % 4;
    const size_t unit_bytes = n_cells * cell_size;
    const size_t chunk_bytes = big ? ((size_t)5 << 20) + rnd() % 4096 : std::max<size_t>(cell_size, (size_t)(rnd() % (3 * unit_bytes + 1)));
    const int threads = 1 + (int)(rnd() % 5), ring = 2 + (int)(rnd() % 2);
    turns += check_shape(dir, (size_t)s, n_files, n_units, n_cells, cell_size, chunk_bytes, threads, ring, rnd() % 2 != 0, &bytes, &reported, &short_cells);
  }
  if (reported == 0 || short_cells == 0) { std::printf("FAILED: no missing file (%ld) or no short file (%ld) was met: the shapes prove nothing\n", reported, short_cells); return 1; }
  std::printf("fill names ok: %ld shapes, %ld turns, %ld bytes compared with a plain read, %ld turns named a missing file, %ld cells past a short file's end\n",
              shapes, turns, bytes, reported, short_cells);
  return 0;
}
