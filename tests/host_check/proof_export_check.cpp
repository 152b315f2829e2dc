// CPU check of what the proof-input routes share (csrc/proof_export.hpp and slot_file_read_list of csrc/fill_pipeline.hpp), the very
// headers the product compiles.  No GPU, no HIP; built with AddressSanitizer + UBSan and again with ThreadSanitizer
// (tests/test_host_check.py).
//
//   proof_export_check run <scratch dir>
//     slot_file_read_list against real files (a full file, one that ends inside a piece and before one, a missing file, a directory,
//       zero pieces) and through the injected reader (EIO on piece 0, on the last piece, after a partial read; EINTR; 1-byte reads):
//       status, index of the failing piece, bytes, and no descriptor left open (/proc/self/fd counted before and after);
//     export_in_chunks with stand-ins for the generate and format steps that count live objects: n = 0, 1, batch, batch + 1,
//       2 * batch + 1; the generator failing on chunk 0, chunk 1, the last chunk; the formatter failing while the next chunk is in
//       flight; a throwing generator; both failing at once -- live objects 0 at return, the (b0, m) sequence, the byte total;
//     format_strided: threads > n, threads = 1, n = 0, which thread's status wins, a throwing task;
//     proof_shape_refusal: every rule just inside and just outside its bound.
//   proof_export_check slotproof <file>
//     slot_proof_of over the dataset tree in <file> (u64 n_slots, max_log2_nslots, n_layers, the layer sizes, then the layers), every
//     slot: one line of hex each, which the pytest side compares with the oracle's padMerkleProof(merkleProof(..)).
#include <dirent.h>
#include <sched.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "fill_pipeline.hpp"
#include "proof_export.hpp"

using namespace cp2i;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::printf("FAILED: %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_case);     \
      std::exit(1);                                                                  \
    }                                                                                \
  } while (0)
static const char* g_case = "";

// ---- the stand-ins export_in_chunks is linked against (the product's are in proof_input.cpp) -------------------------------------------
struct cp2_proof_input { size_t id; };
static std::atomic<long> live{0};               // objects made and not yet freed
static std::atomic<bool> producer_started{false};
static std::vector<std::pair<size_t, size_t>> gen_calls;   // (b0, m), in call order: calls never overlap (one producer, joined per chunk)
static std::vector<std::vector<size_t>> fmt_calls;          // ids per formatted chunk
static std::vector<std::string> fmt_paths;                  // paths seen, "" for NULL
static int fmt_fail_chunk = -1, fmt_fail_status = CP2_ERR_IO;
static bool fmt_waits_for_producer = false;

extern "C" void cp2_proof_input_free(cp2_proof_input* p) {
  if (!p) return;
  --live;
  delete p;
}
extern "C" int cp2_proof_inputs_write_json_batch(const cp2_proof_input* const* ps, size_t n, const char* const* paths, int threads, uint64_t* total_bytes) {
  (void)threads;
  const size_t chunk = fmt_calls.size();
  fmt_calls.emplace_back();
  for (size_t i = 0; i < n; ++i) {
    if (!ps[i]) return CP2_ERR_INVALID;
    fmt_calls.back().push_back(ps[i]->id);
    fmt_paths.push_back(paths && paths[i] ? paths[i] : "");
  }
  if (fmt_waits_for_producer)                               // "while the next chunk is in flight": its generator has begun
    while (!producer_started.load()) sched_yield();
  if ((int)chunk == fmt_fail_chunk) return fmt_fail_status;
  uint64_t b = 0;
  for (size_t i = 0; i < n; ++i) b += 1000 + ps[i]->id;      // the "text" of object id is 1000 + id bytes long
  if (total_bytes) *total_bytes = b;
  return CP2_OK;
}

struct ExportCase {
  const char* name;
  size_t n, batch;
  int gen_fail_chunk, gen_fail_status;   // -1: never
  bool gen_throws;
  int fmt_fail;                          // -1: never
  int want;
  size_t want_gen_calls, want_fmt_chunks;   // generate calls made, chunks whose bytes count
};

static void run_export_case(const ExportCase& c) {
  g_case = c.name;
  gen_calls.clear(); fmt_calls.clear(); fmt_paths.clear();
  fmt_fail_chunk = c.fmt_fail;
  fmt_waits_for_producer = c.fmt_fail >= 0;
  producer_started = false;
  const size_t batch = c.batch ? c.batch : 512;
  std::vector<std::string> names(c.n);
  for (size_t i = 0; i < c.n; ++i) names[i] = "p" + std::to_string(i);
  uint64_t total = ~0ULL;
  const int st = export_in_chunks(c.n, c.batch, 3, [&](size_t b0, size_t m, cp2_proof_input** out) -> int {
    const size_t chunk = b0 / batch;
    if (chunk > 0) producer_started = true;
    gen_calls.emplace_back(b0, m);
    for (size_t i = 0; i < m; ++i) {
      if ((int)chunk == c.gen_fail_chunk && i == m / 2) {     // fails half way: what it made so far is its own to free, or the pipeline's
        if (c.gen_throws) throw std::runtime_error("generator");
        for (size_t j = 0; j < i; ++j) { cp2_proof_input_free(out[j]); out[j] = nullptr; }
        return c.gen_fail_status;
      }
      out[i] = new cp2_proof_input{b0 + i};
      ++live;
    }
    return CP2_OK;
  }, [&](size_t i) { return i % 3 ? names[i].c_str() : nullptr; }, &total);
  CHECK(st == c.want);
  CHECK(live.load() == 0);
  CHECK(gen_calls.size() == c.want_gen_calls);
  for (size_t k = 0; k < gen_calls.size(); ++k) {
    CHECK(gen_calls[k].first == k * batch);
    CHECK(gen_calls[k].second == std::min(batch, c.n - k * batch));
  }
  uint64_t want_total = 0;
  size_t seen = 0;
  for (size_t k = 0; k < fmt_calls.size(); ++k)
    for (size_t i = 0; i < fmt_calls[k].size(); ++i, ++seen) {
      const size_t id = k * batch + i;
      CHECK(fmt_calls[k][i] == id);                          // every chunk formatted in order, every object where it belongs
      CHECK(fmt_paths[seen] == (id % 3 ? names[id] : std::string()));
      if (k < c.want_fmt_chunks) want_total += 1000 + id;
    }
  CHECK(total == want_total);
  if (c.want == CP2_OK) CHECK(seen == c.n);
}

static void export_cases() {
  const int I = CP2_ERR_INVALID, A = CP2_ERR_ALLOC, IO = CP2_ERR_IO, H = CP2_ERR_HIP;
  const ExportCase cases[] = {
      // name                         n  batch gen: chunk status throws  fmt  want  gen calls  formatted chunks
      {"n = 0",                       0, 4,    -1, 0, false,            -1,  CP2_OK, 0, 0},
      {"n = 1",                       1, 4,    -1, 0, false,            -1,  CP2_OK, 1, 1},
      {"n = batch",                   4, 4,    -1, 0, false,            -1,  CP2_OK, 1, 1},
      {"n = batch + 1",               5, 4,    -1, 0, false,            -1,  CP2_OK, 2, 2},
      {"n = 2 batch + 1",             9, 4,    -1, 0, false,            -1,  CP2_OK, 3, 3},
      {"default batch",               9, 0,    -1, 0, false,            -1,  CP2_OK, 1, 1},
      {"batch > n",                   3, ~(size_t)0, -1, 0, false,      -1,  CP2_OK, 1, 1},
      {"generator fails on chunk 0",  9, 4,    0, H, false,             -1,  H, 1, 0},
      {"generator fails on chunk 1",  9, 4,    1, H, false,             -1,  H, 2, 1},
      {"generator fails on the last", 9, 4,    2, IO, false,            -1,  IO, 3, 2},
      {"generator throws on chunk 0", 9, 4,    0, 0, true,              -1,  I, 1, 0},
      {"generator throws on chunk 1", 9, 4,    1, 0, true,              -1,  I, 2, 1},
      {"formatter fails, next chunk in flight", 9, 4, -1, 0, false,     0,   IO, 2, 0},
      {"formatter fails on chunk 1",  9, 4,    -1, 0, false,            1,   IO, 3, 1},
      {"both fail: the formatter's",  9, 4,    1, A, false,             0,   IO, 2, 0},
      {"both fail, generator throws", 9, 4,    1, 0, true,              0,   IO, 2, 0},
  };
  for (const ExportCase& c : cases) run_export_case(c);
  // a generator out of memory is CP2_ERR_ALLOC, on the calling thread (chunk 0) and on the producer thread alike
  for (size_t fail_chunk = 0; fail_chunk < 2; ++fail_chunk) {
    g_case = "bad_alloc";
    fmt_calls.clear(); fmt_paths.clear();
    fmt_fail_chunk = -1;
    fmt_waits_for_producer = false;
    const int st = export_in_chunks(8, 4, 1, [&](size_t b0, size_t m, cp2_proof_input** out) -> int {
      if (b0 / 4 == fail_chunk) throw std::bad_alloc();
      for (size_t i = 0; i < m; ++i) { out[i] = new cp2_proof_input{b0 + i}; ++live; }
      return CP2_OK;
    }, [](size_t) -> const char* { return nullptr; }, nullptr);
    CHECK(st == CP2_ERR_ALLOC && live.load() == 0);
  }
  std::printf("export pipeline ok: %zu cases\n", sizeof cases / sizeof cases[0] + 2);
}

// ---- format_strided ---------------------------------------------------------------------------------------------------------------------
static void strided_cases() {
  struct Case { const char* name; size_t n; int threads; int want_threads; };
  const Case shapes[] = {{"threads > n", 3, 8, 3}, {"threads = 1", 7, 1, 1}, {"n = 0", 0, 4, 1}, {"threads < 1", 5, 0, 1}, {"even", 12, 4, 4}, {"ragged", 13, 4, 4}};
  for (const Case& c : shapes) {
    g_case = c.name;
    std::vector<int> by(c.n, -1);                            // which thread took item i (each item is one thread's alone)
    std::atomic<long> calls{0};
    uint64_t total = 77;
    const int st = format_strided(c.n, c.threads, [&](int t, size_t i, uint64_t* bytes) {
      by[i] = t;
      *bytes += 10 + i;
      ++calls;
      return CP2_OK;
    }, &total);
    CHECK(st == CP2_OK && calls.load() == (long)c.n);
    uint64_t want = 0;
    for (size_t i = 0; i < c.n; ++i) { CHECK(by[i] == (int)(i % (size_t)c.want_threads)); want += 10 + i; }
    CHECK(total == want);
  }
  // a failing item on thread 2 and another on thread 0: thread 0's status; the other items are still formatted; no total
  g_case = "precedence";
  {
    std::atomic<long> calls{0};
    uint64_t total = 77;
    const int st = format_strided(12, 4, [&](int t, size_t i, uint64_t* bytes) {
      ++calls;
      *bytes += 1;
      if (i == 2) { CHECK(t == 2); return (int)CP2_ERR_HIP; }
      if (i == 8) { CHECK(t == 0); return (int)CP2_ERR_IO; }
      return (int)CP2_OK;
    }, &total);
    CHECK(st == CP2_ERR_IO && calls.load() == 12 && total == 77);
  }
  g_case = "only thread 2 fails";
  CHECK(format_strided(12, 4, [&](int, size_t i, uint64_t*) { return i == 6 ? (int)CP2_ERR_HIP : (int)CP2_OK; }, nullptr) == CP2_ERR_HIP);
  g_case = "a throwing task";
  {
    std::atomic<long> calls{0};
    const int st = format_strided(12, 4, [&](int, size_t i, uint64_t*) -> int {
      ++calls;
      if (i == 1) throw std::runtime_error("task");         // thread 1 stops there: items 5 and 9 are not formatted
      return CP2_OK;
    }, nullptr);
    CHECK(st == CP2_ERR_ALLOC && calls.load() == 10);
  }
  std::printf("strided fan-out ok\n");
}

// ---- proof_shape_refusal ----------------------------------------------------------------------------------------------------------------
static void shape_cases() {
  g_case = "shape";
  cp2_config c{};
  c.max_depth = 10; c.max_log2_nslots = 4; c.cell_size = 64; c.block_size = 256; c.n_slots = 11; c.n_cells = 64; c.n_samples = 5;
  CHECK(proof_shape_refusal(c, 6, 4).empty());
  // nCells: a power of two (sample/bn254.nim:20) of at least 2 when anything is sampled (types/bn254.nim:48)
  for (uint64_t nc : {2, 4, 1 << 20}) { c.n_cells = nc; CHECK(proof_shape_refusal(c, 6, 4).empty()); }
  for (uint64_t nc : {0, 1, 3, 6, (1 << 20) + 1}) {
    c.n_cells = nc;
    CHECK(proof_shape_refusal(c, 6, 4) == "nCells " + std::to_string(nc) + " is not a power of two >= 2");
  }
  c.n_samples = 0;
  c.n_cells = 1;
  CHECK(proof_shape_refusal(c, 6, 4).empty());               // nothing sampled: no bits extracted
  c.n_cells = 3;
  CHECK(!proof_shape_refusal(c, 6, 4).empty());
  c.n_samples = 5;
  c.n_cells = 64;
  // padMerkleProof (types.nim:29): the slot tree against maxDepth, the dataset tree against maxLog2NSlots
  CHECK(proof_shape_refusal(c, 10, 4).empty());
  CHECK(proof_shape_refusal(c, 11, 4) == "its slot tree is deeper than maxDepth");
  CHECK(proof_shape_refusal(c, 10, 5) == "its dataset tree is deeper than maxLog2NSlots");
  CHECK(proof_shape_refusal(c, 11, 5) == "its slot tree is deeper than maxDepth");   // in the order the *_many calls report them
  c.max_depth = 0; c.max_log2_nslots = 0;
  CHECK(proof_shape_refusal(c, 0, 0).empty());
  CHECK(!proof_shape_refusal(c, 1, 0).empty() && !proof_shape_refusal(c, 0, 1).empty());
  std::printf("shape refusals ok\n");
}

// ---- slot_file_read_list ----------------------------------------------------------------------------------------------------------------
static size_t open_fds() {
  size_t n = 0;
  DIR* d = opendir("/proc/self/fd");
  if (!d) { std::printf("FAILED: cannot list /proc/self/fd\n"); std::exit(1); }
  while (readdir(d)) ++n;
  closedir(d);
  return n;                                                  // ".", ".." and the listing's own descriptor included: the same every time
}

// the injected reader (fill_pipeline.hpp: slot_file_read); set before a case runs, read-only while it does
struct Fault {
  enum Kind { NONE, EIO_AT, PARTIAL_THEN_EIO, EINTR_TWICE, ONE_BYTE } kind = NONE;
  uint64_t off = 0;                                          // EIO_AT / PARTIAL_THEN_EIO: the file offset of the piece it hits
};
static Fault fault;
static std::atomic<long> injected{0}, intr{0};
static ssize_t injected_pread(int fd, void* buf, size_t n, off_t off) {
  switch (fault.kind) {
    case Fault::EIO_AT:
      if ((uint64_t)off == fault.off) { ++injected; errno = EIO; return -1; }
      break;
    case Fault::PARTIAL_THEN_EIO:
      if ((uint64_t)off == fault.off && n > 1) { ++injected; return ::pread(fd, buf, n / 2, off); }
      if ((uint64_t)off > fault.off && (uint64_t)off < fault.off + 100) { ++injected; errno = EIO; return -1; }
      break;
    case Fault::EINTR_TWICE:
      if (intr++ % 3 != 2) { ++injected; errno = EINTR; return -1; }   // two interruptions before every read that gets through
      break;
    case Fault::ONE_BYTE:
      if (n > 1) { ++injected; n = 1; }
      break;
    case Fault::NONE: break;
  }
  return ::pread(fd, buf, n, off);
}

static void read_list_cases(const std::string& dir) {
  const size_t LEN = 100, NP = 8;
  std::vector<uint8_t> content(1000);
  for (size_t i = 0; i < content.size(); ++i) content[i] = (uint8_t)(i * 131 + 7);
  auto write_file = [&](const std::string& name, size_t bytes) {
    FILE* f = std::fopen(name.c_str(), "wb");
    if (!f || std::fwrite(content.data(), 1, bytes, f) != bytes || std::fclose(f) != 0) { std::printf("FAILED: cannot write %s\n", name.c_str()); std::exit(1); }
  };
  const std::string full = dir + "/full.dat", cut = dir + "/cut.dat", missing = dir + "/missing.dat", isdir = dir + "/dir.dat";
  write_file(full, 1000);
  write_file(cut, 250);
  if (mkdir(isdir.c_str(), 0700) != 0) { std::printf("FAILED: mkdir\n"); std::exit(1); }
  // pieces out of file order, at offsets that are no multiple of anything
  const uint64_t offs[NP] = {701, 3, 333, 899, 105, 555, 207, 440};
  auto len_of = [&](size_t) { return LEN; };
  auto off_of = [&](size_t c) { return offs[c]; };
  std::vector<uint8_t> got;
  auto dst_of = [&](size_t c) { return &got[c * LEN]; };
  // what the read rule gives for piece c of a file of `bytes` bytes (slot.nim:61-66: zeros past the end)
  auto piece_ok = [&](size_t c, size_t bytes) {
    for (size_t i = 0; i < LEN; ++i)
      if (got[c * LEN + i] != (offs[c] + i < bytes ? content[offs[c] + i] : 0)) return false;
    return true;
  };
  auto run = [&](const std::string& name, size_t count, size_t* bad) {
    got.assign(NP * LEN, 0xee);
    const size_t before = open_fds();
    const int st = slot_file_read_list(name, count, len_of, off_of, dst_of, bad);
    CHECK(open_fds() == before);                             // whatever happened, the file is closed again
    return st;
  };
  size_t bad = 99;

  g_case = "a full file";
  CHECK(run(full, NP, &bad) == -1 && bad == 99);
  for (size_t c = 0; c < NP; ++c) CHECK(piece_ok(c, 1000));
  g_case = "a file that ends inside piece 6 (207 .. 307 of 250 bytes) and before pieces 0, 2, 3, 5, 7";
  CHECK(run(cut, NP, &bad) == -1 && bad == 99);
  for (size_t c = 0; c < NP; ++c) CHECK(piece_ok(c, 250));
  CHECK(got[6 * LEN + 42] == content[249] && got[6 * LEN + 43] == 0 && got[0] == 0);
  g_case = "a missing file";
  CHECK(run(missing, NP, &bad) == 0 && bad == 99 && got[0] == 0xee);
  CHECK(slot_file_error(missing, 0) == "cannot open " + missing);
  g_case = "a directory in place of the file";
  CHECK(run(isdir, NP, &bad) == EISDIR && bad == 0);
  g_case = "zero pieces";
  bad = 99;
  CHECK(run(full, 0, &bad) == -1 && bad == 99 && got[0] == 0xee);
  CHECK(run(missing, 0, &bad) == 0);
  CHECK(slot_file_read_list(full, 0, len_of, off_of, dst_of) == -1);   // (bad_piece may be left out)

  slot_file_read = injected_pread;
  struct Case { const char* name; Fault f; int want; size_t bad; };
  const Case cases[] = {
      {"EIO on piece 0", {Fault::EIO_AT, offs[0]}, EIO, 0},
      {"EIO on a middle piece", {Fault::EIO_AT, offs[4]}, EIO, 4},
      {"EIO on the last piece", {Fault::EIO_AT, offs[NP - 1]}, EIO, NP - 1},
      {"EIO after a partial read", {Fault::PARTIAL_THEN_EIO, offs[3]}, EIO, 3},
      {"EINTR", {Fault::EINTR_TWICE, 0}, -1, 99},
      {"1-byte reads", {Fault::ONE_BYTE, 0}, -1, 99},
  };
  for (const Case& c : cases) {
    g_case = c.name;
    fault = c.f;
    injected = 0;
    intr = 0;
    bad = 99;
    CHECK(run(full, NP, &bad) == c.want && bad == c.bad);
    CHECK(injected.load() > 0);                              // a case where nothing was injected proves nothing
    for (size_t p = 0; p < (c.want < 0 ? NP : c.bad); ++p) CHECK(piece_ok(p, 1000));   // every piece before the failing one was read
    if (c.want >= 0) CHECK(got[(c.bad + 1 < NP ? c.bad + 1 : c.bad) * LEN + LEN - 1] == (c.bad + 1 < NP ? 0xee : 0));   // none after it was touched
  }
  fault = Fault();
  slot_file_read = ::pread;

  // as the product calls it: files spread over threads (on_threads), every worker its own file and rows
  g_case = "on four threads";
  {
    const size_t before = open_fds();
    std::vector<std::vector<uint8_t>> rows(16, std::vector<uint8_t>(NP * LEN));
    std::vector<int> st(16, 7);
    on_threads(4, 16, [&](int, size_t k) {
      st[k] = slot_file_read_list(k % 5 == 4 ? missing : (k & 1 ? cut : full), NP, len_of, off_of, [&](size_t c) { return &rows[k][c * LEN]; });
      return true;
    });
    for (size_t k = 0; k < 16; ++k) {
      CHECK(st[k] == (k % 5 == 4 ? 0 : -1));
      got = rows[k];
      if (st[k] < 0) for (size_t c = 0; c < NP; ++c) CHECK(piece_ok(c, k & 1 ? 250 : 1000));
    }
    CHECK(open_fds() == before);
  }
  std::printf("read list ok: 7 file cases, %zu injected cases\n", sizeof cases / sizeof cases[0]);
}

// ---- slot_proof_of over a tree the oracle built -----------------------------------------------------------------------------------------
static int slot_proofs(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  uint64_t head[3];
  if (std::fread(head, 8, 3, f) != 3) return 2;
  const size_t n_slots = head[0], max_log2 = head[1], n_layers = head[2];
  std::vector<uint64_t> sz(n_layers);
  if (std::fread(sz.data(), 8, n_layers, f) != n_layers) return 2;
  std::vector<size_t> dsizes(sz.begin(), sz.end());
  size_t total = 0;
  for (size_t m : dsizes) total += m;
  std::vector<uint8_t> dlayers(total * 32);                  // exactly the tree: a read past it is the sanitizer's to find
  if (std::fread(dlayers.data(), 32, total, f) != total) return 2;
  std::fclose(f);
  std::vector<uint8_t> proof;
  for (size_t s = 0; s < n_slots; ++s) {
    slot_proof_of(dlayers, dsizes, n_slots, max_log2, s, proof);
    if (proof.size() != max_log2 * 32) return 3;
    for (uint8_t b : proof) std::printf("%02x", b);
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && std::string(argv[1]) == "slotproof") return slot_proofs(argv[2]);
  if (argc != 3 || std::string(argv[1]) != "run") {
    std::printf("usage: proof_export_check run <scratch dir> | slotproof <file>\n");
    return 2;
  }
  read_list_cases(argv[2]);
  export_cases();
  strided_cases();
  shape_cases();
  std::printf("proof export check ok\n");
  return 0;
}
