// The host side of the ingestion pipe (csrc/slot_trees.cpp): filling a turn's buffer from slot files (pread) or from a host array
// (memcpy) on several threads.  No HIP in here: tests/host_check/fill_pipeline_check.cpp runs it against real files on the CPU, under
// AddressSanitizer + UBSan and again under ThreadSanitizer.
//
// Bytes [0, m * cell_size) of the turn [c0, c0 + m) of batch `g` go into `buf`, from the slot files "<base><slot>.dat" (dataset.nim:34)
// -- or, with a name table, from the files it lists, one per unit of the batch (scrubbing many datasets at once: scrub.cpp) --
// zero-filled past the end of a file (slot.nim:61-66).  The turn is cut into GRAINS of 4 MiB which the fill threads take from a shared
// counter (round 6; equal byte ranges, one per thread, joined per turn, before): the formatting threads of a streamed build compete for
// the same cores, and a fill thread that loses its core for a scheduler slice no longer holds up a whole turn.  Every thread walks the
// pieces of its grain (ingest_piece) and opens the files it needs itself: nothing is held open between turns, however many files a turn
// touches.
// A fill is POSTED and JOINED apart (begin / join), two turns deep: the building thread posts turn k + 1's fill before it joins turn
// k's, so a worker that finds no grain of turn k left goes straight on to turn k + 1 -- no thread waits at a turn's end for the slowest
// one (16 slots of 8 GiB: 0.96 -> 0.99 of the fake source's rate) -- and turn k's scheduling work (layer passes, the caller's sampling
// hook) runs on the building thread while the workers read.
// O_DIRECT (cp2_set_ingest_direct / CP2_INGEST_DIRECT=1): slot files that are not in the page cache are read straight into the pinned
// ring, whole 4 KiB blocks, without passing through (and evicting) the page cache; a piece whose file offset or buffer address is not
// block aligned, the last partial block of a piece, and a file system that refuses O_DIRECT (tmpfs) are read buffered.
// ONE READ RULE for every read of a slot file (these fills and slot_file_read_list, the reader of listed cells and blocks): a read
// interrupted (EINTR) is retried, a short read reads on, a read of 0 bytes is the end of the file -- zeros from there (slot.nim:61-66) -- and a
// read that fails with any other errno is an ERROR naming the file, never zeros: the reference yields no data for a file it cannot
// read.  The O_DIRECT attempt only ever reads ahead: whatever it fails on (EINVAL included), the buffered loop reads the rest of
// the piece, and only that loop decides whether a read failed.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>

#include "ingest_turns.hpp"
#include "workers.hpp"

namespace cp2i {

inline std::string fill_slot_file_name(const std::string& base, uint64_t slot) { return base + std::to_string(slot) + ".dat"; }   // dataset.nim:34

// the largest cell a SlotFile source may have (slot.nim:60-61: assert(cellSize <= 16384)); larger is CP2_ERR_INVALID
constexpr size_t SLOT_FILE_MAX_CELL = 16384;

// The read every read of a slot file goes through.  ::pread in the product; only the CPU checks (tests/host_check) replace it, to
// inject errors, interruptions and short reads.
using SlotFileRead = ssize_t (*)(int fd, void* buf, size_t n, off_t off);
inline SlotFileRead slot_file_read = ::pread;

// Bytes [pos, n) of `out` from file offset off + pos onward, by the read rule above.  0, or the errno of the read that failed (the
// bytes it did not read are zeros then, too: no caller may use them).
inline int slot_file_read_rest(int fd, uint8_t* out, size_t n, uint64_t off, size_t pos = 0) {
  int err = 0;
  while (pos < n) {
    const ssize_t r = slot_file_read(fd, out + pos, n - pos, (off_t)(off + pos));
    if (r > 0) { pos += (size_t)r; continue; }
    if (r == 0) break;                  // end of file
    if (errno == EINTR) continue;
    err = errno ? errno : EIO;
    break;
  }
  if (pos < n) std::memset(out + pos, 0, n - pos);
  return err;
}

// cell `cell` of an open slot file (slot.nim:57-68): 0, or the errno of a failed read (the CPU checks' yardstick; the product reads lists)
inline int read_file_cell(int fd, size_t cell_size, uint64_t cell, uint8_t* out) { return slot_file_read_rest(fd, out, cell_size, cell * cell_size); }

// what cp2_last_error says about a slot file: err == 0 it could not be opened, otherwise a read of it failed with errno `err`
inline std::string slot_file_error(const std::string& fname, int err) {
  return err == 0 ? "cannot open " + fname : "cannot read " + fname + ": " + std::strerror(err);
}

// ONE FILE, A LIST OF PIECES: `fname` is opened, piece c = [off_of(c), + len_of(c)) of it is read into dst_of(c) for c = 0 .. count - 1
// by the read rule, up to the first read that fails, and the file is closed.  Every reader of listed cells or blocks goes through this
// (the proof-input paths, the read-back of listed blocks, a fill session's re-read); the turns above read ranges, not lists.
// Returns what slot_file_error takes: -1 all read (zeros past the end of the file), 0 the file could not be opened, else the errno of
// the read that failed -- *bad_piece is then the piece it belonged to.  The file is opened for zero pieces, too.
template <typename LenOf, typename OffOf, typename DstOf>
inline int slot_file_read_list(const std::string& fname, size_t count, LenOf len_of, OffOf off_of, DstOf dst_of, size_t* bad_piece = nullptr) {
  const int fd = open(fname.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd < 0) return 0;
  int err = 0;
  size_t c = 0;
  for (; c < count && !err; ++c) err = slot_file_read_rest(fd, dst_of(c), (size_t)len_of(c), (uint64_t)off_of(c));
  (void)close(fd);
  if (!err) return -1;
  if (bad_piece) *bad_piece = c - 1;
  return err;
}

class FillPipeline {
 public:
  static constexpr size_t DIRECT_ALIGN = 4096;   // offset, length and address granule of O_DIRECT reads
  explicit FillPipeline(int threads) : threads_(threads < 1 ? 1 : threads) {
    if (threads_ > 1) pool_.reset(new Workers(threads_ - 1));
  }
  ~FillPipeline() { join_all(); }                // (the workers write into the caller's buffers: none may outlive this)
  Workers* workers() { return pool_.get(); }
  bool idle() const { return jobs_.empty(); }

  // post the fill of the turn [c0, c0 + m) into `buf`: the workers start on it as soon as they run out of grains of the job before.
  // mem != nullptr: the turn's bytes are copied from host memory at `mem` (host arrays) instead of read from slot files.
  // names != nullptr: a NAME TABLE indexed by IngestPiece::unit -- unit i of the batch is the file names[i] (g.n_units entries, which the
  // caller keeps alive until the fill is joined) instead of "<base><slot>.dat"; the lowest UNIT's file is the one a failed join names.
  void begin(const IngestGeom& g, const std::string& base, size_t c0, size_t m, uint8_t* buf, bool want_direct, const uint8_t* mem = nullptr,
             const std::string* names = nullptr) {
    auto job = std::make_shared<Job>();
    job->g = g;
    job->base = base;
    job->names = names;
    job->c0 = c0;
    job->mem = mem;
    job->nbytes = m * g.cell_size;
    job->n_grains = ingest_grain_count(job->nbytes, INGEST_FILL_GRAIN);
    job->buf = buf;
    job->direct = want_direct;
    jobs_.push_back(job);
    if (pool_)
      for (size_t t = 1; t < (size_t)threads_ && t < job->n_grains; ++t) pool_->submit([job] { take_grains(job); });
  }
  // The OLDEST posted fill is complete (this thread takes grains of it too; the workers may already be on the next job).
  // false: a slot file could not be opened or read -- *bad names the one of the LOWEST slot (whichever thread met it), *err is 0 when it
  // could not be opened and the errno of the read that failed otherwise (slot_file_error); the turn's bytes must not be used.
  bool join(std::string* bad, int* err = nullptr) {
    if (jobs_.empty()) return true;
    std::shared_ptr<Job> job = jobs_.front();
    jobs_.pop_front();
    take_grains(job);
    {
      std::unique_lock<std::mutex> lk(job->mu);
      job->cv.wait(lk, [&] { return job->done == job->n_grains; });
      if (!job->first_bad.empty()) {
        if (bad) *bad = job->first_bad;
        if (err) *err = job->first_bad_errno;
        return false;
      }
    }
    return true;
  }
  void join_all() {
    while (!jobs_.empty()) (void)join(nullptr);
  }

 private:
  struct Job {
    IngestGeom g;
    std::string base;
    const std::string* names = nullptr;     // the name table (not owned), or null: fill_slot_file_name(base, slot)
    size_t c0 = 0, nbytes = 0, n_grains = 0;
    uint8_t* buf = nullptr;
    const uint8_t* mem = nullptr;
    bool direct = false;
    std::atomic<size_t> next{0};            // the next grain nobody has taken yet
    std::mutex mu;
    std::condition_variable cv;
    size_t done = 0;                        // grains completed (under mu)
    std::string first_bad;                  // (under mu)
    uint64_t first_bad_slot = ~0ULL;
    int first_bad_errno = 0;                // 0: could not be opened
  };

  static void report(Job& job, uint64_t slot, const std::string& fname, int err) {
    std::lock_guard<std::mutex> lk(job.mu);
    if (slot < job.first_bad_slot) { job.first_bad_slot = slot; job.first_bad = fname; job.first_bad_errno = err; }
  }

  static void fill_range(Job& job, size_t a, size_t b) {
    if (job.mem) { std::memcpy(job.buf + a, job.mem + a, b - a); return; }
    const IngestGeom& g = job.g;
    uint8_t* buf = job.buf;
    for (size_t p = a; p < b;) {
      const IngestPiece q = ingest_piece(g, job.c0, p, b);
      const std::string fname = job.names ? job.names[q.unit] : fill_slot_file_name(job.base, q.slot);
      const uint64_t key = job.names ? (uint64_t)q.unit : q.slot;   // what "lowest" means among the files that failed
      const int fd = open(fname.c_str(), O_RDONLY);
      if (fd < 0) {
        report(job, key, fname, 0);
        std::memset(buf + p, 0, q.len);
        p += q.len;
        continue;
      }
      size_t pos = 0;
      if (job.direct && q.len >= DIRECT_ALIGN && q.file_off % DIRECT_ALIGN == 0 && reinterpret_cast<uintptr_t>(buf + p) % DIRECT_ALIGN == 0) {
        const int dfd = open(fname.c_str(), O_RDONLY | O_DIRECT);
        if (dfd >= 0) {
          const size_t whole = q.len / DIRECT_ALIGN * DIRECT_ALIGN;
          while (pos < whole) {
            const ssize_t r = slot_file_read(dfd, buf + p + pos, whole - pos, (off_t)(q.file_off + pos));
            if (r <= 0) break;                     // end of file or any failure: the buffered reads below go on from pos
            pos += (size_t)r;
            if ((size_t)r % DIRECT_ALIGN) break;   // short, unaligned: end of file (the buffered reads below see that too)
          }
          close(dfd);
        }
      }
      const int err = slot_file_read_rest(fd, buf + p, q.len, q.file_off, pos);
      if (err) report(job, key, fname, err);
      close(fd);
      p += q.len;
    }
  }
  static void take_grains(const std::shared_ptr<Job>& job) {   // any thread: grains of this job until none is left
    size_t mine = 0;
    for (;;) {
      const size_t i = job->next.fetch_add(1, std::memory_order_relaxed);
      if (i >= job->n_grains) break;
      size_t a = 0, b = 0;
      ingest_grain(job->nbytes, INGEST_FILL_GRAIN, i, &a, &b);
      fill_range(*job, a, b);
      ++mine;
    }
    if (mine) {
      std::lock_guard<std::mutex> lk(job->mu);
      job->done += mine;
      if (job->done == job->n_grains) job->cv.notify_all();
    }
  }

  int threads_;
  std::unique_ptr<Workers> pool_;
  std::deque<std::shared_ptr<Job>> jobs_;   // posted, not yet joined: at most two (the turn about to be shipped and the one after it)
};

}  // namespace cp2i
