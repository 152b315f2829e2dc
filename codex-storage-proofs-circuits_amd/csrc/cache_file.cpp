// The library's own cache files, device side (layout, heads, stamps and the tmp-file discipline: cache_file.hpp): the payload's way
// between the device and the file, and on it the tree cache (cp2_slot_trees_save / _load: SURVEY.md 8f rank 2) and the kept form
// (kept_save / kept_load).  A later run with new entropy needs only 2 permutations per sample plus gathers from a loaded cache (the
// reference re-hashes all slots per run AND the proving slot once per sample, gen_input/bn254.nim:42,57).
#include <algorithm>
#include <condition_variable>
#include <memory>
#include <mutex>

#include "cache_file.hpp"
#include "trees.hpp"

using namespace cp2i;

namespace {

// ring-slot flags shared between the streaming thread and its I/O worker
struct SlotFlags {
  static constexpr int K = 3;
  std::mutex mu;
  std::condition_variable cv;
  bool flag[K] = {false, false, false};
  bool failed = false;
  void set(int r, bool v) { { std::lock_guard<std::mutex> lk(mu); flag[r] = v; } cv.notify_all(); }
  void fail() { { std::lock_guard<std::mutex> lk(mu); failed = true; } cv.notify_all(); }
  // waits until flag[r] == v; false if the worker reported a failure
  bool wait(int r, bool v) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return failed || flag[r] == v; });
    return !failed;
  }
};

// The pinned ring a payload moves through in 64 MiB chunks, chunk c in buffer c % depth: up to three buffers, no more than there are
// chunks, each as large as the largest chunk it will hold (only the last is short), an event per buffer for the copy that uses it, and
// one worker thread for the file I/O.  Below two full chunks there is at most a chunk's tail to overlap: the file I/O then runs on the
// calling thread, no thread is started and no chunk changes cores between its I/O and its checksum.  No whole payload is on the host.
struct PayloadRing {
  static constexpr int K = SlotFlags::K;
  static constexpr size_t CHUNK = (size_t)64 << 20;
  size_t total = 0, chunk = 0, n_chunks = 0;
  int depth = 0;
  PinBuf pin[K];
  hipEvent_t ev[K] = {};
  SlotFlags flags;
  std::unique_ptr<Workers> io;         // null: file I/O on the calling thread
  ~PayloadRing() {
    io.reset();                        // joins before the events and the pinned blocks go
    for (int r = 0; r < K; ++r) if (ev[r]) (void)hipEventDestroy(ev[r]);
  }
  int init(cp2_ctx* ctx, size_t bytes) {
    total = bytes;
    chunk = std::min(CHUNK, std::max<size_t>(total, 32));
    n_chunks = (total + chunk - 1) / chunk;
    depth = (int)std::min<size_t>(K, std::max<size_t>(n_chunks, 1));
    if (total >= 2 * CHUNK) io.reset(new Workers(1));
    for (int r = 0; r < depth; ++r) {
      CP2_TRY(pin[r].alloc(ctx, n_chunks && (size_t)r + 1 == n_chunks ? len(r) : chunk));
      CP2_HIP(ctx, hipEventCreateWithFlags(&ev[r], hipEventDisableTiming));
    }
    return CP2_OK;
  }
  int slot(size_t c) const { return (int)(c % (size_t)depth); }
  size_t len(size_t c) const { return std::min(chunk, total - c * chunk); }
  // chunk c between its buffer and the file (payload at `off`), on the worker: the buffer's flag is set once it is read, cleared once written
  void post(int fd, off_t off, size_t c, bool write) {
    const int r = slot(c);
    uint8_t* p = pin[r].u8();
    const size_t m = len(c), at = (size_t)off + c * chunk;
    auto move = [this, r, fd, p, m, at, write] {
      if (write ? pwrite_all(fd, p, m, (off_t)at) : pread_all(fd, p, m, (off_t)at)) flags.set(r, !write);
      else flags.fail();
    };
    if (io) io->submit(move);
    else move();
  }
  void wait_idle() { if (io) io->wait_idle(); }
};

// device -> ring -> file at `off`: the download of chunk i+1, the checksum of chunk i and the write of chunk i-1 overlap.  The caller
// has drained whatever wrote d_buf.
int cache_payload_out(cp2_ctx* ctx, int fd, off_t off, const uint8_t* d_buf, size_t bytes, Checksum64* sum) {
  PayloadRing ring;
  CP2_TRY(ring.init(ctx, bytes));
  SlotFlags& busy = ring.flags;                                     // flag[r]: the writer still reads pin[r]
  int st = CP2_OK;
  auto finish_chunk = [&](size_t c) -> int {                        // landed -> checksum -> hand to the writer
    const int r = ring.slot(c);
    CP2_HIP(ctx, hipEventSynchronize(ring.ev[r]));
    sum->update(ring.pin[r].u8(), ring.len(c));
    busy.set(r, true);
    ring.post(fd, off, c, true);
    return CP2_OK;
  };
  for (size_t c = 0; c < ring.n_chunks && st == CP2_OK; ++c) {
    const int r = ring.slot(c);
    if (!busy.wait(r, false)) { st = CP2_ERR_IO; break; }           // chunk c - depth has left pin[r]
    hipError_t e = hipMemcpyAsync(ring.pin[r].p, d_buf + c * ring.chunk, ring.len(c), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(ring.ev[r], ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("cache download: ") + hipGetErrorString(e); st = CP2_ERR_HIP; break; }
    if (c > 0) st = finish_chunk(c - 1);                            // overlaps the download just enqueued
  }
  if (st == CP2_OK && ring.n_chunks) st = finish_chunk(ring.n_chunks - 1);
  ring.wait_idle();
  (void)hipStreamSynchronize(ctx->stream);
  if (st == CP2_OK && busy.failed) st = CP2_ERR_IO;
  return st;
}

// file at `off` -> ring -> device: the read of chunk i+1, the checksum of chunk i and the upload of chunk i-1 overlap.  The bytes reach
// the device before the checksum is known; the caller discards them on a mismatch.
int cache_payload_in(cp2_ctx* ctx, int fd, off_t off, uint8_t* d_buf, size_t bytes, Checksum64* sum) {
  PayloadRing ring;
  CP2_TRY(ring.init(ctx, bytes));
  for (int r = 0; r < ring.depth; ++r) CP2_HIP(ctx, hipEventRecord(ring.ev[r], ctx->stream));
  SlotFlags& ready = ring.flags;                                    // flag[r]: pin[r] holds the chunk the main thread waits for
  int st = CP2_OK;
  size_t submitted = 0;
  auto submit_read = [&](size_t c) -> int {                         // pin[r] is free once the upload of chunk c - depth has finished
    CP2_HIP(ctx, hipEventSynchronize(ring.ev[ring.slot(c)]));
    ring.post(fd, off, c, false);
    return CP2_OK;
  };
  for (size_t c = 0; c < ring.n_chunks && st == CP2_OK; ++c) {
    while (st == CP2_OK && submitted < ring.n_chunks && submitted < c + (size_t)ring.depth) st = submit_read(submitted++);
    if (st != CP2_OK) break;
    const int r = ring.slot(c);
    if (!ready.wait(r, true)) { st = CP2_ERR_IO; break; }
    ready.set(r, false);
    sum->update(ring.pin[r].u8(), ring.len(c));
    hipError_t e = hipMemcpyAsync(d_buf + c * ring.chunk, ring.pin[r].p, ring.len(c), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(ring.ev[r], ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("cache upload: ") + hipGetErrorString(e); st = CP2_ERR_HIP; }
  }
  ring.wait_idle();
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && st == CP2_OK) st = CP2_ERR_HIP;
  return st;
}

// The cache file of `h` at `path` with the payload at d_buf (complete: the caller has drained its streams): stamps taken, payload
// streamed out under its checksum, the head written last, renamed into place.
int cache_save(cp2_ctx* ctx, const char* path, CacheHead& h, const void* d_buf) {
  if (h.src == (uint64_t)CellSrc::File) h.stamps = file_stamps(h.base, h.first_item, h.n_items, h.units_per_slot);
  TmpFile tmp(path);
  if (!tmp.ok()) { ctx->err = "cannot create " + tmp.tmp_name(); return CP2_ERR_IO; }
  Checksum64 sum;
  CP2_TRY(cache_payload_out(ctx, tmp.fd(), (off_t)h.payload_off(), static_cast<const uint8_t*>(d_buf), h.payload_bytes, &sum));
  h.checksum = sum.finish();
  const std::vector<uint8_t> head = cache_head_bytes(h);
  return pwrite_all(tmp.fd(), head.data(), head.size(), 0) && tmp.commit(false) ? CP2_OK : CP2_ERR_IO;
}

// The payload of the file whose head is `h` into d_buf.  CP2_ERR_IO with *what set when the file is not exactly as long as its head
// states or the payload does not have the checksum; with *what as it was when it cannot be read.
int cache_load_payload(cp2_ctx* ctx, int fd, const CacheHead& h, void* d_buf, const char** what) {
  struct stat sb;
  if (fstat(fd, &sb) != 0 || (uint64_t)sb.st_size != h.payload_off() + h.payload_bytes) { *what = "is truncated"; return CP2_ERR_IO; }   // or appended to
  Checksum64 sum;
  CP2_TRY(cache_payload_in(ctx, fd, (off_t)h.payload_off(), static_cast<uint8_t*>(d_buf), h.payload_bytes, &sum));
  if (sum.finish() != h.checksum) { *what = "is corrupt (checksum)"; return CP2_ERR_IO; }
  return CP2_OK;
}

}  // namespace

// ---- persisted slot trees: every node of the layer-major buffer (canonical 32-byte elements) ----------------------------------------
extern "C" int cp2_slot_trees_save(cp2_slot_trees* t, const char* path) try {
  if (!t || !path) return CP2_ERR_INVALID;
  cp2_ctx* ctx = t->ctx;
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  CacheHead h;
  h.format = CacheFormat::Tree;
  h.n_items = t->n_slots; h.cell_size = t->cell_size; h.block_size = t->block_size; h.n_cells = t->n_cells;
  h.units_per_slot = t->units_per_slot; h.src = (uint64_t)t->src; h.seed = t->dataset_seed; h.first_item = t->first_slot;
  h.base = t->file_base; h.payload_bytes = t->nodes.bytes;
  CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));                  // the trees are complete
  if (ctx->aux_stream) CP2_HIP(ctx, hipStreamSynchronize(ctx->aux_stream));
  return cache_save(ctx, path, h, t->nodes.p);
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

extern "C" int cp2_slot_trees_load(cp2_ctx* ctx, const char* path, cp2_slot_trees** out) try {
  if (!ctx || !path || !out) return CP2_ERR_INVALID;
  *out = nullptr;
  const FdCloser f{open(path, O_RDONLY)};
  if (f.fd < 0) return CP2_ERR_IO;
  CacheHead h;
  CacheRefusal why;
  const bool read = cache_head_read(f.fd, &h, &why);
  // format and geometry are judged on the header's own fields first, whatever else is wrong with the file: then its length
  if (why == CacheRefusal::NotThisVersion || h.format != CacheFormat::Tree ||
      trees_check_geometry(h.cell_size, h.block_size, h.n_cells, h.n_items) != CP2_OK ||
      (h.units_per_slot > 1 && !unit_geometry_ok(h.units_per_slot, h.cell_size, h.block_size, h.n_cells))) {
    ctx->err = std::string("not a slot-tree cache of this version: ") + path;
    return CP2_ERR_IO;
  }
  if (!read) {
    if (why == CacheRefusal::Truncated) ctx->err = std::string("slot-tree cache is truncated: ") + path;
    return CP2_ERR_IO;
  }
  if (h.src == (uint64_t)CellSrc::File && h.stamps != file_stamps(h.base, h.first_item, h.n_items, h.units_per_slot)) {
    ctx->err = std::string("slot files changed since the cache was written: ") + path;
    return CP2_ERR_IO;   // size or mtime of a slot file differs: the trees no longer describe the data
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return CP2_ERR_HIP;
  std::unique_ptr<cp2_slot_trees> t(trees_new(ctx, h.n_items, h.cell_size, h.block_size, h.n_cells));
  if (!t) return CP2_ERR_ALLOC;
  t->src = (CellSrc)h.src; t->dataset_seed = h.seed; t->first_slot = h.first_item; t->units_per_slot = h.units_per_slot; t->file_base = h.base;
  CP2_TRY(trees_layout(t.get()));
  if (t->nodes.bytes != h.payload_bytes) return CP2_ERR_IO;
  const char* what = nullptr;
  const int st = cache_load_payload(ctx, f.fd, h, t->nodes.p, &what);
  if (st != CP2_OK) {
    if (what) ctx->err = std::string("slot-tree cache ") + what + ": " + path;
    return st;
  }
  *out = t.release();
  return CP2_OK;
} catch (const std::bad_alloc&) {
  return CP2_ERR_ALLOC;   // nothing may unwind across the C ABI
} catch (...) {
  return CP2_ERR_INVALID;
}

// ---- persisted compact layers / roots (what a dataset that does not keep every node keeps) -------------------------------------------
int cp2i::kept_save(cp2_ctx* ctx, const char* path, CacheHead h, const void* d_buf, size_t bytes) {
  CP2_HIP(ctx, hipSetDevice(ctx->device));
  h.payload_bytes = bytes;
  return cache_save(ctx, path, h, d_buf);
}

int cp2i::kept_load(cp2_ctx* ctx, const char* path, const CacheHead& want, void* d_buf, size_t bytes) {
  const FdCloser f{open(path, O_RDONLY)};
  if (f.fd < 0) return CP2_ERR_IO;
  CacheHead h;
  CacheRefusal why;
  if (!cache_head_read(f.fd, &h, &why) || h.format != CacheFormat::Kept || !cache_same_items(h, want) || h.mode != want.mode ||
      h.payload_bytes != bytes)
    return CP2_ERR_IO;
  if (h.src == (uint64_t)CellSrc::File && h.stamps != file_stamps(h.base, h.first_item, h.n_items)) return CP2_ERR_IO;   // the slot files changed
  if (hipSetDevice(ctx->device) != hipSuccess) return CP2_ERR_HIP;
  const char* what = nullptr;
  return cache_load_payload(ctx, f.fd, h, d_buf, &what);
}
