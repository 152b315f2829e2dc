// The library's own cache files, host side: the tree cache ("CP2TREE3": every node of a batch of slot trees) and the kept form
// ("CP2KEPT1": what a compact or roots-only dataset keeps).  One layout for both: a 104-byte header (8 magic bytes + twelve u64), the
// slot-file base name, one (size, mtime_ns) stamp per item for the SlotFile source (outside the checksum), the payload under a
// Checksum64.  Here: the one head reader and writer, the stamps and their rewrite after a repair, the tmp-file writer the cache files and the
// fill checkpoints go through, the fd helpers; the payload's way between device and file is cache_file.cpp.  No HIP in here:
// tests/host_check/cache_file_check.cpp runs it against real files on the CPU, under AddressSanitizer + UBSan.
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/codex_p2.h"
#include "checksum64.hpp"
#include "fill_pipeline.hpp"   // fill_slot_file_name
#include "repair_plan.hpp"     // repair_restamp, FileStamp

enum class CellSrc { Fake, Dev, Host, File };   // where the cells of a batch of trees come from (trees.hpp)

namespace cp2i {

// ---- descriptors ------------------------------------------------------------------------------------------------------------------
struct FdCloser { int fd; ~FdCloser() { if (fd >= 0) close(fd); } };

// all n bytes at `off` through pread / pwrite: an interrupted call is repeated, an error or the end of the file is false
template <class Io, class Byte>
bool io_all(Io io, int fd, Byte* p, size_t n, off_t off) {
  while (n) {
    const ssize_t k = io(fd, p, n, off);
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) return false;
    p += k; n -= (size_t)k; off += k;
  }
  return true;
}
inline bool pwrite_all(int fd, const uint8_t* p, size_t n, off_t off) { return io_all(::pwrite, fd, p, n, off); }
inline bool pread_all(int fd, uint8_t* p, size_t n, off_t off) { return io_all(::pread, fd, p, n, off); }

// does the file at `path` start with these eight bytes?  (false for a file that cannot be opened, too)
inline bool file_has_magic(const char* path, const char* magic8) {
  char m[8] = {};
  const FdCloser f{open(path, O_RDONLY | O_CLOEXEC)};
  return f.fd >= 0 && pread(f.fd, m, 8, 0) == 8 && std::memcmp(m, magic8, 8) == 0;
}

// A file written beside its place and renamed into it: "<path>.tmp.<pid>", never through a link at that name, removed again unless
// commit() got it to `path` -- so whatever stood at `path` stays whole until the new file is.  ok() false (errno says why): the tmp
// file could not be created.  commit(sync): fsync when asked, close, rename; false with the errno of the first step that failed.
class TmpFile {
 public:
  explicit TmpFile(const std::string& path)
      : path_(path), tmp_(path + ".tmp." + std::to_string((long)getpid())),
        fd_(open(tmp_.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_NOFOLLOW | O_CLOEXEC, 0644)), mine_(fd_ >= 0) {}
  TmpFile(const TmpFile&) = delete;
  ~TmpFile() { if (fd_ >= 0) close(fd_); if (mine_) std::remove(tmp_.c_str()); }
  bool ok() const { return fd_ >= 0; }
  int fd() const { return fd_; }
  const std::string& tmp_name() const { return tmp_; }
  bool commit(bool sync) {
    bool good = !sync || fsync(fd_) == 0;
    int why = errno;
    if (close(fd_) != 0 && good) { good = false; why = errno; }
    fd_ = -1;
    if (good && std::rename(tmp_.c_str(), path_.c_str()) != 0) { good = false; why = errno; }
    if (good) mine_ = false;
    errno = why;
    return good;
  }

 private:
  std::string path_, tmp_;
  int fd_;
  bool mine_;   // the tmp file exists and is this object's to remove
};

// ---- stamps -----------------------------------------------------------------------------------------------------------------------
// (size, mtime in ns) of the slot file behind each item (slot, or unit: several units then stamp the same file); a missing file
// stamps as (~0, ~0)
inline std::vector<uint64_t> file_stamps(const std::string& base, uint64_t first_item, size_t n_items, uint64_t units_per_slot = 1) {
  std::vector<uint64_t> v(2 * n_items, ~0ULL);
  for (size_t s = 0; s < n_items; ++s) {
    struct stat sb;
    if (stat(fill_slot_file_name(base, (first_item + s) / units_per_slot).c_str(), &sb) != 0) continue;
    v[2 * s] = (uint64_t)sb.st_size;
    v[2 * s + 1] = (uint64_t)sb.st_mtim.tv_sec * 1000000000ULL + (uint64_t)sb.st_mtim.tv_nsec;
  }
  return v;
}

// ---- the head of a cache file -----------------------------------------------------------------------------------------------------
enum class CacheFormat { Tree, Kept };
constexpr uint64_t CACHE_HEADER_BYTES = 104, CACHE_BASE_MAX = 4096;

// Everything before the payload.  Items are slots, or (tree cache, units_per_slot > 1) units of a slot: n_cells then counts the cells
// of one unit.  A tree cache's payload is its node buffer (the file counts it in 32-byte nodes); a kept file's is the layers of `mode`
// (2 compact, 0 roots only).
struct CacheHead {
  CacheFormat format = CacheFormat::Tree;
  uint64_t n_items = 0, cell_size = 0, block_size = 0, n_cells = 0;
  uint64_t units_per_slot = 1;          // a kept file: always 1
  uint64_t src = 0, seed = 0, first_item = 0;   // src: a CellSrc
  uint64_t mode = 0;                    // a kept file only
  std::string base;                     // the slot-file base name (SlotFile source), at most CACHE_BASE_MAX bytes
  std::vector<uint64_t> stamps;         // (size, mtime_ns) per item: present exactly for the SlotFile source
  uint64_t payload_bytes = 0, checksum = 0;
  uint64_t payload_off() const { return CACHE_HEADER_BYTES + base.size() + stamps.size() * 8; }
};

enum class CacheRefusal { None, NotThisVersion, Truncated, Unreadable };

// The header as the files hold it: 8 magic bytes, then twelve u64 (little-endian: the host's), in this order:
//   "CP2TREE3"  n_items cell_size block_size n_cells units_per_slot src seed first_item   base_len n_stamps n_nodes       checksum
//   "CP2KEPT1"  n_items cell_size block_size n_cells src seed first_item mode             base_len n_stamps payload_bytes checksum
// (a tree cache counts its payload in 32-byte nodes).
//
// The head of the cache file open at `fd`.  The magic is recognised and every field bounded before anything is sized from it, and the
// file is at least header + base name + stamps long before those are read.  false with *why set: the header's own fields are in `head`
// then unless *why is NotThisVersion, base name and stamps are not.
inline bool cache_head_read(int fd, CacheHead* head, CacheRefusal* why) {
  uint8_t raw[CACHE_HEADER_BYTES];
  uint64_t w[12];
  CacheHead& h = *head;
  h = CacheHead();
  *why = CacheRefusal::NotThisVersion;
  if (!pread_all(fd, raw, sizeof raw, 0)) return false;
  std::memcpy(w, raw + 8, sizeof w);
  const bool tree = std::memcmp(raw, "CP2TREE3", 8) == 0;
  if (!tree && std::memcmp(raw, "CP2KEPT1", 8) != 0) return false;
  h.format = tree ? CacheFormat::Tree : CacheFormat::Kept;
  h.n_items = w[0]; h.cell_size = w[1]; h.block_size = w[2]; h.n_cells = w[3];
  if (tree) { h.units_per_slot = w[4]; h.src = w[5]; h.seed = w[6]; h.first_item = w[7]; }
  else { h.src = w[4]; h.seed = w[5]; h.first_item = w[6]; h.mode = w[7]; }
  const uint64_t base_len = w[8], n_stamps = w[9], unit = tree ? 32 : 1;
  if (base_len > CACHE_BASE_MAX || h.src > (uint64_t)CellSrc::File || h.units_per_slot == 0 || w[10] > ~0ULL / unit ||
      (n_stamps != 0 && n_stamps != h.n_items) || (h.src == (uint64_t)CellSrc::File) != (n_stamps != 0))
    return false;
  h.payload_bytes = w[10] * unit;
  h.checksum = w[11];
  *why = CacheRefusal::Truncated;
  struct stat sb;
  if (fstat(fd, &sb) != 0 || n_stamps > ((uint64_t)1 << 40) || (uint64_t)sb.st_size < sizeof raw + base_len + 16 * n_stamps) return false;
  *why = CacheRefusal::Unreadable;
  h.base.assign(base_len, '\0');
  if (base_len && !pread_all(fd, reinterpret_cast<uint8_t*>(&h.base[0]), base_len, sizeof raw)) return false;
  h.stamps.assign(2 * n_stamps, 0);
  if (n_stamps && !pread_all(fd, reinterpret_cast<uint8_t*>(h.stamps.data()), h.stamps.size() * 8, (off_t)(sizeof raw + base_len))) return false;
  *why = CacheRefusal::None;
  return true;
}

// header + base name + stamps exactly as the file starts: payload_off() bytes
inline std::vector<uint8_t> cache_head_bytes(const CacheHead& h) {
  const bool tree = h.format == CacheFormat::Tree;
  std::vector<uint64_t> w = tree ? std::vector<uint64_t>{h.n_items, h.cell_size, h.block_size, h.n_cells, h.units_per_slot, h.src, h.seed, h.first_item}
                                 : std::vector<uint64_t>{h.n_items, h.cell_size, h.block_size, h.n_cells, h.src, h.seed, h.first_item, h.mode};
  w.insert(w.end(), {(uint64_t)h.base.size(), (uint64_t)h.stamps.size() / 2, h.payload_bytes / (tree ? 32 : 1), h.checksum});
  std::vector<uint8_t> out(h.payload_off());
  std::memcpy(out.data(), tree ? "CP2TREE3" : "CP2KEPT1", 8);
  std::memcpy(out.data() + 8, w.data(), 96);
  if (!h.base.empty()) std::memcpy(out.data() + CACHE_HEADER_BYTES, h.base.data(), h.base.size());
  if (!h.stamps.empty()) std::memcpy(out.data() + CACHE_HEADER_BYTES + h.base.size(), h.stamps.data(), h.stamps.size() * 8);
  return out;
}

// do the two heads describe the same items of the same data?  Counts, geometry, source, first item, units per slot and base name; the
// seed where the data is generated from it.  Neither the format nor what is kept of the items (mode, payload) is looked at.
inline bool cache_same_items(const CacheHead& a, const CacheHead& b) {
  return a.n_items == b.n_items && a.cell_size == b.cell_size && a.block_size == b.block_size && a.n_cells == b.n_cells && a.src == b.src &&
         a.first_item == b.first_item && a.units_per_slot == b.units_per_slot && a.base == b.base &&
         (a.src != (uint64_t)CellSrc::Fake || a.seed == b.seed);
}

// ---- the kept form ----------------------------------------------------------------------------------------------------------------
// the head of the kept form of local slots [first_slot, + n_local) of a dataset of `cfg` in `mode`; stamps and payload are the saver's
inline CacheHead kept_meta(const cp2_config& cfg, uint64_t first_slot, uint64_t n_local, bool from_file, const std::string& file_base, int mode) {
  CacheHead h;
  h.format = CacheFormat::Kept;
  h.n_items = n_local; h.cell_size = cfg.cell_size; h.block_size = cfg.block_size; h.n_cells = cfg.n_cells;
  h.src = (uint64_t)(from_file ? CellSrc::File : CellSrc::Fake); h.seed = cfg.seed; h.first_item = first_slot;
  h.mode = (uint64_t)mode; h.base = file_base;
  return h;
}

// where a kept form is written: a tree cache at the path is the richer representation and stays, the kept form goes beside it
inline std::string kept_cache_path(const char* cache_path) {
  return file_has_magic(cache_path, "CP2TREE3") ? std::string(cache_path) + ".kept" : std::string(cache_path);
}

// ---- stamps of a cache after a block repair (repair.cpp) --------------------------------------------------------------------------
// The per-item stamps of the cache file at `path`, of either format, when it describes exactly the items of `want` (slot-file data):
// the stamps of items whose file this call wrote follow the writes by repair_restamp's rule (repair_plan.hpp), with pwrite and fdatasync
// in place.  *restamped = how many changed; no file, or one of other items, is left alone (CP2_OK, 0).  CP2_ERR_IO: it cannot be rewritten.
inline int cache_restamp(const char* path, const CacheHead& want, const std::vector<FileStamp>& written, size_t* restamped, std::string* err) {
  *restamped = 0;
  const FdCloser f{open(path, O_RDWR | O_NOFOLLOW | O_CLOEXEC)};
  if (f.fd < 0) return CP2_OK;                                    // no cache there: nothing to keep valid
  CacheHead h;
  CacheRefusal why;
  if (!cache_head_read(f.fd, &h, &why) || h.src != (uint64_t)CellSrc::File || !cache_same_items(h, want)) return CP2_OK;
  const std::vector<size_t> changed = repair_restamp(h.stamps, h.first_item, h.units_per_slot, written);
  for (size_t i : changed)
    if (!pwrite_all(f.fd, reinterpret_cast<const uint8_t*>(&h.stamps[2 * i]), 16, (off_t)(CACHE_HEADER_BYTES + h.base.size() + 16 * i))) {
      *err = std::string("cannot restamp ") + path + ": " + std::strerror(errno);
      return CP2_ERR_IO;
    }
  if (!changed.empty() && fdatasync(f.fd) != 0) {
    *err = std::string("cannot sync ") + path + ": " + std::strerror(errno);
    return CP2_ERR_IO;
  }
  *restamped = changed.size();
  return CP2_OK;
}

}  // namespace cp2i
