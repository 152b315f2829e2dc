// The host side of a block repair (csrc/repair.cpp, cp2_multi_dataset_repair_blocks in multi_gpu.cpp): which requests are valid, where
// a request's block root is kept, which shard and unit hold it, how the matched blocks are written, and which cache stamps may follow
// the writes.  No HIP in here: tests/host_check/repair_plan_check.cpp walks it over random request sets on the CPU, under
// AddressSanitizer + UBSan.
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace cp2i {

// ---- validation -------------------------------------------------------------------------------------------------------------------
// Requests are (dataset slot, block of the slot) pairs, slot_block[2 i], slot_block[2 i + 1].  Every slot inside
// [first_slot, first_slot + n_local), every block below n_blocks, no pair twice.  false with *err naming the (lowest) request index
// that breaks a rule; for a duplicate, the later of the two.
inline bool repair_validate(const uint64_t* slot_block, size_t n, uint64_t first_slot, uint64_t n_local, uint64_t n_blocks, std::string* err) {
  for (size_t i = 0; i < n; ++i) {
    const uint64_t s = slot_block[2 * i], b = slot_block[2 * i + 1];
    if (s < first_slot || s - first_slot >= n_local) {
      *err = "repair: request " + std::to_string(i) + ": slot " + std::to_string(s) + " is not inside the local range " +
             std::to_string(first_slot) + " + " + std::to_string(n_local);
      return false;
    }
    if (b >= n_blocks) {
      *err = "repair: request " + std::to_string(i) + ": block " + std::to_string(b) + " of slot " + std::to_string(s) + " is not below nBlocks = " +
             std::to_string(n_blocks);
      return false;
    }
  }
  std::vector<size_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = i;
  auto key_less = [&](size_t a, size_t b) {
    if (slot_block[2 * a] != slot_block[2 * b]) return slot_block[2 * a] < slot_block[2 * b];
    if (slot_block[2 * a + 1] != slot_block[2 * b + 1]) return slot_block[2 * a + 1] < slot_block[2 * b + 1];
    return a < b;
  };
  std::sort(order.begin(), order.end(), key_less);
  size_t worst = n;                                   // the lowest index that repeats an earlier request
  for (size_t k = 1; k < n; ++k) {
    const size_t a = order[k - 1], b = order[k];
    if (slot_block[2 * a] == slot_block[2 * b] && slot_block[2 * a + 1] == slot_block[2 * b + 1]) worst = std::min(worst, b);
  }
  if (worst < n) {
    size_t first = worst;
    for (size_t i = 0; i < worst; ++i)
      if (slot_block[2 * i] == slot_block[2 * worst] && slot_block[2 * i + 1] == slot_block[2 * worst + 1]) { first = i; break; }
    *err = "repair: request " + std::to_string(worst) + ": (slot " + std::to_string(slot_block[2 * worst]) + ", block " +
           std::to_string(slot_block[2 * worst + 1]) + ") is request " + std::to_string(first) + " again";
    return false;
  }
  return true;
}

// ---- where the kept block root is (32-byte rows of the dataset's node buffer) ------------------------------------------------------
// every node kept (cp2_slot_trees, layer-major): the last block-tree layer, boff.back(), one row per block (bsizes.back() == 1) of
// block (local * nblocks + block); the same row as layer 0 of the big trees, toff[0] + local * tsizes[0] + block
inline uint64_t repair_row_full(uint64_t boff_last, uint64_t bsize_last, uint64_t nblocks, uint64_t local, uint64_t block) {
  return boff_last + (local * nblocks + block) * bsize_last;
}
// compact: layer 0 of the kept layers, coff[0] + local * csizes[0] + block
inline uint64_t repair_row_compact(uint64_t coff0, uint64_t csize0, uint64_t local, uint64_t block) { return coff0 + local * csize0 + block; }

// ---- shards and units --------------------------------------------------------------------------------------------------------------
// A slot cut into `units_per_slot` units of nblocks / units_per_slot blocks each: block b of slot s is block b % per of unit
// s * units_per_slot + b / per.
struct UnitBlock { uint64_t unit, block; };
inline UnitBlock repair_unit_of(uint64_t slot, uint64_t block, uint64_t units_per_slot, uint64_t blocks_per_unit) {
  return {slot * units_per_slot + block / blocks_per_unit, block % blocks_per_unit};
}
// the shard whose item range [first[k], first[k] + count[k]) holds `item`, or shards.size() when none does
inline size_t repair_shard_of(const std::vector<uint64_t>& first, const std::vector<uint64_t>& count, uint64_t item) {
  for (size_t k = 0; k < first.size(); ++k)
    if (item >= first[k] && item - first[k] < count[k]) return k;
  return first.size();
}

// ---- writes ------------------------------------------------------------------------------------------------------------------------
// The matched requests grouped by slot file, files in ascending slot order, each file's blocks in ascending offset order: the writer
// opens every file once, writes its blocks front to back and syncs it once after the last.
struct WriteGroup {
  uint64_t slot = 0;
  std::vector<size_t> reqs;                           // request indices, ascending block
};
inline std::vector<WriteGroup> repair_write_groups(const uint64_t* slot_block, const std::vector<size_t>& matched) {
  std::vector<size_t> order(matched);
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    if (slot_block[2 * a] != slot_block[2 * b]) return slot_block[2 * a] < slot_block[2 * b];
    return slot_block[2 * a + 1] < slot_block[2 * b + 1];
  });
  std::vector<WriteGroup> g;
  for (size_t i : order) {
    if (g.empty() || g.back().slot != slot_block[2 * i]) {
      g.emplace_back();
      g.back().slot = slot_block[2 * i];
    }
    g.back().reqs.push_back(i);
  }
  return g;
}

// One file of the writer (repair_write_rows in repair.cpp; the threaded writer of repair_many_plan.hpp): opened once (created with mode
// 0644 where it is missing), row q of its n rows -- block_size bytes at row_of(q) -- written with pwrite at byte offset off_of(q) in the
// order given, synced once after the last, closed.  0, or what stopped it: the errno, REPAIR_WRITE_NO_PROGRESS for a pwrite that wrote
// nothing.  Touches nothing but its own file and its arguments, so different files may be written from different threads.
constexpr int REPAIR_WRITE_NO_PROGRESS = -1;
template <typename OffOf, typename RowOf>
inline int repair_write_file(const std::string& name, size_t block_size, size_t n, OffOf off_of, RowOf row_of) {
  int what = 0;
  const int fd = open(name.c_str(), O_WRONLY | O_CREAT | O_CLOEXEC, 0644);
  if (fd < 0) return errno ? errno : EIO;
  for (size_t q = 0; !what && q < n; ++q) {
    const uint8_t* p = row_of(q);
    size_t left = block_size;
    off_t off = (off_t)off_of(q);
    while (left) {
      const ssize_t w = pwrite(fd, p, left, off);
      if (w < 0 && errno == EINTR) continue;
      if (w <= 0) { what = w < 0 ? errno : REPAIR_WRITE_NO_PROGRESS; break; }
      p += w; left -= (size_t)w; off += w;
    }
  }
  if (!what && fdatasync(fd) != 0) what = errno;
  if (close(fd) != 0 && !what) what = errno;
  return what;
}
inline std::string repair_write_reason(int what) { return what == REPAIR_WRITE_NO_PROGRESS ? "no progress" : std::strerror(what); }

// ---- cache stamps ------------------------------------------------------------------------------------------------------------------
// A cache holds one (size, mtime_ns) stamp per item (slot, or unit: several units stamp the file of their slot); a missing file stamps
// as (~0, ~0).  After the writes, an item's stamp is replaced by the file's new stat only when its file was WRITTEN by this call and the
// stamp equalled that file's stat taken before the call's first write: a cache that was already stale for the file (the damage itself
// changed the mtime) must stay stale.  Returns the item indices whose stamp changes; `stamps` is updated in place.
struct FileStamp {
  uint64_t slot = 0;
  uint64_t before[2] = {~0ULL, ~0ULL}, after[2] = {~0ULL, ~0ULL};
};
// the (size, mtime_ns) stamp of a file as the caches hold it; false and (~0, ~0) for a file that is not there
inline bool repair_stat_stamp(const std::string& path, uint64_t out[2]) {
  struct stat sb;
  if (stat(path.c_str(), &sb) != 0) { out[0] = out[1] = ~0ULL; return false; }
  out[0] = (uint64_t)sb.st_size;
  out[1] = (uint64_t)sb.st_mtim.tv_sec * 1000000000ULL + (uint64_t)sb.st_mtim.tv_nsec;
  return true;
}
inline std::vector<size_t> repair_restamp(std::vector<uint64_t>& stamps, uint64_t first_item, uint64_t units_per_slot,
                                          const std::vector<FileStamp>& written) {
  std::vector<size_t> changed;
  const size_t n = stamps.size() / 2;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t slot = (first_item + i) / units_per_slot;
    for (const FileStamp& f : written) {
      if (f.slot != slot) continue;
      if (stamps[2 * i] == f.before[0] && stamps[2 * i + 1] == f.before[1] &&
          (stamps[2 * i] != f.after[0] || stamps[2 * i + 1] != f.after[1])) {
        stamps[2 * i] = f.after[0];
        stamps[2 * i + 1] = f.after[1];
        changed.push_back(i);
      }
      break;
    }
  }
  return changed;
}

}  // namespace cp2i
