// The host side of the library's cache files (csrc/cache_file.hpp, the header cache_file.cpp, fill.cpp, proof_input.cpp and repair.cpp
// use) against REAL files in a scratch directory: the byte image of a head of either format against one assembled here from the field
// order written out below, and back through cache_head_read; every refusal, each a one-field damage of a good file; cache_restamp over
// real "slot files" (exactly the 16 bytes of each changed stamp differ; a cache of other items stays byte-identical); the tmp-file
// writer; and the golden files of tests/golden/cache_files parsed and their payload checksummed -- the whole load path except the
// upload.  Built with AddressSanitizer + UBSan: a refusal that sized anything from the damaged field would not get past them.  No GPU.
//   g++ -std=c++17 -pthread -fsanitize=address,undefined -I<csrc> cache_file_check.cpp -o check && ./check <scratch dir> [<golden dir>]
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cache_file.hpp"

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

using Bytes = std::vector<uint8_t>;

static void put_u64(Bytes& b, uint64_t v) { for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(v >> (8 * i))); }   // little-endian
static void set_u64(Bytes& b, size_t at, uint64_t v) { for (int i = 0; i < 8; ++i) b[at + i] = (uint8_t)(v >> (8 * i)); }

static void put_file(const std::string& name, const Bytes& b) {
  FILE* f = std::fopen(name.c_str(), "wb");
  if (!f || (!b.empty() && std::fwrite(b.data(), 1, b.size(), f) != b.size())) { std::printf("cannot write %s\n", name.c_str()); std::exit(2); }
  std::fclose(f);
}
static Bytes get_file(const std::string& name) {
  Bytes b;
  FILE* f = std::fopen(name.c_str(), "rb");
  if (!f) return b;
  uint8_t buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + n);
  std::fclose(f);
  return b;
}
// how many names in `dir` contain ".tmp."
static size_t tmp_files_in(const std::string& dir) {
  size_t n = 0;
  DIR* d = opendir(dir.c_str());
  if (!d) return 0;
  while (dirent* e = readdir(d)) n += std::string(e->d_name).find(".tmp.") != std::string::npos;
  closedir(d);
  return n;
}

// ---- the layout, restated: 8 magic bytes + twelve little-endian u64 = 104 bytes, then the base name, then the stamps ------------------
// word index of each field, per format
enum TreeWord { T_N_SLOTS, T_CELL_SIZE, T_BLOCK_SIZE, T_N_CELLS, T_UNITS_PER_SLOT, T_SRC, T_SEED, T_FIRST_SLOT, T_BASE_LEN, T_N_STAMPS, T_N_NODES, T_CHECKSUM };
enum KeptWord { K_N_SLOTS, K_CELL_SIZE, K_BLOCK_SIZE, K_N_CELLS, K_SRC, K_SEED, K_FIRST_SLOT, K_MODE, K_BASE_LEN, K_N_STAMPS, K_PAYLOAD_BYTES, K_CHECKSUM };
static size_t word_at(int w) { return 8 + 8 * (size_t)w; }

static Bytes image_of(const CacheHead& h) {
  Bytes b;
  const char* magic = h.format == CacheFormat::Tree ? "CP2TREE3" : "CP2KEPT1";
  b.insert(b.end(), magic, magic + 8);
  if (h.format == CacheFormat::Tree) {
    for (uint64_t v : {h.n_items, h.cell_size, h.block_size, h.n_cells, h.units_per_slot, h.src, h.seed, h.first_item, (uint64_t)h.base.size(),
                       (uint64_t)h.stamps.size() / 2, h.payload_bytes / 32, h.checksum})
      put_u64(b, v);
  } else {
    for (uint64_t v : {h.n_items, h.cell_size, h.block_size, h.n_cells, h.src, h.seed, h.first_item, h.mode, (uint64_t)h.base.size(),
                       (uint64_t)h.stamps.size() / 2, h.payload_bytes, h.checksum})
      put_u64(b, v);
  }
  b.insert(b.end(), h.base.begin(), h.base.end());
  for (uint64_t v : h.stamps) put_u64(b, v);
  return b;
}

static bool same_head(const CacheHead& a, const CacheHead& b) {
  return a.format == b.format && a.n_items == b.n_items && a.cell_size == b.cell_size && a.block_size == b.block_size && a.n_cells == b.n_cells &&
         a.units_per_slot == b.units_per_slot && a.src == b.src && a.seed == b.seed && a.first_item == b.first_item && a.mode == b.mode &&
         a.base == b.base && a.stamps == b.stamps && a.payload_bytes == b.payload_bytes && a.checksum == b.checksum;
}

// a good head: `file` = the SlotFile source (base name and one stamp per item), else the fake source
static CacheHead good_head(CacheFormat format, bool file) {
  CacheHead h;
  h.format = format;
  h.n_items = 3; h.cell_size = 64; h.block_size = 256; h.n_cells = 16;
  h.units_per_slot = format == CacheFormat::Tree ? 2 : 1;
  h.src = (uint64_t)(file ? CellSrc::File : CellSrc::Fake);
  h.seed = 0x1122334455667788ULL; h.first_item = 5;
  h.mode = format == CacheFormat::Kept ? 2 : 0;
  if (file) {
    h.base = "some/dir/slot";
    for (uint64_t i = 0; i < 2 * h.n_items; ++i) h.stamps.push_back(0xa0b0c0d000000000ULL + i);
  }
  h.payload_bytes = 96; h.checksum = 0x0123456789abcdefULL;
  return h;
}

static Bytes payload_of(size_t n) {
  Bytes p(n);
  for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)(i * 7 + 1);
  return p;
}

// cache_head_read of the file holding `bytes`
static bool read_bytes(const std::string& name, const Bytes& bytes, CacheHead* h, CacheRefusal* why) {
  put_file(name, bytes);
  const FdCloser f{open(name.c_str(), O_RDONLY)};
  if (f.fd < 0) { std::printf("cannot open %s\n", name.c_str()); std::exit(2); }
  return cache_head_read(f.fd, h, why);
}

static size_t check_images_and_refusals(const std::string& dir) {
  const std::string name = dir + "/head.bin";
  size_t refused = 0;
  CacheHead got;
  CacheRefusal why;
  auto refuse = [&](const Bytes& bytes, CacheRefusal want, const char* what) {
    const bool ok = read_bytes(name, bytes, &got, &why);
    CHECK(!ok && why == want, "%s: read %d, refusal %d (wanted %d)", what, (int)ok, (int)why, (int)want);
    ++refused;
  };
  for (CacheFormat format : {CacheFormat::Tree, CacheFormat::Kept}) {
    const bool tree = format == CacheFormat::Tree;
    const int w_n_items = tree ? (int)T_N_SLOTS : (int)K_N_SLOTS, w_base_len = tree ? (int)T_BASE_LEN : (int)K_BASE_LEN,
              w_n_stamps = tree ? (int)T_N_STAMPS : (int)K_N_STAMPS;
    for (bool file : {false, true}) {
      const CacheHead h = good_head(format, file);
      const Bytes image = image_of(h);
      CHECK(image.size() == 104 + h.base.size() + 8 * h.stamps.size() && image.size() == h.payload_off(), "image of %zu bytes", image.size());
      CHECK(cache_head_bytes(h) == image, "cache_head_bytes differs from the restated image (format %d, file %d)", (int)format, (int)file);
      Bytes whole = image;
      const Bytes payload = payload_of(h.payload_bytes);
      whole.insert(whole.end(), payload.begin(), payload.end());
      const bool ok = read_bytes(name, whole, &got, &why);
      CHECK(ok && why == CacheRefusal::None && same_head(got, h), "a good file does not come back (format %d, file %d)", (int)format, (int)file);
      CHECK(ok && cache_head_bytes(got) == image, "the head read does not give the image back");

      // ---- one-field damages of this good file
      for (const char* magic : {"CP2TREE1", "CP2TREE2", "CP2KEPT0", "CP2FILL1"}) {
        Bytes bad = whole;
        std::memcpy(bad.data(), magic, 8);
        refuse(bad, CacheRefusal::NotThisVersion, magic);
      }
      { Bytes bad = whole; set_u64(bad, word_at(w_base_len), 4097); refuse(bad, CacheRefusal::NotThisVersion, "file_base_len 4097"); }
      { Bytes bad = whole; set_u64(bad, word_at(w_base_len), ~0ULL); refuse(bad, CacheRefusal::NotThisVersion, "file_base_len 2^64 - 1"); }
      for (uint64_t n : {(uint64_t)1, h.n_items - 1, h.n_items + 1, ~(uint64_t)0}) {
        Bytes bad = whole; set_u64(bad, word_at(w_n_stamps), n); refuse(bad, CacheRefusal::NotThisVersion, "n_stamps neither 0 nor the item count");
      }
      if (file) { Bytes bad = whole; set_u64(bad, word_at(w_n_stamps), 0); refuse(bad, CacheRefusal::NotThisVersion, "slot-file source without stamps"); }
      else { Bytes bad = whole; set_u64(bad, word_at(w_n_stamps), h.n_items); refuse(bad, CacheRefusal::NotThisVersion, "fake source with stamps"); }
      if (file) {                                        // as many stamps as items, more than any file holds: nothing may be sized from the count
        for (uint64_t n : {((uint64_t)1 << 40) + 1, (uint64_t)1 << 59, ~(uint64_t)0}) {
          Bytes bad = whole;
          set_u64(bad, word_at(w_n_items), n);
          set_u64(bad, word_at(w_n_stamps), n);
          refuse(bad, CacheRefusal::Truncated, "n_stamps above 2^40");
        }
      }
      for (size_t len : {(size_t)0, (size_t)7, (size_t)8, (size_t)103}) refuse(Bytes(whole.begin(), whole.begin() + len), CacheRefusal::NotThisVersion, "shorter than the header");
      if (file) {                                        // header whole, base name or stamps cut: refused before either is read
        for (size_t len : {(size_t)104, (size_t)104 + h.base.size(), image.size() - 1})
          refuse(Bytes(whole.begin(), whole.begin() + len), CacheRefusal::Truncated, "shorter than header + base + stamps");
      }
      CHECK(read_bytes(name, image, &got, &why) && same_head(got, h), "a file that ends where its payload starts still has a head");
    }
  }
  {   // a tree cache counts its payload in nodes: a count whose bytes do not fit 64 bits is refused, and zero units per slot
    const CacheHead h = good_head(CacheFormat::Tree, false);
    Bytes bad = image_of(h); set_u64(bad, word_at(T_N_NODES), ((uint64_t)1 << 59) + 1); refuse(bad, CacheRefusal::NotThisVersion, "n_nodes past 2^59");
    bad = image_of(h); set_u64(bad, word_at(T_UNITS_PER_SLOT), 0); refuse(bad, CacheRefusal::NotThisVersion, "units_per_slot 0");
    bad = image_of(h); set_u64(bad, word_at(T_SRC), 4); refuse(bad, CacheRefusal::NotThisVersion, "an unknown source");
  }
  unlink(name.c_str());
  return refused;
}

// ---- restamp -----------------------------------------------------------------------------------------------------------------------
static void stat_of(const std::string& name, uint64_t out[2]) {
  struct stat sb;
  if (stat(name.c_str(), &sb) != 0) { out[0] = out[1] = ~0ULL; return; }
  out[0] = (uint64_t)sb.st_size;
  out[1] = (uint64_t)sb.st_mtim.tv_sec * 1000000000ULL + (uint64_t)sb.st_mtim.tv_nsec;
}

static size_t check_restamp(const std::string& dir) {
  size_t cases = 0;
  const std::string base = dir + "/slot";
  for (CacheFormat format : {CacheFormat::Tree, CacheFormat::Kept}) {
    const bool tree = format == CacheFormat::Tree;
    // the tree cache holds units 4 .. 7 of slots cut in two (slots 2 and 3), the kept file slots 2 .. 4
    CacheHead h = good_head(format, true);
    h.base = base;
    h.units_per_slot = tree ? 2 : 1;
    h.first_item = tree ? 4 : 2;
    h.n_items = tree ? 4 : 3;
    for (uint64_t s = 2; s <= 4; ++s) put_file(fill_slot_file_name(base, s), payload_of(100 + (size_t)s));
    h.stamps = file_stamps(base, h.first_item, h.n_items, h.units_per_slot);
    CHECK(h.stamps.size() == 2 * h.n_items && h.stamps[0] == 102, "stamps of real files");
    const std::string cache = dir + (tree ? "/tree.cp2" : "/kept.cp2");
    Bytes whole = cache_head_bytes(h);
    const Bytes payload = payload_of(h.payload_bytes);
    whole.insert(whole.end(), payload.begin(), payload.end());
    put_file(cache, whole);

    // slot 3 is rewritten, as a repair does: its stamp before the write and after it
    FileStamp w;
    w.slot = 3;
    stat_of(fill_slot_file_name(base, 3), w.before);
    put_file(fill_slot_file_name(base, 3), payload_of(333));
    const struct timespec later[2] = {{0, UTIME_OMIT}, {(time_t)2000000000, 123456789}};
    utimensat(AT_FDCWD, fill_slot_file_name(base, 3).c_str(), later, 0);
    stat_of(fill_slot_file_name(base, 3), w.after);
    CHECK(w.before[0] == 103 && w.after[0] == 333 && w.after[1] == 2000000000ULL * 1000000000ULL + 123456789, "the rewritten file's stamps");
    const std::vector<FileStamp> written{w};

    // a cache that describes other items: each describing field in turn differs, the file stays as it is
    CacheHead want;
    want.n_items = h.n_items; want.cell_size = h.cell_size; want.block_size = h.block_size; want.n_cells = h.n_cells; want.src = (uint64_t)CellSrc::File;
    want.first_item = h.first_item; want.units_per_slot = h.units_per_slot; want.base = base;
    size_t n = 99;
    std::string err;
    auto left_alone = [&](const CacheHead& other, const char* what) {
      n = 99;
      CHECK(cache_restamp(cache.c_str(), other, written, &n, &err) == CP2_OK && n == 0, "%s: restamped %zu", what, n);
      CHECK(get_file(cache) == whole, "%s: the cache file changed", what);
      ++cases;
    };
    { CacheHead o = want; o.n_items += 1; left_alone(o, "another item count"); }
    { CacheHead o = want; o.cell_size *= 2; left_alone(o, "another cell size"); }
    { CacheHead o = want; o.block_size *= 2; left_alone(o, "another block size"); }
    { CacheHead o = want; o.n_cells *= 2; left_alone(o, "another cell count"); }
    { CacheHead o = want; o.first_item += 1; left_alone(o, "another first item"); }
    { CacheHead o = want; o.units_per_slot *= 2; left_alone(o, "other units per slot"); }
    { CacheHead o = want; o.base += "x"; left_alone(o, "another base name"); }
    { CacheHead o = want; o.base.pop_back(); left_alone(o, "a shorter base name"); }
    { CacheHead o = want; o.src = (uint64_t)CellSrc::Fake; left_alone(o, "another source"); }
    {   // no file at the path, and a file that is no cache
      n = 99;
      CHECK(cache_restamp((cache + ".absent").c_str(), want, written, &n, &err) == CP2_OK && n == 0, "no file: restamped %zu", n);
      const std::string other = dir + "/other.bin";
      const Bytes junk = payload_of(300);
      put_file(other, junk);
      n = 99;
      CHECK(cache_restamp(other.c_str(), want, written, &n, &err) == CP2_OK && n == 0 && get_file(other) == junk, "a file that is no cache");
      unlink(other.c_str());
      cases += 2;
    }

    // the cache of these items: exactly the 16 bytes of each stamp of slot 3 change, to the file's stat after the write
    n = 99;
    CHECK(cache_restamp(cache.c_str(), want, written, &n, &err) == CP2_OK, "restamp failed: %s", err.c_str());
    const std::vector<size_t> items = tree ? std::vector<size_t>{2, 3} : std::vector<size_t>{1};   // units 6, 7 of slot 3; slot 3
    CHECK(n == items.size(), "restamped %zu of %zu", n, items.size());
    Bytes expect = whole;
    for (size_t i : items) {
      set_u64(expect, 104 + base.size() + 16 * i, w.after[0]);
      set_u64(expect, 104 + base.size() + 16 * i + 8, w.after[1]);
    }
    const Bytes now = get_file(cache);
    CHECK(now == expect, "the restamped file is not the old one with the stamps of slot 3 replaced");
    size_t differing = 0;
    for (size_t i = 0; i < now.size() && i < whole.size(); ++i) differing += now[i] != whole[i];
    CHECK(differing > 0 && differing <= 16 * items.size(), "%zu bytes differ", differing);
    // the stamps now equal the files': a loader would accept them; a second restamp changes nothing
    CacheHead back;
    CacheRefusal why;
    {
      const FdCloser f{open(cache.c_str(), O_RDONLY)};
      CHECK(cache_head_read(f.fd, &back, &why) && back.stamps == file_stamps(base, h.first_item, h.n_items, h.units_per_slot), "stamps after the restamp");
    }
    n = 99;
    CHECK(cache_restamp(cache.c_str(), want, written, &n, &err) == CP2_OK && n == 0 && get_file(cache) == expect, "a second restamp");
    // a stamp that was stale before the write stays stale
    FileStamp stale = w;
    stale.slot = 2;
    stale.before[1] ^= 1;
    n = 99;
    CHECK(cache_restamp(cache.c_str(), want, {stale}, &n, &err) == CP2_OK && n == 0 && get_file(cache) == expect, "a stale stamp followed the write");
    cases += 3;
    unlink(cache.c_str());
    for (uint64_t s = 2; s <= 4; ++s) unlink(fill_slot_file_name(base, s).c_str());
  }
  return cases;
}

// ---- the tmp-file writer -----------------------------------------------------------------------------------------------------------
static size_t check_tmp_file(const std::string& dir) {
  size_t cases = 0;
  const std::string path = dir + "/out.bin";
  const Bytes older = payload_of(50), newer = payload_of(70);
  for (bool sync : {false, true}) {
    put_file(path, older);
    {
      TmpFile t(path);
      CHECK(t.ok() && t.tmp_name() == path + ".tmp." + std::to_string((long)getpid()), "tmp name %s", t.tmp_name().c_str());
      CHECK(pwrite_all(t.fd(), newer.data(), newer.size(), 0), "write");
      CHECK(get_file(path) == older && tmp_files_in(dir) == 1, "before the commit the older file stands");
      CHECK(t.commit(sync), "commit(%d): %s", (int)sync, std::strerror(errno));
      CHECK(!t.ok(), "a committed writer still has a descriptor");
    }
    CHECK(get_file(path) == newer && tmp_files_in(dir) == 0, "after commit(%d): %zu tmp files", (int)sync, tmp_files_in(dir));
    struct stat sb;
    CHECK(stat(path.c_str(), &sb) == 0 && (sb.st_mode & 0777 & ~0644) == 0, "mode %o", (unsigned)sb.st_mode);
    ++cases;
  }
  {   // destroyed without a commit: the older file stays whole, the tmp file goes
    put_file(path, older);
    {
      TmpFile t(path);
      CHECK(t.ok() && pwrite_all(t.fd(), newer.data(), newer.size(), 0), "write");
      CHECK(tmp_files_in(dir) == 1, "the tmp file is there while written");
    }
    CHECK(get_file(path) == older && tmp_files_in(dir) == 0, "no commit: the older file changed or the tmp file stayed");
    ++cases;
  }
  {   // a commit that cannot rename (the place is a directory that is not empty): false, errno set, the tmp file goes
    const std::string place = dir + "/place";
    mkdir(place.c_str(), 0755);
    put_file(place + "/inside", older);
    {
      TmpFile t(place);
      CHECK(t.ok() && pwrite_all(t.fd(), newer.data(), newer.size(), 0), "write");
      errno = 0;
      CHECK(!t.commit(false) && errno != 0, "a rename onto a directory succeeded");
    }
    CHECK(tmp_files_in(dir) == 0 && get_file(place + "/inside") == older, "after a failed commit");
    unlink((place + "/inside").c_str());
    rmdir(place.c_str());
    ++cases;
  }
  {   // a link at the tmp name is not followed, and is not this writer's to remove
    const std::string target = dir + "/target.bin", link = path + ".tmp." + std::to_string((long)getpid());
    put_file(target, older);
    CHECK(symlink(target.c_str(), link.c_str()) == 0, "symlink");
    {
      TmpFile t(path);
      CHECK(!t.ok() && errno == ELOOP, "a link at the tmp name was followed (errno %d)", errno);
    }
    struct stat sb;
    CHECK(get_file(target) == older && lstat(link.c_str(), &sb) == 0 && S_ISLNK(sb.st_mode), "the link or its target changed");
    unlink(link.c_str());
    unlink(target.c_str());
    ++cases;
  }
  {   // a directory that does not exist: not created, nothing to remove
    TmpFile t(dir + "/no/such/dir/out.bin");
    CHECK(!t.ok() && errno == ENOENT, "errno %d", errno);
    ++cases;
  }
  unlink(path.c_str());
  // file_has_magic and kept_cache_path: the kept form goes beside a tree cache, and only beside a tree cache
  const std::string cache = dir + "/c.cp2";
  CHECK(kept_cache_path(cache.c_str()) == cache && !file_has_magic(cache.c_str(), "CP2TREE3"), "no file at the path");
  put_file(cache, image_of(good_head(CacheFormat::Kept, false)));
  CHECK(kept_cache_path(cache.c_str()) == cache && file_has_magic(cache.c_str(), "CP2KEPT1"), "a kept file at the path");
  put_file(cache, image_of(good_head(CacheFormat::Tree, false)));
  CHECK(kept_cache_path(cache.c_str()) == cache + ".kept" && file_has_magic(cache.c_str(), "CP2TREE3"), "a tree cache at the path");
  put_file(cache, Bytes{'C', 'P', '2', 'T', 'R', 'E', 'E'});
  CHECK(kept_cache_path(cache.c_str()) == cache, "seven bytes of a magic");
  unlink(cache.c_str());
  // kept_meta: every field from where it belongs
  cp2_config cfg{};
  cfg.cell_size = 64; cfg.block_size = 256; cfg.n_cells = 16; cfg.n_slots = 9; cfg.seed = 77;
  const CacheHead m = kept_meta(cfg, 5, 3, true, "b/", 2);
  CHECK(m.format == CacheFormat::Kept && m.n_items == 3 && m.cell_size == 64 && m.block_size == 256 && m.n_cells == 16 && m.units_per_slot == 1 &&
        m.src == (uint64_t)CellSrc::File && m.seed == 77 && m.first_item == 5 && m.mode == 2 && m.base == "b/" && m.stamps.empty(), "kept_meta");
  CHECK(kept_meta(cfg, 0, 9, false, "", 0).src == (uint64_t)CellSrc::Fake, "kept_meta: the fake source");
  return cases + 2;
}

// ---- golden files ------------------------------------------------------------------------------------------------------------------
// every field of the head on one line (the caller compares it with the configuration that wrote the file), after the head has given
// its own bytes back and the payload its checksum
static void check_golden(const std::string& name, const std::string& file) {
  const Bytes whole = get_file(name);
  const FdCloser f{open(name.c_str(), O_RDONLY)};
  CacheHead h;
  CacheRefusal why = CacheRefusal::None;
  if (f.fd < 0 || !cache_head_read(f.fd, &h, &why)) {
    CHECK(false, "%s: no head (refusal %d)", name.c_str(), (int)why);
    return;
  }
  CHECK(whole.size() == h.payload_off() + h.payload_bytes, "%s: %zu bytes, the head states %llu", name.c_str(), whole.size(),
        (unsigned long long)(h.payload_off() + h.payload_bytes));
  if (whole.size() != h.payload_off() + h.payload_bytes) return;
  CHECK(cache_head_bytes(h) == Bytes(whole.begin(), whole.begin() + (ptrdiff_t)h.payload_off()), "%s: the head does not give its bytes back", name.c_str());
  Bytes payload(h.payload_bytes);
  CHECK(pread_all(f.fd, payload.data(), payload.size(), (off_t)h.payload_off()), "%s: payload", name.c_str());
  Checksum64 sum;
  sum.update(payload.data(), payload.size());
  CHECK(sum.finish() == h.checksum, "%s: checksum", name.c_str());
  std::printf("golden %s: format=%s n_items=%llu cell_size=%llu block_size=%llu n_cells=%llu units_per_slot=%llu src=%llu seed=%llu first_item=%llu "
              "mode=%llu base=%zu stamps=%zu payload=%llu\n",
              file.c_str(), h.format == CacheFormat::Tree ? "tree" : "kept", (unsigned long long)h.n_items, (unsigned long long)h.cell_size,
              (unsigned long long)h.block_size, (unsigned long long)h.n_cells, (unsigned long long)h.units_per_slot, (unsigned long long)h.src,
              (unsigned long long)h.seed, (unsigned long long)h.first_item, (unsigned long long)h.mode, h.base.size(), h.stamps.size() / 2,
              (unsigned long long)h.payload_bytes);
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s <scratch dir> [<golden dir>]\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  const size_t refused = check_images_and_refusals(dir);
  const size_t restamps = check_restamp(dir);
  const size_t tmps = check_tmp_file(dir);
  if (argc > 2)
    for (const char* file : {"tree_3slots.cp2", "kept_mode2.cp2", "kept_mode0.cp2"}) check_golden(std::string(argv[2]) + "/" + file, file);
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("cache file check ok: %zu refusals, %zu restamp cases, %zu tmp-file cases\n", refused, restamps, tmps);
  return 0;
}
