// The host logic of a fill checkpoint with nodes (csrc/node_ckpt_plan.hpp, the header fill.cpp uses) walked over random geometries and
// known sets, every answer compared with a direct restatement kept here: the layout's offsets and size; the round trip (1 block per slot,
// odd layers, bitmaps that are no multiple of 64 bits, rows that are neither present nor known written as zeros or left out whatever
// they held, two serialisations byte-identical); every truncation point and every single flipped byte of a small file refused; known bits
// past the last row, a packed-row count that disagrees with the bitmap and a size the header does not allow refused under a VALID
// checksum; the candidate set and the flag bytes; the model of k_nodes_restore_layer against a recursive restatement; what comes back
// (D within known' within K, equality with unchanged presence, a forged row rejected with its candidate sibling and nothing restored
// below it, every restored value the true one).  Built with AddressSanitizer + UBSan.  No GPU.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "node_ckpt_plan.hpp"

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

static std::mt19937_64 rng(20261018);
static uint64_t pick(uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); }

// an opaque value and a compression that does not collide on what a run meets
typedef uint64_t V;
static V compress(V a, V b, uint32_t key) {
  uint64_t x = a * 0x9e3779b97f4a7c15ULL ^ (b + 0x7f4a7c15ULL) * 0xc2b2ae3d27d4eb4fULL ^ (key + 1) * 0x165667b19e3779f9ULL;
  x ^= x >> 29; x *= 0xbf58476d1ce4e5b9ULL; x ^= x >> 32;
  return x | 1;
}

static FillCkptMeta random_meta(uint64_t n_local, uint64_t n_blocks, bool file) {
  FillCkptMeta m;
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
  return m;
}

// a keeping session as a run of operations leaves it: blocks present before keep_nodes (derived), whole paths, anchored adds
static void random_session(FillPlan* p, uint64_t first, uint64_t n_local, uint64_t n_blocks) {
  p->init(first, n_local, n_blocks);
  std::vector<uint64_t> sb;
  std::vector<uint32_t> st;
  const uint32_t ok = 0;
  for (uint64_t g = 0; g < p->total(); ++g)
    if (pick(0, 3) == 0) { sb = {first + g / n_blocks, g % n_blocks}; st = {FILL_NEW}; p->commit(sb.data(), st.data(), 1); }
  p->derive_from_presence();
  p->keeps_nodes = true;
  const uint64_t adds = pick(0, p->total());
  for (uint64_t i = 0; i < adds; ++i) {
    const uint64_t g = pick(0, p->total() - 1), s = g / n_blocks, b = g % n_blocks;
    sb = {first + s, b};
    if (pick(0, 2) == 0) {
      const uint32_t level = (uint32_t)p->anchor_level(s, b);
      p->mark_proved_anchored(sb.data(), &level, &ok, 1);
    } else p->mark_proved(sb.data(), &ok, 1);
    if (pick(0, 4)) { st = {FILL_NEW}; p->commit(sb.data(), st.data(), 1); }   // (an UNWRITTEN block stays absent, its nodes known)
  }
}

static void put_sum(std::vector<uint8_t>* buf) {
  Checksum64 sum;
  sum.update(buf->data(), buf->size() - 8);
  fill_ckpt_put(buf->data() + buf->size() - 8, sum.finish());
}

// the restatement of the restore: the state of row r, recursively from its parent's
struct Direct {
  const FillPlan& p;
  const std::vector<V>&tree, &cand, &roots;
  const std::vector<uint8_t>& up;
  std::map<uint64_t, uint8_t> memo;
  uint8_t state(size_t l, uint64_t s, uint64_t k) {
    const uint64_t r = p.node_row(l, s, k);
    if (up[r] != NODE_F_CAND) return up[r];
    auto it = memo.find(r);
    if (it != memo.end()) return it->second;
    uint8_t out = NODE_F_CAND;
    const uint8_t fp = state(l + 1, s, k >> 1);
    const uint64_t sib = k ^ 1;
    const bool pair = sib < p.csizes[l];
    const uint8_t fs = pair ? up[p.node_row(l, s, sib)] : NODE_F_KNOWN;
    if ((fp & (NODE_F_KNOWN | NODE_F_RESTORED)) && (fs & (NODE_F_KNOWN | NODE_F_CAND))) {
      const V me = cand[r], other = !pair ? 0 : fs == NODE_F_KNOWN ? tree[p.node_row(l, s, sib)] : cand[p.node_row(l, s, sib)];
      const V v = compress((k & 1) ? other : me, (k & 1) ? me : other, (uint32_t)((l == 0 ? 1 : 0) + (pair ? 0 : 2)));
      const uint64_t rp = p.node_row(l + 1, s, k >> 1);
      const V want = l + 1 == p.depth() ? roots[s] : (up[rp] == NODE_F_KNOWN ? tree[rp] : cand[rp]);   // a restored parent holds its candidate
      out = v == want ? NODE_F_RESTORED : NODE_F_REJECTED;
    }
    memo[r] = out;
    return out;
  }
};

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 500;
  std::string err;
  uint64_t n_restored = 0, n_rejected = 0, n_unproved = 0, n_files = 0, n_refused = 0;

  for (int round = 0; round < rounds; ++round) {
    const uint64_t n_blocks = round % 7 == 0 ? 1 : (round % 5 == 0 ? pick(1, 70) : (uint64_t)1 << pick(0, 6));
    const uint64_t n_local = round % 11 == 0 ? 1 : pick(1, 5);
    const FillCkptMeta m = random_meta(n_local, n_blocks, round & 1);
    FillPlan p;
    random_session(&p, m.first_slot, n_local, n_blocks);
    const uint64_t total = p.total(), top = p.coff[p.depth()];

    // ---- the layout ----------------------------------------------------------------------------------------------------------------------
    NodeCkptLayout l;
    CHECK(node_ckpt_layout(m.file_base.size(), n_local, n_blocks, &l), "round %d: layout refused", round);
    CHECK(l.rows == p.rows && l.mid_begin == total && l.mid_end == top && l.known_words == p.known.size(), "round %d: layout rows", round);
    const size_t head = 88 + (m.file_base.size() + 7) / 8 * 8 + n_local * 32 + (total + 63) / 64 * 8;
    CHECK(l.known_at == head && l.layer0_at == head + (p.rows + 63) / 64 * 8 && l.mid_at == l.layer0_at + total * 32, "round %d: layout offsets", round);

    // ---- the round trip --------------------------------------------------------------------------------------------------------------------
    std::vector<uint8_t> image(p.rows * 32), buf, again;
    for (auto& b : image) b = (uint8_t)(rng() | 1);             // never zero: an unknown row must come back as zeros or not at all
    CHECK(node_ckpt_serialise(m, p, image.data(), &buf) && node_ckpt_serialise(m, p, image.data(), &again) && buf == again,
          "round %d: serialise fails or is not deterministic", round);
    const uint64_t n_mid = node_ckpt_count(p.known, total, top);
    CHECK(buf.size() == l.mid_at + n_mid * 32 + 8, "round %d: size", round);
    ++n_files;
    {
      std::vector<uint8_t> other(image);                         // what is not known does not reach the file
      for (uint64_t r = 0; r < p.rows; ++r)
        if (!p.is_known(r) && !(r < total && node_ckpt_bit(p.bits, r)))
          for (int i = 0; i < 32; ++i) other[r * 32 + i] ^= 0x5a;
      CHECK(node_ckpt_serialise(m, p, other.data(), &again) && buf == again, "round %d: an unknown row reached the file", round);
    }
    NodeCheckpoint c;
    CHECK(node_ckpt_parse(buf.data(), buf.size(), &c, &err), "round %d: parse: %s", round, err.c_str());
    CHECK(c.known == p.known && c.base.bits == p.bits && c.base.meta.roots == m.roots && c.base.meta.file_base == m.file_base &&
              c.base.meta.seed == m.seed && c.base.meta.n_local == n_local && c.base.meta.n_blocks() == n_blocks,
          "round %d: fields", round);
    CHECK(c.base.layer0.size() == total * 32 && c.mid.size() == n_mid * 32, "round %d: sizes of the parts", round);
    size_t at = 0;
    for (uint64_t r = 0; r < top && c.base.layer0.size() == total * 32 && c.mid.size() == n_mid * 32; ++r) {
      if (r < total) {
        const bool kept = p.is_known(r) || node_ckpt_bit(p.bits, r);
        bool same = true, zero = true;
        for (int i = 0; i < 32; ++i) { same &= c.base.layer0[r * 32 + i] == image[r * 32 + i]; zero &= c.base.layer0[r * 32 + i] == 0; }
        CHECK(kept ? same : zero, "round %d: layer-0 row %llu", round, (unsigned long long)r);
      } else if (p.is_known(r)) {
        CHECK(std::memcmp(&c.mid[at], &image[r * 32], 32) == 0, "round %d: packed row %llu", round, (unsigned long long)r);
        at += 32;
      }
    }
    // the same header under the other magic is each format's to refuse
    {
      FillCheckpoint c1;
      CHECK(!fill_ckpt_parse(buf.data(), buf.size(), &c1, &err) && err.find("magic") != std::string::npos, "round %d: CP2FILL1's parser took a CP2FILL2 file", round);
    }

    // ---- corrupt files -----------------------------------------------------------------------------------------------------------------------
    if (buf.size() < 1500) {
      for (size_t n = 0; n < buf.size(); ++n) { CHECK(!node_ckpt_parse(buf.data(), n, &c, &err), "round %d: truncation at %zu accepted", round, n); ++n_refused; }
      for (size_t i = 0; i < buf.size(); ++i) {
        std::vector<uint8_t> bad(buf);
        bad[i] ^= (uint8_t)(1u << pick(0, 7));
        CHECK(!node_ckpt_parse(bad.data(), bad.size(), &c, &err), "round %d: flipped byte %zu accepted", round, i);
        ++n_refused;
      }
    }
    if (p.rows & 63) {                                           // a known bit past the last row, checksum valid
      std::vector<uint8_t> bad(buf);
      const uint64_t bit = p.rows + pick(0, 63 - (p.rows & 63));
      bad[l.known_at + (bit >> 3)] |= (uint8_t)(1u << (bit & 7));
      put_sum(&bad);
      CHECK(!node_ckpt_parse(bad.data(), bad.size(), &c, &err) && err.find("known bits past the last row") != std::string::npos, "round %d: bit past the rows: %s", round, err.c_str());
    }
    if (top > total) {                                           // the packed count against the bitmap, checksum valid
      std::vector<uint8_t> bad(buf);
      const uint64_t r = pick(total, top - 1);
      bad[l.known_at + (r >> 3)] ^= (uint8_t)(1u << (r & 7));
      put_sum(&bad);
      CHECK(!node_ckpt_parse(bad.data(), bad.size(), &c, &err) && err.find("packed row") != std::string::npos, "round %d: packed count: %s", round, err.c_str());
      std::vector<uint8_t> longer(buf);
      longer.insert(longer.end() - 8, 32, (uint8_t)7);
      put_sum(&longer);
      CHECK(!node_ckpt_parse(longer.data(), longer.size(), &c, &err), "round %d: one packed row too many accepted", round);
    }
    {
      std::vector<uint8_t> odd(buf);                             // a size the header does not allow, checksum valid
      odd.insert(odd.end() - 8, 8, (uint8_t)0);
      put_sum(&odd);
      CHECK(!node_ckpt_parse(odd.data(), odd.size(), &c, &err) && err.find("no size its header allows") != std::string::npos, "round %d: odd size: %s", round, err.c_str());
    }
    CHECK(node_ckpt_parse(buf.data(), buf.size(), &c, &err), "round %d: parse again: %s", round, err.c_str());

    // ---- the restore -----------------------------------------------------------------------------------------------------------------------
    // the truth: a tree per slot; the saved rows hold it, one of them forged in every third round
    std::vector<V> truth(p.rows), roots(n_local);
    for (uint64_t g = 0; g < total; ++g) truth[g] = rng() | 1;
    for (size_t lv = 0; lv < p.depth(); ++lv)
      for (uint64_t s = 0; s < n_local; ++s)
        for (uint64_t j = 0; j < p.csizes[lv + 1]; ++j) {
          const bool pair = 2 * j + 1 < p.csizes[lv];
          truth[p.node_row(lv + 1, s, j)] = compress(truth[p.node_row(lv, s, 2 * j)], pair ? truth[p.node_row(lv, s, 2 * j + 1)] : 0,
                                                     (uint32_t)((lv == 0 ? 1 : 0) + (pair ? 0 : 2)));
        }
    for (uint64_t s = 0; s < n_local; ++s) roots[s] = truth[p.node_row(p.depth(), s, 0)];
    // the resumed session: some present blocks dropped in every second round, then D
    FillPlan q;
    q.init(m.first_slot, n_local, n_blocks);
    q.restore(p.bits);
    std::vector<uint64_t> drop;
    if (round % 2)
      for (uint64_t g = 0; g < total; ++g)
        if (node_ckpt_bit(p.bits, g) && pick(0, 5) == 0) drop.push_back(g);
    q.drop(drop.data(), drop.size());
    q.derive_from_presence();
    q.keeps_nodes = true;
    const std::vector<uint64_t> d_bits = q.known;
    // the values as 32-byte rows of the file's parts (the value in the first 8 bytes)
    std::vector<uint8_t> layer0(total * 32, 0), mid;
    std::vector<uint64_t> saved_rows;
    for (uint64_t r = 0; r < top; ++r)
      if (p.is_known(r)) saved_rows.push_back(r);
    uint64_t forged = UINT64_MAX;
    if (round % 3 == 0 && !saved_rows.empty()) forged = saved_rows[pick(0, saved_rows.size() - 1)];
    for (uint64_t r = 0; r < top; ++r) {
      const V v = r == forged ? truth[r] ^ 0x10 : truth[r];
      if (r < total) { if (p.is_known(r) || node_ckpt_bit(p.bits, r)) std::memcpy(&layer0[r * 32], &v, 8); }
      else if (p.is_known(r)) { mid.resize(mid.size() + 32, 0); std::memcpy(&mid[mid.size() - 32], &v, 8); }
    }
    NodeRestorePlan rp;
    CHECK(node_restore_plan(q, p.known, layer0, mid, &rp), "round %d: restore plan refused", round);
    {
      NodeRestorePlan none;
      CHECK(!node_restore_plan(q, p.known, layer0, std::vector<uint8_t>(mid.size() + 32), &none), "round %d: a packed row too many accepted", round);
    }
    uint64_t want_cand = 0;
    std::vector<V> tree(p.rows, 0xdead), cand(p.rows, 0);
    for (uint64_t r = 0; r < p.rows; ++r) {
      const uint8_t want = r >= top ? NODE_F_KNOWN : q.is_known(r) ? NODE_F_KNOWN : p.is_known(r) ? NODE_F_CAND : 0;
      CHECK(rp.flags[r] == want, "round %d: flag byte of row %llu is %d, expected %d", round, (unsigned long long)r, rp.flags[r], want);
      want_cand += want == NODE_F_CAND;
      std::memcpy(&cand[r], &rp.cand[r * 32], 8);
      if (want == NODE_F_CAND) CHECK(cand[r] == (r == forged ? truth[r] ^ 0x10 : truth[r]), "round %d: candidate value of row %llu", round, (unsigned long long)r);
      else CHECK(cand[r] == 0, "round %d: row %llu is no candidate and has a value", round, (unsigned long long)r);
      if (r < top && q.is_known(r)) tree[r] = truth[r];          // D holds what the device rebuilt from the re-checked blocks: the truth
    }
    CHECK(rp.n_cand == want_cand, "round %d: n_cand", round);
    const std::vector<V> tree0 = tree;
    std::vector<uint8_t> down = rp.flags;
    node_restore_model(q, &tree, cand, roots, (V)0, &down, compress);
    Direct direct{q, tree0, cand, roots, rp.flags, {}};
    for (size_t lv = 0; lv < p.depth(); ++lv)
      for (uint64_t s = 0; s < n_local; ++s)
        for (uint64_t k = 0; k < p.csizes[lv]; ++k) {
          const uint64_t r = p.node_row(lv, s, k);
          const uint8_t want = direct.state(lv, s, k);
          CHECK(down[r] == want, "round %d: row %llu comes back as %d, the restatement says %d", round, (unsigned long long)r, down[r], want);
          if (down[r] == NODE_F_RESTORED) CHECK(tree[r] == cand[r] && tree[r] == truth[r], "round %d: restored row %llu is not the true node", round, (unsigned long long)r);
          else CHECK(tree[r] == tree0[r], "round %d: row %llu was written", round, (unsigned long long)r);
        }
    for (uint64_t r = top; r < p.rows; ++r) CHECK(down[r] == NODE_F_KNOWN && tree[r] == tree0[r], "round %d: top row %llu touched", round, (unsigned long long)r);
    const NodeRestoreCounts counts = node_restore_apply(&q, p.known, rp.flags, down);
    CHECK(counts.restored + counts.rejected + counts.unproved == rp.n_cand, "round %d: the counts do not add up", round);
    n_restored += counts.restored; n_rejected += counts.rejected; n_unproved += counts.unproved;
    uint64_t newly = 0;
    for (uint64_t r = 0; r < p.rows; ++r) {
      CHECK(!node_ckpt_bit(d_bits, r) || q.is_known(r), "round %d: row %llu of D is lost", round, (unsigned long long)r);
      CHECK(!q.is_known(r) || p.is_known(r) || node_ckpt_bit(d_bits, r), "round %d: row %llu is known and was neither saved nor derived", round, (unsigned long long)r);
      if (r < top) newly += q.is_known(r) && !node_ckpt_bit(d_bits, r);
      else CHECK(q.is_known(r) == (p.is_known(r) || node_ckpt_bit(d_bits, r)), "round %d: top row %llu's bit", round, (unsigned long long)r);
      if (r < top && q.is_known(r)) CHECK(tree[r] == truth[r], "round %d: known row %llu does not hold the true node", round, (unsigned long long)r);
    }
    CHECK(newly == counts.restored, "round %d: %llu rows became known, %llu restored", round, (unsigned long long)newly, (unsigned long long)counts.restored);
    if (drop.empty() && forged == UINT64_MAX) {
      // (a top row may be derived where the session never stored it -- an anchored add's walk ends below it: that bit is checked above)
      bool same = true;
      for (uint64_t r = 0; r < top; ++r) same &= q.is_known(r) == p.is_known(r);
      CHECK(same && counts.rejected == 0 && counts.unproved == 0, "round %d: unchanged files, and the known set differs (%llu rejected, %llu unproved)",
            round, (unsigned long long)counts.rejected, (unsigned long long)counts.unproved);
    }
    if (forged != UINT64_MAX && rp.flags[forged] == NODE_F_CAND) {
      CHECK(down[forged] != NODE_F_RESTORED && !q.is_known(forged), "round %d: the forged row %llu was restored", round, (unsigned long long)forged);
    }
    // a byte that claims what the bytes sent up rule out is ignored
    {
      FillPlan q2;
      q2.init(m.first_slot, n_local, n_blocks);
      q2.known = d_bits;
      std::vector<uint8_t> lies(p.rows, NODE_F_RESTORED);
      const NodeRestoreCounts c2 = node_restore_apply(&q2, p.known, rp.flags, lies);
      CHECK(c2.restored == rp.n_cand, "round %d: lies: restored", round);
      for (uint64_t r = 0; r < top; ++r) CHECK(q2.is_known(r) == (node_ckpt_bit(d_bits, r) || rp.flags[r] == NODE_F_CAND), "round %d: lies: row %llu", round, (unsigned long long)r);
    }
  }

  // ---- headers no session has: bounded before anything is sized --------------------------------------------------------------------------
  {
    NodeCkptLayout l;
    CHECK(!node_ckpt_layout(0, 0, 8, &l) && !node_ckpt_layout(0, 8, 0, &l) && !node_ckpt_layout(5000, 1, 1, &l), "layout bounds");
    CHECK(!node_ckpt_layout(0, 1ULL << 30, 1ULL << 30, &l) && !node_ckpt_layout(0, UINT64_MAX, 2, &l), "layout products");
    CHECK(node_ckpt_layout(0, 1, 1ULL << 40, &l) && l.rows > l.base.total && l.rows < 2 * l.base.total + 64, "layout at the bound");
    std::vector<uint8_t> head(FILL_CKPT_FIXED + 8, 0);
    FillCkptMeta m;
    CHECK(!node_ckpt_fixed(head.data(), head.size(), &m, &l, &err), "an all-zero header accepted");
    std::memcpy(head.data(), "CP2FILL2", 8);
    CHECK(!node_ckpt_fixed(head.data(), head.size(), &m, &l, &err), "a header of zeros accepted");
    const uint64_t w[10] = {64, 256, 1ULL << 62, 1, 0, 1, 0, 0, 0, 1ULL << 60};
    for (int i = 0; i < 10; ++i) fill_ckpt_put(head.data() + 8 + 8 * i, w[i]);
    CHECK(!node_ckpt_fixed(head.data(), head.size(), &m, &l, &err), "a header of 2^60 blocks accepted");
  }

  std::printf("node checkpoint ok: %d sessions, %llu files, %llu corruptions refused, %llu rows restored, %llu rejected, %llu unproved, %d failures\n", rounds,
              (unsigned long long)n_files, (unsigned long long)n_refused, (unsigned long long)n_restored, (unsigned long long)n_rejected,
              (unsigned long long)n_unproved, failures);
  return failures ? 1 : 0;
}
