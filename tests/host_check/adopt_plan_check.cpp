// The host side of cp2_fill_adopt (csrc/adopt_plan.hpp) walked over random geometries -- 1, 2, 4, 8 and 64 blocks a slot, 1 ... 4 local
// slots, a random selected range -- random known sets (presence, then mark_proved / mark_proved_anchored of random requests), random file
// lengths, random candidate sets and random corruptions.  Compression is a stand-in that is injective by construction: every distinct
// (left, right, key) gets a number of its own, which is all the rule needs.  Asserted on the way:
//   - the blocks to read and the flag bytes sent up, against brute force;
//   - a row is proved exactly when an independent TOP-DOWN restatement says so (a known node that matches vouches for its children; an
//     unknown node hands the voucher on), and a block adopted exactly when its row is proved or known and equal;
//   - no known row is ever written, and after the proved rows are written every known row holds the true node;
//   - a corrupted candidate is never adopted, and neither is any row whose way up to its first known node passes a node it feeds;
//   - adopt_apply sets exactly the proved rows' bits, clears none, and presence follows the adopted blocks;
//   - an all-intact file is adopted whole from the stated root alone;
//   - with one corrupted block and one proved full path to another block, exactly the subtrees under the matching siblings are adopted.
// Built with AddressSanitizer + UBSan.  No GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "adopt_plan.hpp"

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

typedef unsigned long long ull;
typedef uint64_t V;

// the stand-in: 0 is the zero sibling, leaves and junk come from fresh(), every compression of new operands gets a new number
static std::map<std::tuple<V, V, uint32_t>, V> interned;
static V next_value = 1;
static V fresh() { return next_value++; }
static V compress(const V& l, const V& r, uint32_t key) {
  auto it = interned.find(std::make_tuple(l, r, key));
  if (it != interned.end()) return it->second;
  const V v = fresh();
  interned[std::make_tuple(l, r, key)] = v;
  return v;
}

struct World {
  FillPlan plan;
  std::vector<V> truth, kept, roots, cand;
  std::vector<bool> has_cand0, corrupt;                // per global block
  uint64_t s0 = 0, ns = 0;

  void init(uint64_t first, uint64_t n_local, uint64_t nb) {
    plan.init(first, n_local, nb);
    plan.keeps_nodes = true;
    truth.assign(plan.rows, 0);
    for (uint64_t s = 0; s < n_local; ++s) {
      for (uint64_t b = 0; b < nb; ++b) truth[plan.node_row(0, s, b)] = fresh();
      for (size_t l = 0; l < plan.depth(); ++l)
        for (uint64_t j = 0; j < plan.csizes[l + 1]; ++j) {
          const bool pair = 2 * j + 1 < plan.csizes[l];
          truth[plan.node_row(l + 1, s, j)] = compress(truth[plan.node_row(l, s, 2 * j)], pair ? truth[plan.node_row(l, s, 2 * j + 1)] : 0,
                                                       (l == 0 ? 1 : 0) + (pair ? 0 : 2));
        }
    }
    roots.resize(n_local);
    for (uint64_t s = 0; s < n_local; ++s) roots[s] = truth[plan.node_row(plan.depth(), s, 0)];
    has_cand0.assign(plan.total(), false);
    corrupt.assign(plan.total(), false);
  }
  // the session's buffer: the true node where it is known, junk elsewhere
  void fill_kept() {
    kept.resize(plan.rows);
    for (uint64_t r = 0; r < plan.rows; ++r) kept[r] = plan.is_known(r) ? truth[r] : fresh();
  }
};

// ---- the top-down restatement --------------------------------------------------------------------------------------------------------------
struct TopDown {
  const World& w;
  std::vector<uint8_t> defined, computed;              // per row
  std::vector<V> comp;
  std::vector<bool> proved, match;
  explicit TopDown(const World& world) : w(world), defined(world.plan.rows, 0), computed(world.plan.rows, 0), comp(world.plan.rows, 0),
                                          proved(world.plan.rows, false), match(world.plan.rows, false) {}
  // bottom-up by recursion from the top: what a node would compute
  void compute(size_t l, uint64_t s, uint64_t k) {
    const FillPlan& p = w.plan;
    const uint64_t r = p.node_row(l, s, k);
    if (l == 0) {
      const uint64_t g = s * p.n_blocks + k;
      if (w.has_cand0[g]) { computed[r] = 1; comp[r] = w.cand[r]; }
    } else {
      bool all = true;
      V v[2] = {0, 0};
      for (uint64_t c = 0; c < 2; ++c) {
        if (2 * k + c >= p.csizes[l - 1]) continue;
        compute(l - 1, s, 2 * k + c);
        const uint64_t rc = p.node_row(l - 1, s, 2 * k + c);
        all = all && defined[rc];
        v[c] = p.is_known(rc) ? w.kept[rc] : comp[rc];
      }
      if (all) {
        computed[r] = 1;
        comp[r] = compress(v[0], v[1], (l == 1 ? 1 : 0) + (2 * k + 1 < p.csizes[l - 1] ? 0 : 2));
      }
    }
    defined[r] = computed[r] || (l < p.depth() && p.is_known(r));
  }
  void visit(size_t l, uint64_t s, uint64_t k, bool vouched) {
    const FillPlan& p = w.plan;
    const uint64_t r = p.node_row(l, s, k);
    bool down;
    if (l == p.depth()) down = match[r] = computed[r] && comp[r] == w.roots[s];
    else if (p.is_known(r)) down = match[r] = computed[r] && comp[r] == w.kept[r];
    else down = proved[r] = vouched && computed[r];
    if (l == 0) return;
    for (uint64_t c = 0; c < 2; ++c)
      if (2 * k + c < p.csizes[l - 1]) visit(l - 1, s, 2 * k + c, down);
  }
};

static std::mt19937_64 rng(0xAD0B7);
static uint64_t below(uint64_t n) { return n ? rng() % n : 0; }

// one judged call on `w`: flags, model, restatement and every assertion; returns the out bytes
static std::vector<uint8_t> judge(World& w, std::vector<uint64_t>* have, const char* what) {
  FillPlan& p = w.plan;
  const std::vector<uint64_t> known_before = p.known, bits_before = p.bits;
  uint64_t n_cand = 0;
  std::vector<uint8_t> flags = adopt_flags(p, w.s0, w.ns, have, &n_cand);
  // the flag bytes against brute force
  uint64_t want_cand = 0;
  for (size_t l = 0; l <= p.depth(); ++l)
    for (uint64_t s = 0; s < p.n_local; ++s)
      for (uint64_t k = 0; k < p.csizes[l]; ++k) {
        const uint64_t r = p.node_row(l, s, k);
        uint8_t f = (l == p.depth() || p.is_known(r)) ? ADOPT_F_KNOWN : 0;
        if (l == 0 && w.has_cand0[s * p.n_blocks + k] && s >= w.s0 && s < w.s0 + w.ns) { f |= ADOPT_F_CAND; ++want_cand; }
        CHECK(flags[r] == f, "%s: flag byte of row %llu is %u, expected %u", what, (ull)r, flags[r], f);
      }
  CHECK(n_cand == want_cand, "%s: %llu candidates counted, expected %llu", what, (ull)n_cand, (ull)want_cand);
  const std::vector<V> kept_before = w.kept;
  std::vector<V> cand = w.cand;
  adopt_model_layers<V>(p, w.s0, w.ns, w.kept, w.roots, (V)0, &cand, &flags, compress);
  const std::vector<uint8_t> out = adopt_model_resolve<V>(p, w.s0, w.ns, w.kept, cand, flags);
  CHECK(w.kept == kept_before, "%s: the model wrote the kept rows", what);
  // top down
  TopDown td(w);
  for (uint64_t s = w.s0; s < w.s0 + w.ns; ++s) {
    td.compute(p.depth(), s, 0);
    td.visit(p.depth(), s, 0, false);
  }
  for (size_t l = 0; l < p.depth(); ++l)
    for (uint64_t s = 0; s < p.n_local; ++s)
      for (uint64_t k = 0; k < p.csizes[l]; ++k) {
        const uint64_t r = p.node_row(l, s, k);
        const bool sel = s >= w.s0 && s < w.s0 + w.ns;
        const bool proved = (out[r] & ADOPT_F_PROVED) != 0, adopted = (out[r] & ADOPT_F_ADOPTED) != 0;
        if (!sel) { CHECK(out[r] == 0, "%s: row %llu of an unselected slot got %u", what, (ull)r, out[r]); continue; }
        CHECK(proved == td.proved[r], "%s: row %llu (layer %zu) proved %d, the restatement says %d", what, (ull)r, l, proved, (int)td.proved[r]);
        CHECK(!(proved && p.is_known(r)), "%s: known row %llu would be written", what, (ull)r);
        if (proved) CHECK(cand[r] == w.truth[r], "%s: row %llu proved with a value that is not the true node", what, (ull)r);
        if (l == 0) {
          const uint64_t g = s * p.n_blocks + k;
          const bool want = td.proved[r] || (p.is_known(r) && w.has_cand0[g] && w.cand[r] == w.kept[r]);
          CHECK(adopted == want, "%s: block %llu adopted %d, expected %d", what, (ull)g, adopted, want);
          if (w.corrupt[g]) CHECK(!adopted, "%s: corrupted block %llu adopted", what, (ull)g);
          if (adopted) CHECK(w.has_cand0[g] && !p.present(s, k), "%s: block %llu adopted without being an absent candidate", what, (ull)g);
        } else {
          CHECK(!adopted, "%s: row %llu above layer 0 marked adopted", what, (ull)r);
        }
      }
  // what a corrupted candidate feeds: its unknown ancestors, up to and including the first known one; nothing that leans on them is proved
  std::set<uint64_t> fed;
  for (uint64_t g = 0; g < p.total(); ++g) {
    if (!w.corrupt[g] || !w.has_cand0[g]) continue;
    const uint64_t s = g / p.n_blocks;
    if (s < w.s0 || s >= w.s0 + w.ns) continue;
    uint64_t k = g % p.n_blocks;
    if (p.is_known(p.node_row(0, s, k))) continue;     // a known row passes its kept value upward
    fed.insert(p.node_row(0, s, k));
    for (size_t l = 1; l <= p.depth(); ++l) {
      k >>= 1;
      const uint64_t r = p.node_row(l, s, k);
      if (!(flags[r] & ADOPT_F_CAND)) break;
      fed.insert(r);
      if (flags[r] & ADOPT_F_KNOWN) break;
    }
  }
  for (uint64_t r : fed) CHECK(!(flags[r] & ADOPT_F_MATCH) && !(out.size() > r && (out[r] & ADOPT_F_PROVED)), "%s: fed row %llu matched or proved", what, (ull)r);
  for (size_t l = 0; l < p.depth(); ++l)
    for (uint64_t s = w.s0; s < w.s0 + w.ns; ++s)
      for (uint64_t k = 0; k < p.csizes[l]; ++k) {
        const uint64_t r = p.node_row(l, s, k);
        if (p.is_known(r) || !(out[r] & ADOPT_F_PROVED)) continue;
        uint64_t j = k;
        for (size_t up = l + 1; up <= p.depth(); ++up) {
          j >>= 1;
          const uint64_t ra = p.node_row(up, s, j);
          CHECK(!fed.count(ra), "%s: row %llu proved through fed row %llu", what, (ull)r, (ull)ra);
          if (flags[ra] & ADOPT_F_KNOWN) break;
        }
      }
  // applied: exactly the proved rows become known, nothing is cleared, presence only through the commit
  const AdoptVerdict v = adopt_apply(&p, w.s0, w.ns, out);
  uint64_t n_proved = 0;
  for (uint64_t r = 0; r < p.rows; ++r) {
    const bool was = (known_before[r >> 6] >> (r & 63)) & 1, proved = r < out.size() && (out[r] & ADOPT_F_PROVED);
    n_proved += proved;
    CHECK(p.is_known(r) == (was || proved), "%s: known bit of row %llu is %d after the apply", what, (ull)r, (int)p.is_known(r));
    if (proved) w.kept[r] = cand[r];                   // what the kernel's copy does
  }
  CHECK(v.rows_proved == n_proved, "%s: %llu rows proved reported, %llu in the bytes", what, (ull)v.rows_proved, (ull)n_proved);
  CHECK(p.bits == bits_before, "%s: the apply changed presence", what);
  for (uint64_t r = 0; r < p.rows; ++r)
    if (p.is_known(r)) CHECK(w.kept[r] == w.truth[r], "%s: known row %llu does not hold the true node", what, (ull)r);
  CHECK(v.adopted.size() == w.ns, "%s: adopted lists for %zu slots", what, v.adopted.size());
  for (uint64_t i = 0; i < w.ns && i < v.adopted.size(); ++i) {
    std::vector<uint64_t> want;
    for (uint64_t b = 0; b < p.n_blocks; ++b)
      if (out[p.node_row(0, w.s0 + i, b)] & ADOPT_F_ADOPTED) want.push_back((w.s0 + i) * p.n_blocks + b);
    CHECK(v.adopted[i] == want, "%s: the adopted list of slot %llu differs", what, (ull)(w.s0 + i));
    const uint64_t before = p.n_present;
    const size_t set = adopt_commit(&p, v.adopted[i]);
    CHECK(set == want.size() && p.n_present == before + set, "%s: commit set %zu bits of %zu", what, set, want.size());
    for (uint64_t g : want) CHECK(p.present(g / p.n_blocks, g % p.n_blocks), "%s: block %llu not present after the commit", what, (ull)g);
  }
  return out;
}

static const uint64_t SHAPES[] = {1, 2, 4, 8, 64};

static void random_trial() {
  World w;
  const uint64_t nb = SHAPES[below(5)], n_local = 1 + below(4), first = below(5);
  w.init(first, n_local, nb);
  FillPlan& p = w.plan;
  w.s0 = below(n_local);
  w.ns = 1 + below(n_local - w.s0);
  // a known set: presence, what presence gives, then proved requests of both kinds
  std::vector<uint64_t> present;
  const uint64_t density = below(4);
  for (uint64_t g = 0; g < p.total(); ++g)
    if (below(4) < density && below(3)) present.push_back(g);
  p.set_present(present.data(), present.size());
  p.derive_from_presence();
  for (uint64_t i = below(4); i > 0; --i) {
    const uint64_t sb[2] = {first + below(n_local), below(nb)};
    const uint32_t verdict = 0, level = (uint32_t)p.anchor_level(sb[0] - first, sb[1]);
    if (below(2)) p.mark_proved(sb, &verdict, 1);
    else p.mark_proved_anchored(sb, &level, &verdict, 1);
    if (below(2)) { const uint64_t g = (sb[0] - first) * nb + sb[1]; p.set_present(&g, 1); }
  }
  w.fill_kept();
  // the files, and what is read of them
  std::vector<uint64_t> whole(w.ns);
  for (uint64_t i = 0; i < w.ns; ++i) whole[i] = below(3) ? nb : below(nb + 1);
  const std::vector<uint64_t> read_bits = adopt_read_bits(p, w.s0, w.ns, whole);
  for (uint64_t g = 0; g < p.total(); ++g) {
    const uint64_t s = g / nb, b = g % nb;
    const bool want = s >= w.s0 && s < w.s0 + w.ns && !p.present(s, b) && b < whole[s - w.s0 < w.ns ? s - w.s0 : 0];
    CHECK(adopt_bit(read_bits, g) == want, "block %llu read %d, expected %d", (ull)g, (int)adopt_bit(read_bits, g), want);
  }
  for (size_t i = p.total(); i < read_bits.size() * 64; ++i) CHECK(!adopt_bit(read_bits, i), "a bit past the last block is set");
  // remembered: other slots keep what they had, the selected ones hold exactly what was read
  std::vector<uint64_t> have(p.bits.size(), 0);
  for (uint64_t g = 0; g < p.total(); ++g)
    if (below(3) == 0) adopt_set_bit(&have, g, true);
  const std::vector<uint64_t> had = have;
  adopt_remember(p, w.s0, w.ns, read_bits, &have);
  w.cand.assign(p.rows, 0);
  for (uint64_t r = 0; r < p.rows; ++r) w.cand[r] = fresh();
  const uint64_t corruption = below(4);
  for (uint64_t g = 0; g < p.total(); ++g) {
    const uint64_t s = g / nb;
    const bool sel = s >= w.s0 && s < w.s0 + w.ns;
    CHECK(adopt_bit(have, g) == (sel ? adopt_bit(read_bits, g) : adopt_bit(had, g)), "remembered bit of block %llu", (ull)g);
    // what the flags will call a candidate: remembered and absent (a remembered present block of another slot is forgotten)
    w.has_cand0[g] = adopt_bit(have, g) && !p.present(s, g % nb);
    if (!w.has_cand0[g]) continue;
    w.corrupt[g] = corruption && below(8) < corruption;
    w.cand[p.node_row(0, s, g % nb)] = w.corrupt[g] ? fresh() : w.truth[p.node_row(0, s, g % nb)];
  }
  judge(w, &have, "random");
  // a second judgement over what is remembered, after one more proved path: what became present is no candidate any more
  const uint64_t sb[2] = {first + w.s0 + below(w.ns), below(nb)};
  const uint32_t verdict = 0;
  p.mark_proved(sb, &verdict, 1);
  for (size_t l = 0; l <= p.depth(); ++l) {             // the rows that path stored hold the true nodes
    const uint64_t s = sb[0] - first;
    const uint64_t sib = (sb[1] >> l) ^ 1;
    if (l < p.depth() && sib < p.csizes[l]) w.kept[p.node_row(l, s, sib)] = w.truth[p.node_row(l, s, sib)];
    w.kept[p.node_row(l, s, sb[1] >> l)] = w.truth[p.node_row(l, s, sb[1] >> l)];
  }
  for (uint64_t g = 0; g < p.total(); ++g) w.has_cand0[g] = adopt_bit(have, g) && !p.present(g / nb, g % nb);
  judge(w, &have, "no-read");
  uint64_t left = 0;                                     // the next call forgets what the last one adopted
  (void)adopt_flags(p, w.s0, w.ns, &have, &left);
  for (uint64_t g = 0; g < p.total(); ++g)
    if (p.present(g / nb, g % nb)) CHECK(!adopt_bit(have, g), "present block %llu is still remembered", (ull)g);
}

// an intact file under nothing but the stated root; then one corrupted block and one proved path
static void scenarios(uint64_t nb, uint64_t n_local) {
  {
    World w;
    w.init(3, n_local, nb);
    w.s0 = 0; w.ns = n_local;
    w.fill_kept();
    FillPlan& p = w.plan;
    std::vector<uint64_t> have(p.bits.size(), 0);
    adopt_remember(p, 0, n_local, adopt_read_bits(p, 0, n_local, std::vector<uint64_t>(n_local, nb)), &have);
    w.cand.assign(p.rows, 0);
    for (uint64_t g = 0; g < p.total(); ++g) { w.has_cand0[g] = true; w.cand[g] = w.truth[g]; }
    const std::vector<uint8_t> out = judge(w, &have, "intact");
    CHECK(p.n_missing() == 0, "intact: %llu block(s) of %llu still missing", (ull)p.n_missing(), (ull)p.total());
    for (uint64_t r = 0; r < p.coff[p.depth()]; ++r) CHECK(out[r] & ADOPT_F_PROVED, "intact: row %llu not proved", (ull)r);
  }
  if (nb < 2) return;
  for (uint64_t c = 0; c < nb; ++c)
    for (uint64_t q = 0; q < nb; ++q) {
      if (q == c || (nb == 64 && (c * 7 + q) % 13)) continue;
      World w;
      w.init(0, n_local, nb);
      w.s0 = n_local - 1; w.ns = 1;
      FillPlan& p = w.plan;
      const uint64_t s = n_local - 1, sb[2] = {s, q}, gq = s * nb + q;
      const uint32_t verdict = 0;
      p.mark_proved(sb, &verdict, 1);
      p.set_present(&gq, 1);
      w.fill_kept();
      std::vector<uint64_t> have(p.bits.size(), 0);
      adopt_remember(p, s, 1, adopt_read_bits(p, s, 1, std::vector<uint64_t>(1, nb)), &have);
      w.cand.assign(p.rows, 0);
      for (uint64_t b = 0; b < nb; ++b) {
        if (b == q) continue;
        w.has_cand0[s * nb + b] = true;
        w.corrupt[s * nb + b] = b == c;
        w.cand[p.node_row(0, s, b)] = b == c ? fresh() : w.truth[p.node_row(0, s, b)];
      }
      judge(w, &have, "one corrupted");
      // the sibling of level l of q's path covers blocks [(q >> l ^ 1) << l, + 2^l): adopted whole unless c lies in it
      for (uint64_t b = 0; b < nb; ++b) {
        if (b == q) continue;
        size_t l = 0;
        while ((b >> (l + 1)) != (q >> (l + 1))) ++l;
        const bool holds_c = (c >> l) == (b >> l);
        CHECK(p.present(s, b) == !holds_c, "one corrupted (c %llu, path %llu): block %llu present %d", (ull)c, (ull)q, (ull)b, (int)p.present(s, b));
      }
    }
}

int main(int argc, char** argv) {
  const int trials = argc > 1 ? std::atoi(argv[1]) : 500;
  for (int t = 0; t < trials; ++t) random_trial();
  for (uint64_t nb : SHAPES)
    for (uint64_t n_local = 1; n_local <= 4; n_local += 3) scenarios(nb, n_local);
  std::printf("adopt plan ok: %d random trials, scenarios over 5 shapes, %d failures\n", trials, failures);
  return failures ? 1 : 0;
}
