// The host side of anchored fill adds (csrc/fill_plan.hpp: anchor_level, validate_anchored, device_requests_anchored,
// mark_proved_anchored) walked over random geometries -- 1 ... 64 blocks a slot, odd layer sizes included, 1 ... 3 local slots -- and random
// interleavings of full adds, anchored adds, derive_from_presence and drop.  Every answer is compared with a restatement kept here: a set
// of (slot, layer, index) triples and a brute-force layout.  The invariants the design rests on are asserted on the way: anchor_level
// never rises for a block as requests are proved; a proved anchored request never clears a bit and never sets the bit of its anchor or of
// a row above it; after a proved request at level a the block's anchor is 0 and, for every level l < a, the blocks under its sibling of
// level l are anchored at l or lower; and a whole slot of 2^k blocks filled at lowest anchors, one request a call in a shuffled order,
// takes exactly nBlocks - 1 siblings (k >= 1; the one-block slot takes the one zero its single round pairs it with).  Built with
// AddressSanitizer + UBSan.  No GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "block_proof_plan.hpp"
#include "fill_plan.hpp"

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

// layer sizes of a tree over n leaves, bottom first; the bottom layer always gets one round
static std::vector<uint64_t> layers(uint64_t n) {
  std::vector<uint64_t> s;
  uint64_t m = n;
  bool bottom = true;
  for (;;) {
    s.push_back(m);
    if (m == 1 && !bottom) break;
    m = (m + 1) / 2;
    bottom = false;
  }
  return s;
}

typedef std::tuple<uint64_t, size_t, uint64_t> Node;   // (local slot, layer, index)

struct Model {
  uint64_t n_local, n_blocks;
  std::vector<uint64_t> sizes;
  std::set<std::pair<uint64_t, uint64_t>> present;     // (local, block)
  std::set<Node> known;
  bool keeping = false;
  size_t depth() const { return sizes.size() - 1; }
  uint64_t row(uint64_t local, size_t level, uint64_t index) const {
    uint64_t r = 0;
    for (size_t l = 0; l < level; ++l) r += n_local * sizes[l];
    return r + local * sizes[level] + index;
  }
  size_t anchor(uint64_t local, uint64_t b) const {
    if (!keeping) return depth();
    uint64_t j = b;
    for (size_t l = 0; l < depth(); ++l, j /= 2)
      if (known.count(Node(local, l, j))) return l;
    return depth();
  }
  bool anchor_known(uint64_t local, uint64_t b, size_t a) const {
    if (a == depth()) return true;
    uint64_t j = b;
    for (size_t l = 0; l < a; ++l) j /= 2;
    return known.count(Node(local, a, j)) != 0;
  }
  void prove(uint64_t local, uint64_t b) {             // a whole path
    known.insert(Node(local, 0, b));
    uint64_t j = b;
    for (size_t l = 0; l < depth(); ++l) {
      if ((j ^ 1) < sizes[l]) known.insert(Node(local, l, j ^ 1));
      j /= 2;
      known.insert(Node(local, l + 1, j));
    }
  }
  void prove_anchored(uint64_t local, uint64_t b, size_t a) {
    if (a == 0) return;
    known.insert(Node(local, 0, b));
    uint64_t j = b;
    for (size_t l = 0; l < a; ++l) {
      if ((j ^ 1) < sizes[l]) known.insert(Node(local, l, j ^ 1));
      j /= 2;
      if (l + 1 < a) known.insert(Node(local, l + 1, j));
    }
  }
  void derive() {
    known.clear();
    for (const auto& p : present) known.insert(Node(p.first, 0, p.second));
    for (size_t l = 0; l < depth(); ++l)
      for (uint64_t s = 0; s < n_local; ++s)
        for (uint64_t k = 0; k < sizes[l + 1]; ++k) {
          bool all = known.count(Node(s, l, 2 * k)) != 0;
          if (2 * k + 1 < sizes[l]) all = all && known.count(Node(s, l, 2 * k + 1)) != 0;
          if (all) known.insert(Node(s, l + 1, k));
        }
  }
};

static void compare(const FillPlan& p, const Model& m, int round) {
  for (uint64_t s = 0; s < m.n_local; ++s) {
    for (size_t l = 0; l <= m.depth(); ++l)
      for (uint64_t k = 0; k < m.sizes[l]; ++k)
        CHECK(p.is_known(p.node_row(l, s, k)) == (m.known.count(Node(s, l, k)) != 0), "known(%zu, %llu, %llu) differs, round %d", l, (ull)s, (ull)k, round);
    for (uint64_t b = 0; b < m.n_blocks; ++b) {
      CHECK(p.anchor_level(s, b) == m.anchor(s, b), "anchor_level(%llu, %llu) = %zu, brute force %zu, round %d", (ull)s, (ull)b, p.anchor_level(s, b),
            m.anchor(s, b), round);
      CHECK(p.present(s, b) == (m.present.count({s, b}) != 0), "presence differs");
    }
  }
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 1000;
  std::mt19937_64 rng(20261019);
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  uint64_t steps = 0, anchored = 0, zero_level = 0, refused = 0, same_call = 0, odd_geoms = 0, whole_slots = 0, pow2_slots = 0;

  for (int round = 0; round < rounds; ++round) {
    const uint64_t n_blocks = round % 9 == 0 ? 1 : round % 9 == 1 ? (1ULL << pick(0, 6)) : pick(1, 64), n_local = pick(1, 3), first_slot = pick(0, 9);
    odd_geoms += n_blocks & 1;
    FillPlan p;
    p.init(first_slot, n_local, n_blocks);
    Model m{n_local, n_blocks, layers(n_blocks), {}, {}};
    const size_t depth = m.depth();
    CHECK(p.depth() == depth, "depth %zu for %llu blocks", p.depth(), (ull)n_blocks);

    // ---- a session that keeps no nodes answers depth throughout and takes no anchored request -------------------------------------------
    {
      std::string err;
      const uint64_t sb[2] = {first_slot, 0};
      const uint32_t lv[1] = {(uint32_t)depth};
      for (uint64_t s = 0; s < n_local; ++s)
        for (uint64_t b = 0; b < n_blocks; ++b) CHECK(p.anchor_level(s, b) == depth, "a plain session anchors (%llu, %llu) at %zu", (ull)s, (ull)b, p.anchor_level(s, b));
      CHECK(!p.validate_anchored(sb, lv, 1, &err) && err.find("cp2_fill_keep_nodes") != std::string::npos, "a plain session takes an anchored request");
      CHECK(p.validate(sb, 1, &err), "validate refuses a good request: %s", err.c_str());
    }
    // some blocks arrive before keeping is turned on
    const size_t early = (size_t)pick(0, n_local * n_blocks / 2);
    for (size_t k = 0; k < early; ++k) {
      const uint64_t s = pick(0, n_local - 1), b = pick(0, n_blocks - 1);
      const uint64_t sb[2] = {first_slot + s, b};
      const uint32_t st[1] = {FILL_NEW};
      p.commit(sb, st, 1);
      m.present.insert({s, b});
    }
    p.derive_from_presence();
    p.keeps_nodes = true;
    m.derive();
    m.keeping = true;
    compare(p, m, round);

    // ---- random interleaving ---------------------------------------------------------------------------------------------------------
    const int ops = (int)pick(5, 40);
    for (int op = 0; op < ops; ++op) {
      ++steps;
      const uint64_t kind = pick(0, 9);
      std::vector<size_t> before(n_local * n_blocks);
      for (uint64_t s = 0; s < n_local; ++s)
        for (uint64_t b = 0; b < n_blocks; ++b) before[s * n_blocks + b] = p.anchor_level(s, b);
      const std::vector<uint64_t> known_before = p.known;
      bool proving = true;
      if (kind == 0) {                                 // the blocks the disk no longer backs, then what presence still gives
        std::vector<uint64_t> gone;
        for (int k = 0; k < 3; ++k) gone.push_back(pick(0, n_local * n_blocks));       // (one past the end is ignored)
        p.drop(gone.data(), gone.size());
        for (uint64_t g : gone)
          if (g < n_local * n_blocks) m.present.erase({g / n_blocks, g % n_blocks});
        p.derive_from_presence();
        m.derive();
        proving = false;
      } else if (kind <= 2) {                          // whole paths, some not proved
        const size_t n = (size_t)pick(1, 4);
        std::vector<uint64_t> sb;
        std::vector<uint32_t> verdict, status(n);
        for (size_t i = 0; i < n; ++i) {
          const uint64_t s = pick(0, n_local - 1), b = pick(0, n_blocks - 1);
          sb.push_back(first_slot + s); sb.push_back(b);
          verdict.push_back(pick(0, 3) == 0 ? 1 : 0);
          if (verdict.back() == 0) { m.prove(s, b); m.present.insert({s, b}); }
        }
        p.mark_proved(sb.data(), verdict.data(), n);
        p.resolve(sb.data(), verdict.data(), n, status.data());
        p.commit(sb.data(), status.data(), n);
      } else if (kind <= 4) {                          // one anchored request a call: the invariants of a single proved request
        const uint64_t s = pick(0, n_local - 1), b = pick(0, n_blocks - 1);
        std::vector<size_t> ok;
        for (size_t a = 0; a <= depth; ++a)
          if (m.anchor_known(s, b, a)) ok.push_back(a);
        const size_t a = pick(0, 1) ? ok.front() : ok[(size_t)pick(0, ok.size() - 1)];   // the lowest, or any known level
        CHECK(ok.front() == p.anchor_level(s, b), "the lowest known level");
        const uint64_t sb[2] = {first_slot + s, b};
        const uint32_t lv[1] = {(uint32_t)a}, verdict[1] = {pick(0, 4) == 0 ? 1u : 0u};
        std::string err;
        CHECK(p.validate_anchored(sb, lv, 1, &err), "a known level is refused: %s", err.c_str());
        p.mark_proved_anchored(sb, lv, verdict, 1);
        uint32_t status[1];
        p.resolve(sb, verdict, 1, status);
        const bool unwritten = verdict[0] == 0 && pick(0, 5) == 0;   // proved, not written: missing, its nodes known
        if (unwritten) status[0] = FILL_UNWRITTEN;
        p.commit(sb, status, 1);
        if (verdict[0] == 0) {
          ++anchored;
          zero_level += a == 0;
          m.prove_anchored(s, b, a);
          if (!unwritten) m.present.insert({s, b});
          for (size_t w = 0; w < p.known.size(); ++w) CHECK((known_before[w] & ~p.known[w]) == 0, "a proved anchored request cleared a bit");
          for (size_t l = a; l <= depth; ++l) {
            const uint64_t r = p.node_row(l, s, b >> l);
            CHECK(p.is_known(r) == (bool)((known_before[(size_t)(r >> 6)] >> (r & 63)) & 1), "the bit of level %zu changed under an anchor at %zu", l, a);
          }
          CHECK(p.anchor_level(s, b) == 0, "after a proved request at level %zu the block is anchored at %zu", a, p.anchor_level(s, b));
          for (size_t l = 0; l < a; ++l) {
            const uint64_t sib = (b >> l) ^ 1;
            if (sib >= m.sizes[l]) continue;
            for (uint64_t nb = sib << l; nb < std::min(n_blocks, (sib + 1) << l); ++nb)
              CHECK(p.anchor_level(s, nb) <= l, "block %llu under the level-%zu sibling of %llu is anchored at %zu", (ull)nb, l, (ull)b, p.anchor_level(s, nb));
          }
        } else {
          CHECK(p.known == known_before, "a request that did not prove changed the known rows");
        }
      } else if (kind <= 7) {                          // a call of several anchored requests, judged against the state at its start
        const size_t n = (size_t)pick(1, 6);
        std::vector<uint64_t> sb;
        std::vector<uint32_t> lv, verdict, status(n);
        for (size_t i = 0; i < n; ++i) {
          const uint64_t s = pick(0, n_local - 1), b = pick(0, n_blocks - 1);
          std::vector<size_t> ok;
          for (size_t a = 0; a <= depth; ++a)
            if (m.anchor_known(s, b, a)) ok.push_back(a);
          sb.push_back(first_slot + s); sb.push_back(b);
          lv.push_back((uint32_t)ok[(size_t)pick(0, ok.size() - 1)]);
          verdict.push_back(pick(0, 4) == 0 ? 1 : 0);
        }
        std::string err;
        CHECK(p.validate_anchored(sb.data(), lv.data(), n, &err), "known levels are refused: %s", err.c_str());
        std::vector<uint64_t> lb, dest, lb0, dest0, off, arow;
        p.device_requests_anchored(sb.data(), lv.data(), n, &lb, &dest, &off, &arow);
        p.device_requests(sb.data(), n, &lb0, &dest0);
        CHECK(lb == lb0 && dest == dest0 && off.size() == n + 1 && arow.size() == n, "the tables of an anchored call");
        uint64_t sum = 0;
        for (size_t i = 0; i < n && off.size() == n + 1 && arow.size() == n; ++i) {
          CHECK(off[i] == sum, "path_off[%zu] = %llu, prefix sum %llu", i, (ull)off[i], (ull)sum);
          sum += lv[i];
          uint64_t j = sb[2 * i + 1];
          for (uint32_t l = 0; l < lv[i]; ++l) j /= 2;
          const uint64_t want = lv[i] == depth ? UINT64_MAX : m.row(sb[2 * i] - first_slot, lv[i], j);
          CHECK(arow[i] == want && (want == UINT64_MAX || want < p.rows), "anchor_row[%zu] = %llu, brute force %llu", i, (ull)arow[i], (ull)want);
        }
        CHECK(off.back() == sum, "the last entry of path_off is the sum of the levels");
        p.mark_proved_anchored(sb.data(), lv.data(), verdict.data(), n);
        p.resolve(sb.data(), verdict.data(), n, status.data());
        p.commit(sb.data(), status.data(), n);
        for (size_t i = 0; i < n; ++i)
          if (verdict[i] == 0) {
            m.prove_anchored(sb[2 * i] - first_slot, sb[2 * i + 1], lv[i]);
            m.present.insert({sb[2 * i] - first_slot, sb[2 * i + 1]});
            ++anchored;
          }
        for (size_t w = 0; w < p.known.size(); ++w) CHECK((known_before[w] & ~p.known[w]) == 0, "a proved anchored call cleared a bit");
      } else {                                         // calls that must be refused, naming the lowest offending index
        const size_t n = (size_t)pick(2, 6), bad = (size_t)pick(0, n - 1);
        std::vector<uint64_t> sb;
        std::vector<uint32_t> lv;
        std::string want_word;
        for (size_t i = 0; i < n; ++i) {
          const uint64_t s = pick(0, n_local - 1), b = pick(0, n_blocks - 1);
          sb.push_back(first_slot + s); sb.push_back(b);
          lv.push_back((uint32_t)p.anchor_level(s, b));
        }
        const uint64_t how = pick(0, 4);
        const uint64_t s = sb[2 * bad] - first_slot, b = sb[2 * bad + 1];
        if (how == 0) { sb[2 * bad] = first_slot + n_local; want_word = "slot"; }
        else if (how == 1) { sb[2 * bad + 1] = n_blocks; want_word = "block"; }
        else if (how == 2) { lv[bad] = (uint32_t)depth + 1 + (uint32_t)pick(0, 1) * 1000000u; want_word = "level"; }
        else if (how == 3 && first_slot > 0) { sb[2 * bad] = first_slot - 1; want_word = "slot"; }
        else {
          // a level below the lowest known one: its node is not known now, even where an earlier request of this very call would prove it
          const size_t lowest = p.anchor_level(s, b);
          if (lowest == 0) { lv[bad] = (uint32_t)depth + 1; want_word = "level"; }
          else {
            lv[bad] = (uint32_t)pick(0, lowest - 1);
            want_word = "not known";
            if (bad > 0 && n_blocks > 1) {             // request bad - 1: the neighbour's whole path, which would prove the node asked for
              const uint64_t nb = (b ^ 1) < n_blocks ? (b ^ 1) : b;
              sb[2 * (bad - 1)] = first_slot + s; sb[2 * (bad - 1) + 1] = nb;
              lv[bad - 1] = (uint32_t)p.anchor_level(s, nb);
              same_call += nb != b && lv[bad] == 0 && lv[bad - 1] > 0;
            }
          }
        }
        std::string err;
        const bool took = p.validate_anchored(sb.data(), lv.data(), n, &err);
        CHECK(!took, "a bad call was accepted (how %llu, round %d)", (ull)how, round);
        CHECK(err.find("request " + std::to_string(bad) + ":") != std::string::npos && err.find(want_word) != std::string::npos,
              "the refusal of request %zu (%s) reads: %s", bad, want_word.c_str(), err.c_str());
        CHECK(p.known == known_before, "a refused call changed the session");
        ++refused;
        proving = false;
      }
      compare(p, m, round);
      if (proving)
        for (uint64_t s = 0; s < n_local; ++s)
          for (uint64_t b = 0; b < n_blocks; ++b)
            CHECK(p.anchor_level(s, b) <= before[s * n_blocks + b], "anchor_level(%llu, %llu) rose from %zu to %zu", (ull)s, (ull)b, before[s * n_blocks + b],
                  p.anchor_level(s, b));
    }
    {                                                  // a finished session takes nothing
      FillPlan done = p;
      done.finished = true;
      std::string err;
      const uint64_t sb[2] = {first_slot, 0};
      const uint32_t lv[1] = {(uint32_t)depth};
      CHECK(!done.validate_anchored(sb, lv, 1, &err) && err.find("finished") != std::string::npos, "a finished session takes an anchored request");
    }

    // ---- a whole slot at lowest anchors, one request a call, in a shuffled order ----------------------------------------------------------
    FillPlan q;
    q.init(first_slot, n_local, n_blocks);
    q.derive_from_presence();
    q.keeps_nodes = true;
    for (uint64_t s = 0; s < n_local; ++s) {
      std::vector<uint64_t> order(n_blocks);
      for (uint64_t b = 0; b < n_blocks; ++b) order[b] = b;
      std::shuffle(order.begin(), order.end(), rng);
      uint64_t siblings = 0, bare = 0;
      for (uint64_t b : order) {
        const uint64_t sb[2] = {first_slot + s, b};
        const uint32_t lv[1] = {(uint32_t)q.anchor_level(s, b)}, verdict[1] = {0};
        uint32_t status[1];
        std::string err;
        CHECK(q.validate_anchored(sb, lv, 1, &err), "the lowest anchor is refused: %s", err.c_str());
        siblings += lv[0];
        bare += lv[0] == 0;
        q.mark_proved_anchored(sb, lv, verdict, 1);
        q.resolve(sb, verdict, 1, status);
        CHECK(status[0] == FILL_NEW, "a first block is %u", status[0]);
        q.commit(sb, status, 1);
      }
      ++whole_slots;
      if (n_blocks == 1) {
        // the one-block slot still gets its one round of compression, against a zero that has no row: one sibling, never known beforehand
        CHECK(siblings == 1 && depth == 1, "the one-block slot took %llu siblings", (ull)siblings);
      } else if ((n_blocks & (n_blocks - 1)) == 0) {
        ++pow2_slots;
        CHECK(siblings == n_blocks - 1, "a slot of %llu blocks took %llu siblings", (ull)n_blocks, (ull)siblings);
        CHECK(bare == n_blocks / 2, "%llu of %llu blocks needed no sibling", (ull)bare, (ull)n_blocks);
      } else {
        // an odd layer's last node brings a zero that has no row: at most one more per level
        CHECK(siblings >= n_blocks - 1 && siblings <= n_blocks - 1 + depth, "a slot of %llu blocks took %llu siblings", (ull)n_blocks, (ull)siblings);
      }
      for (uint64_t b = 0; b < n_blocks; ++b) CHECK(q.servable(s, b), "a slot filled at lowest anchors does not serve block %llu", (ull)b);
    }
    CHECK(q.n_missing() == 0, "%llu blocks are missing at the end", (ull)q.n_missing());
  }
  CHECK(anchored > 0 && zero_level > 0 && refused > 0 && same_call > 0 && odd_geoms > 0 && pow2_slots > 0, "the walk missed a case: %llu anchored, %llu at "
        "level 0, %llu refused, %llu same-call, %llu odd, %llu powers of two", (ull)anchored, (ull)zero_level, (ull)refused, (ull)same_call, (ull)odd_geoms,
        (ull)pow2_slots);
  std::printf("fill anchor ok: %d sessions, %llu steps, %llu anchored requests proved (%llu at level 0), %llu refusals (%llu on a same-call node), %llu whole "
              "slots (%llu of 2^k blocks), %d failures\n", rounds, (ull)steps, (ull)anchored, (ull)zero_level, (ull)refused, (ull)same_call, (ull)whole_slots,
              (ull)pow2_slots, failures);
  return failures ? 1 : 0;
}
