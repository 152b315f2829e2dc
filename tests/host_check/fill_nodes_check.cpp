// What a serving fill session knows (csrc/fill_plan.hpp: node_row, mark_proved, derive_from_presence, servable) walked over random
// geometries -- 1 ... 64 blocks a slot, odd counts included, 1 ... 4 local slots -- with random arrival orders, requests that do not
// prove, proved blocks that are not written, and node keeping turned on at a random point.  Every answer is compared with a restatement
// kept here: rows against a brute-force layout, the known bits against a set of (slot, layer, index) triples, and after every step
// servable(b) <=> b is present and every in-range sibling row of block_proof_rows (csrc/block_proof_plan.hpp) is known.  The two
// corollaries the design rests on come out of the walk: a block added after keeping was turned on is servable from the moment its bit is
// set, and after derive_from_presence on a complete session every block is.  Built with AddressSanitizer + UBSan.  No GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
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
  size_t depth() const { return sizes.size() - 1; }
  // layer-major over the slots: every layer below `level` whole, then the slots before this one
  uint64_t row(uint64_t local, size_t level, uint64_t index) const {
    uint64_t r = 0;
    for (size_t l = 0; l < level; ++l) r += n_local * sizes[l];
    return r + local * sizes[level] + index;
  }
  void prove(uint64_t local, uint64_t b) {
    known.insert(Node(local, 0, b));
    uint64_t j = b;
    for (size_t l = 0; l < depth(); ++l) {
      if ((j ^ 1) < sizes[l]) known.insert(Node(local, l, j ^ 1));
      j /= 2;
      known.insert(Node(local, l + 1, j));
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

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 1000;
  std::mt19937_64 rng(20261018);
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  uint64_t steps = 0, served_late = 0, partial_seen = 0, odd_geoms = 0;

  for (int round = 0; round < rounds; ++round) {
    const uint64_t n_blocks = round % 9 == 0 ? 1 : pick(1, 64), n_local = pick(1, 4), first_slot = pick(0, 9);
    odd_geoms += n_blocks & 1;
    FillPlan p;
    p.init(first_slot, n_local, n_blocks);
    Model m{n_local, n_blocks, layers(n_blocks), {}, {}};
    const size_t depth = m.depth();
    CHECK(p.depth() == depth && depth == block_proof_depth(n_blocks), "depth %zu for %llu blocks", p.depth(), (unsigned long long)n_blocks);
    CHECK(p.known.size() == (p.rows + 63) / 64, "the known bitmap has %zu words for %zu rows", p.known.size(), p.rows);

    // ---- the row arithmetic: the brute-force layout, and the rows a proof is gathered from -------------------------------------------
    std::set<uint64_t> seen;
    for (uint64_t s = 0; s < n_local; ++s)
      for (size_t l = 0; l <= depth; ++l)
        for (uint64_t k = 0; k < m.sizes[l]; ++k) {
          const uint64_t r = p.node_row(l, s, k);
          CHECK(r == m.row(s, l, k) && r < p.rows, "node_row(%zu, %llu, %llu) = %llu", l, (unsigned long long)s, (unsigned long long)k, (unsigned long long)r);
          seen.insert(r);
        }
    CHECK(seen.size() == p.rows, "node_row reaches %zu of %zu rows", seen.size(), p.rows);
    for (uint64_t s = 0; s < n_local; ++s)
      for (uint64_t b = 0; b < n_blocks; ++b) {
        CHECK(p.node_row(0, s, b) == p.dest_row(first_slot + s, b), "layer 0 is not where the block roots go");
        std::vector<uint64_t> rows(depth);
        block_proof_rows(p.coff, p.csizes, s, b, depth, rows.data());
        for (size_t l = 0; l < depth; ++l) {
          const uint64_t sib = (b >> l) ^ 1;
          CHECK(rows[l] == (sib < m.sizes[l] ? p.node_row(l, s, sib) : BLOCK_PROOF_NO_ROW), "sibling row of level %zu", l);
        }
      }

    // ---- the session: every block once in a random order, with noise, keeping turned on at a random point ------------------------------
    std::vector<std::pair<uint64_t, uint64_t>> order;
    for (uint64_t s = 0; s < n_local; ++s)
      for (uint64_t b = 0; b < n_blocks; ++b) order.push_back({s, b});
    std::shuffle(order.begin(), order.end(), rng);
    const size_t keep_at = (size_t)pick(0, order.size());
    bool keeping = false;
    auto compare = [&]() {
      ++steps;
      for (uint64_t s = 0; s < n_local; ++s) {
        for (size_t l = 0; l <= depth; ++l)
          for (uint64_t k = 0; k < m.sizes[l]; ++k)
            CHECK(p.is_known(p.node_row(l, s, k)) == (m.known.count(Node(s, l, k)) != 0), "known(%zu, %llu, %llu) differs, round %d", l,
                  (unsigned long long)s, (unsigned long long)k, round);
        for (uint64_t b = 0; b < n_blocks; ++b) {
          const bool here = m.present.count({s, b}) != 0;
          std::vector<uint64_t> rows(depth);
          block_proof_rows(p.coff, p.csizes, s, b, depth, rows.data());
          bool all = true;
          for (uint64_t r : rows)
            if (r != BLOCK_PROOF_NO_ROW && !p.is_known(r)) all = false;
          CHECK(p.present(s, b) == here, "presence differs");
          CHECK(p.servable(s, b) == (here && all), "servable(%llu, %llu) = %d, present %d, siblings known %d, round %d", (unsigned long long)s,
                (unsigned long long)b, (int)p.servable(s, b), (int)here, (int)all, round);
          const uint32_t want = !here ? FILL_PROOF_ABSENT : all ? FILL_PROOF_OK : FILL_PROOF_PARTIAL;
          CHECK(p.proof_status(s, b) == want, "proof_status differs");
          partial_seen += want == FILL_PROOF_PARTIAL;
        }
      }
    };
    auto keep = [&]() {
      p.derive_from_presence();
      p.keeps_nodes = true;
      m.derive();
      keeping = true;
      compare();
    };
    for (size_t at = 0; at < order.size();) {
      if (!keeping && at >= keep_at) keep();
      // one call: some of the next blocks, a request that does not prove, a proved block whose write fails, a repeat
      const size_t take = std::min<size_t>((size_t)pick(1, 6), order.size() - at);
      std::vector<uint64_t> sb;
      std::vector<uint32_t> verdict, written;
      std::vector<size_t> fresh;                     // indices of the requests that are new, proved and written
      for (size_t k = 0; k < take; ++k) {
        sb.push_back(first_slot + order[at + k].first); sb.push_back(order[at + k].second);
        verdict.push_back(0); written.push_back(FILL_WRITE);
        fresh.push_back(verdict.size() - 1);
        if (pick(0, 3) == 0) {                       // the same block again from another peer
          sb.push_back(first_slot + order[at + k].first); sb.push_back(order[at + k].second);
          verdict.push_back(0); written.push_back(FILL_SKIP);
        }
      }
      const std::pair<uint64_t, uint64_t> wrong = order[(size_t)pick(0, order.size() - 1)];
      sb.push_back(first_slot + wrong.first); sb.push_back(wrong.second);
      verdict.push_back(1); written.push_back(FILL_SKIP);
      size_t unwritten = ~(size_t)0;                 // a block of a LATER position proves but is not written: missing, its nodes known
      if (at + take < order.size() && pick(0, 2) == 0) {
        const auto& u = order[(size_t)pick(at + take, order.size() - 1)];
        sb.push_back(first_slot + u.first); sb.push_back(u.second);
        verdict.push_back(0); written.push_back(FILL_WRITE_FAILED);
        unwritten = verdict.size() - 1;
        if (keeping) m.prove(u.first, u.second);
      }
      const size_t n = verdict.size();
      std::vector<uint32_t> status(n);
      if (keeping) p.mark_proved(sb.data(), verdict.data(), n);
      p.resolve(sb.data(), verdict.data(), n, status.data());
      FillPlan::roll_back(sb.data(), written, status.data());
      if (unwritten != ~(size_t)0) CHECK(status[unwritten] == FILL_UNWRITTEN, "the failed write is %u", status[unwritten]);
      p.commit(sb.data(), status.data(), n);
      for (size_t i : fresh) {
        const uint64_t s = sb[2 * i] - first_slot, b = sb[2 * i + 1];
        CHECK(status[i] == FILL_NEW, "a first proved block is %u", status[i]);
        m.present.insert({s, b});
        if (keeping) {
          m.prove(s, b);
          CHECK(p.servable(s, b), "a block added after keeping is not servable at once: (%llu, %llu), round %d", (unsigned long long)s,
                (unsigned long long)b, round);
          ++served_late;
        }
      }
      at += take;
      if (keeping) compare();
    }
    if (!keeping) keep();                             // keep_at == the end: a complete session, derived
    CHECK(p.n_missing() == 0, "%llu blocks are missing at the end", (unsigned long long)p.n_missing());
    for (uint64_t s = 0; s < n_local; ++s)
      for (uint64_t b = 0; b < n_blocks; ++b) CHECK(p.servable(s, b), "a complete session does not serve (%llu, %llu)", (unsigned long long)s, (unsigned long long)b);

    // ---- a complete session that never kept nodes: one derivation makes every row known and every block servable -------------------------
    FillPlan q;
    q.init(first_slot, n_local, n_blocks);
    std::fill(q.bits.begin(), q.bits.end(), 0);
    std::vector<uint64_t> all_sb;
    std::vector<uint32_t> all_new;
    for (const auto& o : order) { all_sb.push_back(first_slot + o.first); all_sb.push_back(o.second); all_new.push_back(FILL_NEW); }
    q.commit(all_sb.data(), all_new.data(), all_new.size());
    for (uint64_t s = 0; s < n_local; ++s)
      for (uint64_t b = 0; b < n_blocks; ++b) CHECK(!q.servable(s, b) || depth == 0 || (n_blocks == 1), "servable before anything is known");
    q.derive_from_presence();
    for (uint64_t r = 0; r < q.rows; ++r) CHECK(q.is_known(r), "row %llu of a complete session is unknown", (unsigned long long)r);
    for (uint64_t s = 0; s < n_local; ++s)
      for (uint64_t b = 0; b < n_blocks; ++b) CHECK(q.servable(s, b), "a derived complete session does not serve (%llu, %llu)", (unsigned long long)s, (unsigned long long)b);
  }
  CHECK(served_late > 0 && partial_seen > 0 && odd_geoms > 0, "the walk missed a case: %llu late, %llu partial, %llu odd", (unsigned long long)served_late,
        (unsigned long long)partial_seen, (unsigned long long)odd_geoms);
  std::printf("fill nodes ok: %d sessions, %llu compared states, %llu blocks served at once, %llu partial answers, %d failures\n", rounds,
              (unsigned long long)steps, (unsigned long long)served_late, (unsigned long long)partial_seen, failures);
  return failures ? 1 : 0;
}
