// The host side of multiproofs against what a fill session knows (cp2_fill_multiproof_want, cp2_fill_add_multi_anchored; fill.cpp): which
// rows a group of blocks still needs from a peer, and the tables the device works from.  No HIP in here:
// tests/host_check/multiproof_anchor_check.cpp prints it for seeded inputs on the CPU, under AddressSanitizer + UBSan, and
// tests/multiproof_anchor_models.py restates it.
//
// The geometry is multiproof_plan.hpp's.  known(l, i) says whether the session holds the authentic node i of level l; (depth, 0), the
// stated slot root, always counts as known.  For a non-empty set B of distinct blocks let A_0 = B; for l = 0 .. depth and every i in A_l:
//   known(l, i)      (l, i) is a TOP: the value that reaches it is compared with the kept row (the stated root at l = depth).  A top puts
//                    nothing into A_{l+1}; a top of level 0 is the fresh block root itself.
//   otherwise        i >> 1 is in A_{l+1}, and when i ^ 1 < m_l the sibling comes (a) from the call, when i ^ 1 is in A_l and unknown;
//                    (b) from the session's buffer when known(l, i ^ 1): a KEPT INPUT, never sent, used even when i ^ 1 is a top too;
//                    (c) else it is SENT: a row of the want list.  i ^ 1 >= m_l: the zero under key + 2.
// The want list is the sent rows (l, i ^ 1) by level and then by index: multiproof_layout's order, and its rows when only the root is
// known.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "multiproof_plan.hpp"

namespace cp2i {

struct AnchorNode {
  uint64_t index;
  uint32_t row;   // its row of the work table (the plan builder's; the want list leaves it 0)
};
enum AnchorSibling { ANCHOR_SIB_PAIR = 0, ANCHOR_SIB_KEPT = 1, ANCHOR_SIB_SENT = 2, ANCHOR_SIB_ZERO = 3 };

// One level of one group's walk, the one statement of the rules above.  cur: A_l ascending.  top(node) is called for every known node;
// parent(node, kind, pair_row) for every unknown node that is not consumed as the right half of a pair, with what its sibling is (kind;
// pair_row: the row of the right node of a pair), and returns the row of the parent, which goes into *next (A_{l+1}, ascending).
template <class Known, class Top, class Parent>
inline void multiproof_anchor_level(const std::vector<AnchorNode>& cur, uint64_t m, const Known& known, std::vector<AnchorNode>* next, const Top& top,
                                    const Parent& parent) {
  next->clear();
  for (size_t t = 0; t < cur.size(); ++t) {
    const uint64_t i = cur[t].index, sib = i ^ 1;
    if (known(i)) {
      top(cur[t]);
      continue;
    }
    AnchorSibling kind;
    uint32_t pair_row = 0;
    if (sib >= m) kind = ANCHOR_SIB_ZERO;
    else if (known(sib)) kind = ANCHOR_SIB_KEPT;
    else if (!(i & 1) && t + 1 < cur.size() && cur[t + 1].index == sib) {   // (an unknown left sibling in A_l has taken an odd i with it)
      kind = ANCHOR_SIB_PAIR;
      pair_row = cur[++t].row;
    } else kind = ANCHOR_SIB_SENT;
    next->push_back(AnchorNode{i >> 1, parent(cur[t - (kind == ANCHOR_SIB_PAIR ? 1 : 0)], kind, pair_row)});
  }
}

// The want list of blocks[0, k) (multiproof_list_ok) against known(level, index), as (level, index) pairs appended to *level_index when
// that is not NULL.  Returns the number of rows.
template <class Known>
inline size_t multiproof_want(uint64_t n_blocks, const uint64_t* blocks, size_t k, const Known& known, std::vector<uint64_t>* level_index) {
  const size_t depth = block_proof_depth(n_blocks);
  std::vector<AnchorNode> cur(k), next;
  for (size_t j = 0; j < k; ++j) cur[j] = AnchorNode{blocks[j], 0};
  size_t rows = 0;
  uint64_t m = n_blocks;
  for (size_t l = 0; l <= depth && !cur.empty(); ++l) {
    multiproof_anchor_level(
        cur, m, [&](uint64_t i) { return l == depth || known(l, i); }, &next, [](const AnchorNode&) {},
        [&](const AnchorNode& node, AnchorSibling kind, uint32_t) -> uint32_t {
          if (kind == ANCHOR_SIB_SENT) {
            ++rows;
            if (level_index) {
              level_index->push_back(l);
              level_index->push_back(node.index ^ 1);
            }
          }
          return 0;
        });
    cur.swap(next);
    m = (m + 1) >> 1;
  }
  return rows;
}

// ---- validation -------------------------------------------------------------------------------------------------------------------
// multiproof_validate's rules in their order over the requests of one call, with its last rule against the session: n_rows (when
// check_rows) must be the sum of the groups' want lists against known(group, level, index) AS IT STANDS -- a list made before another add
// landed is stale, and shows here.  *rows_out, group_rows (n_groups) and *level_index (the lists packed in group order) may be NULL.
template <class Known>
inline bool multiproof_anchor_validate(const char* call, const uint64_t* groups, size_t n_groups, const uint64_t* blocks, uint64_t first, uint64_t n_local,
                                       uint64_t n_blocks, const Known& known, bool check_rows, uint64_t n_rows, uint64_t* rows_out, uint64_t* group_rows,
                                       std::vector<uint64_t>* level_index, std::string* err) {
  if (!multiproof_validate(call, "slot", groups, n_groups, blocks, first, n_local, n_blocks, false, 0, nullptr, err)) return false;
  uint64_t rows = 0;
  size_t at = 0;
  for (size_t g = 0; g < n_groups; ++g) {
    const size_t r = multiproof_want(
        n_blocks, blocks + at, (size_t)groups[2 * g + 1], [&](size_t l, uint64_t i) { return known(g, l, i); }, level_index);
    if (group_rows) group_rows[g] = r;
    rows += r;
    at += (size_t)groups[2 * g + 1];
  }
  if (rows_out) *rows_out = rows;
  if (check_rows && rows != n_rows) {
    *err = std::string(call) + ": n_rows = " + std::to_string(n_rows) + ", the groups' want lists against the session as it stands hold " +
           std::to_string(rows) + " rows";
    return false;
  }
  return true;
}

// ---- rows by place -----------------------------------------------------------------------------------------------------------------
// The requests of cp2_dataset_block_tree_rows and cp2_fill_block_tree_rows: places is n x 3 (dataset slot, level, index); every slot
// inside [first, first + n_local), every level at most depth (depth: the slot root), every index below its layer's size
// (layer_sizes: depth + 1 entries).  false with *err naming the lowest request that breaks a rule.
inline bool tree_places_validate(const char* call, const uint64_t* places, size_t n, uint64_t first, uint64_t n_local,
                                 const std::vector<size_t>& layer_sizes, std::string* err) {
  for (size_t i = 0; i < n; ++i) {
    const uint64_t s = places[3 * i], l = places[3 * i + 1], x = places[3 * i + 2];
    const std::string head = std::string(call) + ": request " + std::to_string(i) + ": ";
    if (s < first || s - first >= n_local) {
      *err = head + "slot " + std::to_string(s) + " is not inside the local range " + std::to_string(first) + " + " + std::to_string(n_local);
      return false;
    }
    if (l >= layer_sizes.size()) {
      *err = head + "level " + std::to_string(l) + " is above the depth " + std::to_string(layer_sizes.size() - 1);
      return false;
    }
    if (x >= layer_sizes[(size_t)l]) {
      *err = head + "index " + std::to_string(x) + " is not below the " + std::to_string(layer_sizes[(size_t)l]) + " node(s) of level " + std::to_string(l);
      return false;
    }
  }
  return true;
}

// ---- the work table, the jobs, the tops and the commit list -------------------------------------------------------------------------
// The work table of a call: the n leaf rows in request order, the n_rows sent rows in packed order, the n_kept kept inputs group after
// group in the order the walk meets them, then the computed rows level after level, group-major inside a level.  No job has `last` set:
// the verdicts come from the tops.
struct MultiproofAnchorPlan : MultiproofPlan {
  size_t n_kept = 0;
  std::vector<uint32_t> top_row, top_group, top_level;   // group-major; inside a group by level, then by index
  std::vector<uint64_t> top_index;
  std::vector<uint64_t> top_off;                         // n_groups + 1
  std::vector<uint32_t> commit;                          // the rows a proved group leaves: unknown leaves, sent rows, computed non-tops
  size_t n_tops() const { return top_row.size(); }
  size_t kept_base() const { return n + n_rows; }
};

// The plan of validated groups against known(group, level, index); n_blocks_of[g] is the block count of group g's slot.  false with *err
// when the rows would reach MULTIPROOF_ROW_LIMIT.  With only the roots known: multiproof_plan's numbering and jobs (without `last`), one
// top per group, and every row but the tops in the commit list.
template <class Known>
inline bool multiproof_anchor_plan(const uint64_t* counts, const uint64_t* n_blocks_of, size_t n_groups, const uint64_t* blocks, const Known& known,
                                   MultiproofAnchorPlan* p, std::string* err) {
  *p = MultiproofAnchorPlan();
  const auto refuse = [&]() {
    *err = "multiproof: the rows of this call reach 2^32 - 1";
    return false;
  };
  uint64_t n = 0;
  for (size_t g = 0; g < n_groups; ++g) {
    if (!multiproof_rows_fit(n, counts[g])) return refuse();
    n += counts[g];
  }
  std::vector<size_t> depth(n_groups);
  std::vector<uint64_t> first(n_groups);
  size_t max_depth = 0;
  uint64_t at = 0;
  for (size_t g = 0; g < n_groups; ++g) {
    depth[g] = block_proof_depth(n_blocks_of[g]);
    if (depth[g] > max_depth) max_depth = depth[g];
    first[g] = at;
    for (uint64_t j = 0; j < counts[g]; ++j, ++at) {
      p->row_group.push_back((uint32_t)g);
      p->row_level.push_back(0);
      p->row_index.push_back(blocks[at]);
    }
  }
  // pass 1, group after group: the sent rows, then the kept inputs, in the order the walk meets them
  struct Place {
    uint32_t group, level;
    uint64_t index;
  };
  std::vector<Place> kept;
  std::vector<uint64_t> sent_at(n_groups), kept_at(n_groups);
  std::vector<AnchorNode> cur, next;
  uint64_t n_rows = 0;
  for (size_t g = 0; g < n_groups; ++g) {
    sent_at[g] = n_rows;
    kept_at[g] = kept.size();
    cur.resize((size_t)counts[g]);
    for (size_t j = 0; j < cur.size(); ++j) cur[j] = AnchorNode{blocks[first[g] + j], 0};
    uint64_t m = n_blocks_of[g];
    for (size_t l = 0; l <= depth[g] && !cur.empty(); ++l) {
      multiproof_anchor_level(
          cur, m, [&](uint64_t i) { return l == depth[g] || known(g, l, i); }, &next, [](const AnchorNode&) {},
          [&](const AnchorNode& node, AnchorSibling kind, uint32_t) -> uint32_t {
            if (kind == ANCHOR_SIB_SENT) {
              ++n_rows;
              p->row_group.push_back((uint32_t)g);
              p->row_level.push_back((uint32_t)l);
              p->row_index.push_back(node.index ^ 1);
            } else if (kind == ANCHOR_SIB_KEPT) kept.push_back(Place{(uint32_t)g, (uint32_t)l, node.index ^ 1});
            return 0;
          });
      cur.swap(next);
      m = (m + 1) >> 1;
    }
    if (!multiproof_rows_fit(n, n_rows) || !multiproof_rows_fit(n + n_rows, kept.size())) return refuse();
  }
  for (const Place& k : kept) {
    p->row_group.push_back(k.group);
    p->row_level.push_back(k.level);
    p->row_index.push_back(k.index);
  }
  p->n = (size_t)n;
  p->n_rows = (size_t)n_rows;
  p->n_kept = kept.size();
  for (size_t g = 0; g < n_groups; ++g) {
    sent_at[g] += n;
    kept_at[g] += n + n_rows;
  }
  // pass 2, level after level over all groups: the jobs and the tops
  struct Top {
    uint32_t row, level;
    uint64_t index;
  };
  std::vector<std::vector<AnchorNode>> level_of(n_groups);
  std::vector<std::vector<Top>> tops(n_groups);
  std::vector<uint64_t> m(n_groups);
  for (size_t g = 0; g < n_groups; ++g) {
    level_of[g].resize((size_t)counts[g]);
    for (size_t j = 0; j < level_of[g].size(); ++j) level_of[g][j] = AnchorNode{blocks[first[g] + j], (uint32_t)(first[g] + j)};
    m[g] = n_blocks_of[g];
  }
  uint64_t base = n + n_rows + kept.size();
  bool full = false;
  for (size_t l = 0; l <= max_depth; ++l) {
    if (l < max_depth) {
      p->level_base.push_back(base);
      p->level_off.push_back(p->jobs.size());
    }
    for (size_t g = 0; g < n_groups; ++g) {
      if (depth[g] < l || level_of[g].empty()) continue;
      multiproof_anchor_level(
          level_of[g], m[g], [&](uint64_t i) { return l == depth[g] || known(g, l, i); }, &next,
          [&](const AnchorNode& node) { tops[g].push_back(Top{node.row, (uint32_t)l, node.index}); },
          [&](const AnchorNode& node, AnchorSibling kind, uint32_t pair_row) -> uint32_t {
            const uint32_t other = kind == ANCHOR_SIB_PAIR   ? pair_row
                                   : kind == ANCHOR_SIB_KEPT ? (uint32_t)kept_at[g]++
                                   : kind == ANCHOR_SIB_SENT ? (uint32_t)sent_at[g]++
                                                             : MULTIPROOF_ZERO;
            MultiproofJob j;
            if (node.index & 1) {
              j.left = other;
              j.right = node.row;
            } else {
              j.left = node.row;
              j.right = other;
            }
            j.key_last = (l == 0 ? 1u : 0u) + (kind == ANCHOR_SIB_ZERO ? 2u : 0u);
            j.group = (uint32_t)g;
            if (!multiproof_rows_fit(base, 1)) full = true;
            p->jobs.push_back(j);
            p->row_group.push_back((uint32_t)g);
            p->row_level.push_back((uint32_t)l + 1);
            p->row_index.push_back(node.index >> 1);
            return (uint32_t)base++;
          });
      if (full) return refuse();
      level_of[g].swap(next);
      m[g] = (m[g] + 1) >> 1;
    }
  }
  p->level_off.push_back(p->jobs.size());
  p->n_work = (size_t)base;
  // the tops group-major, and what is left of the table once they and the kept inputs are taken out
  std::vector<bool> is_top(p->n_work, false);
  for (size_t g = 0; g < n_groups; ++g) {
    p->top_off.push_back(p->top_row.size());
    for (const Top& t : tops[g]) {
      p->top_row.push_back(t.row);
      p->top_group.push_back((uint32_t)g);
      p->top_level.push_back(t.level);
      p->top_index.push_back(t.index);
      is_top[t.row] = true;
    }
  }
  p->top_off.push_back(p->top_row.size());
  for (size_t r = 0; r < p->n_work; ++r)
    if (!is_top[r] && !(r >= p->kept_base() && r < p->kept_base() + p->n_kept)) p->commit.push_back((uint32_t)r);
  return true;
}

}  // namespace cp2i
