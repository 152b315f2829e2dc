// The host side of block multiproofs (csrc/multiproofs.cpp): which rows the multiproof of a set of blocks of one slot holds, which calls
// are refused, and the tables k_multiproof_layer (kernels.hip) works from.  No HIP in here: tests/host_check/multiproof_plan_check.cpp
// prints it for seeded inputs on the CPU, under AddressSanitizer + UBSan, and tests/multiproof_models.py restates it.
//
// For a non-empty set B of distinct blocks of a slot of n_blocks blocks let K_0 = B and K_{l+1} = { i >> 1 : i in K_l }; layer l of the
// tree has m_l nodes, m_0 = n_blocks, m_{l+1} = (m_l + 1) >> 1.  The multiproof of B is the rows (l, i ^ 1) over every level l < depth and
// every i in K_l with i ^ 1 not in K_l and i ^ 1 < m_l, by level and then by index.  A sibling past its layer's end is NOT sent (a single
// path carries a zero row there).  Checking computes every node of K_{l+1} from K_l and the sent rows with k_compress_layer's rule; the
// one node of K_depth is the slot root.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "block_proof_plan.hpp"

namespace cp2i {

// ---- layout -----------------------------------------------------------------------------------------------------------------------
// The rows of the multiproof of blocks[0, k) (strictly ascending, every one below n_blocks, k > 0: multiproof_list_ok), as (level, index)
// pairs appended to *level_index when that is not NULL.  Returns their number.
inline size_t multiproof_layout(uint64_t n_blocks, const uint64_t* blocks, size_t k, std::vector<uint64_t>* level_index) {
  std::vector<uint64_t> cur(blocks, blocks + k), next;
  const size_t depth = block_proof_depth(n_blocks);
  size_t rows = 0;
  uint64_t m = n_blocks;
  for (size_t l = 0; l < depth; ++l) {
    next.clear();
    for (size_t t = 0; t < cur.size(); ++t) {
      const uint64_t i = cur[t], sib = i ^ 1;
      const bool held = (i & 1) ? (t > 0 && cur[t - 1] == sib) : (t + 1 < cur.size() && cur[t + 1] == sib);
      if (!held && sib < m) {
        ++rows;
        if (level_index) {
          level_index->push_back(l);
          level_index->push_back(sib);
        }
      }
      if (next.empty() || next.back() != i >> 1) next.push_back(i >> 1);
    }
    cur.swap(next);
    m = (m + 1) >> 1;
  }
  return rows;
}

// a list a layout is made of: not empty, strictly ascending, every block below n_blocks
inline bool multiproof_list_ok(uint64_t n_blocks, const uint64_t* blocks, size_t k) {
  if (k == 0 || !blocks) return false;
  for (size_t i = 0; i < k; ++i)
    if (blocks[i] >= n_blocks || (i && blocks[i] <= blocks[i - 1])) return false;
  return true;
}

// ---- validation -------------------------------------------------------------------------------------------------------------------
// The requests of one call: groups is n_groups x 2 (slot or root index, count), blocks the sum of the counts, group after group.  The rules
// in the order the header states them, each over every group before the next: a count of 0; a first entry outside [first, first + n_local)
// (`what` names it: "slot" with the dataset's local range, "root index" with first = 0 and n_local = n_roots); a block at or past
// n_blocks; blocks not strictly ascending inside a group; n_rows different from the sum of the groups' layouts.  false with *err naming
// the rule and the lowest group (and request) that breaks it.  *n_out receives the number of requests.
inline bool multiproof_count(const uint64_t* groups, size_t n_groups, size_t* n_out) {
  uint64_t n = 0;
  for (size_t g = 0; g < n_groups; ++g) {
    if (groups[2 * g + 1] > UINT64_MAX - n) return false;
    n += groups[2 * g + 1];
  }
  if (n > SIZE_MAX / 64) return false;
  *n_out = (size_t)n;
  return true;
}
inline bool multiproof_validate(const char* call, const char* what, const uint64_t* groups, size_t n_groups, const uint64_t* blocks, uint64_t first,
                                uint64_t n_local, uint64_t n_blocks, bool check_rows, uint64_t n_rows, uint64_t* rows_out, std::string* err) {
  const std::string head = std::string(call) + ": group ";
  for (size_t g = 0; g < n_groups; ++g)
    if (groups[2 * g + 1] == 0) {
      *err = head + std::to_string(g) + " holds no block";
      return false;
    }
  for (size_t g = 0; g < n_groups; ++g) {
    const uint64_t s = groups[2 * g];
    if (s < first || s - first >= n_local) {
      *err = head + std::to_string(g) + ": " + what + " " + std::to_string(s) + " is not inside the range " + std::to_string(first) + " + " +
             std::to_string(n_local);
      return false;
    }
  }
  size_t at = 0;
  for (size_t g = 0; g < n_groups; ++g)
    for (uint64_t j = 0; j < groups[2 * g + 1]; ++j, ++at)
      if (blocks[at] >= n_blocks) {
        *err = head + std::to_string(g) + ", request " + std::to_string(at) + ": block " + std::to_string(blocks[at]) + " is not below nBlocks = " +
               std::to_string(n_blocks);
        return false;
      }
  at = 0;
  for (size_t g = 0; g < n_groups; ++g)
    for (uint64_t j = 0; j < groups[2 * g + 1]; ++j, ++at)
      if (j && blocks[at] <= blocks[at - 1]) {
        *err = head + std::to_string(g) + ", request " + std::to_string(at) + ": block " + std::to_string(blocks[at]) + " does not ascend from " +
               std::to_string(blocks[at - 1]);
        return false;
      }
  uint64_t rows = 0;
  at = 0;
  for (size_t g = 0; g < n_groups; ++g) {
    rows += multiproof_layout(n_blocks, blocks + at, (size_t)groups[2 * g + 1], nullptr);
    at += (size_t)groups[2 * g + 1];
  }
  if (rows_out) *rows_out = rows;
  if (check_rows && rows != n_rows) {
    *err = std::string(call) + ": n_rows = " + std::to_string(n_rows) + ", the groups' layouts hold " + std::to_string(rows) + " rows";
    return false;
  }
  return true;
}

// ---- the work table and the jobs --------------------------------------------------------------------------------------------------
// The work table of a call, 32-byte rows: the n leaf rows in request order, the n_rows sent rows in packed order, then the computed rows
// level after level, group-major inside a level.  One job per computed row; job k of level l writes row level_base[l] + k.
struct MultiproofJob {
  uint32_t left;       // a work-table row
  uint32_t right;      // a work-table row, or MULTIPROOF_ZERO: the zero beside an odd layer's last node
  uint32_t key_last;   // the compression's key 0..3 | last << 8; last: the job's row is its group's top, compared with the stated root
  uint32_t group;
};
constexpr uint32_t MULTIPROOF_ZERO = 0xFFFFFFFFu;
constexpr uint64_t MULTIPROOF_ROW_LIMIT = 0xFFFFFFFFull;   // a call whose rows would reach it is refused: rows are 32-bit, ~0 is the zero

// whether a table of `rows` rows that `more` are added to stays below the limit
inline bool multiproof_rows_fit(uint64_t rows, uint64_t more) { return rows < MULTIPROOF_ROW_LIMIT && more < MULTIPROOF_ROW_LIMIT - rows; }

struct MultiproofPlan {
  size_t n = 0, n_rows = 0, n_work = 0;       // leaves, sent rows, all rows
  std::vector<uint64_t> level_base;           // per level: the first row its jobs write ...
  std::vector<uint64_t> level_off;            // ... and its first job in `jobs`, one more entry than levels
  std::vector<MultiproofJob> jobs;
  // what every row is: its group, level and index inside that level of the group's tree (the commit list of a fill)
  std::vector<uint32_t> row_group, row_level;
  std::vector<uint64_t> row_index;
  size_t levels() const { return level_base.size(); }
  size_t computed() const { return jobs.size(); }
};

// The plan of validated groups; n_blocks_of[g] is the block count of group g's slot (one value for every group of a call of the boundary;
// the launcher test mixes depths).  false with *err when the rows would reach MULTIPROOF_ROW_LIMIT.
inline bool multiproof_plan(const uint64_t* counts, const uint64_t* n_blocks_of, size_t n_groups, const uint64_t* blocks, MultiproofPlan* p,
                            std::string* err) {
  struct Node {
    uint64_t index;
    uint32_t row;
  };
  *p = MultiproofPlan();
  std::vector<std::vector<Node>> cur(n_groups);
  std::vector<uint64_t> m(n_groups), sent(n_groups);
  std::vector<size_t> depth(n_groups);
  uint64_t n = 0, n_rows = 0;
  size_t max_depth = 0;
  const auto refuse = [&]() {
    *err = "multiproof: the rows of this call reach 2^32 - 1";
    return false;
  };
  for (size_t g = 0; g < n_groups; ++g) {
    if (!multiproof_rows_fit(n, counts[g])) return refuse();
    n += counts[g];
  }
  uint64_t at = 0;
  for (size_t g = 0; g < n_groups; ++g)
    for (uint64_t j = 0; j < counts[g]; ++j, ++at) {
      p->row_group.push_back((uint32_t)g);
      p->row_level.push_back(0);
      p->row_index.push_back(blocks[at]);
    }
  at = 0;
  for (size_t g = 0; g < n_groups; ++g) {
    const size_t k = (size_t)counts[g];
    std::vector<uint64_t> li;
    multiproof_layout(n_blocks_of[g], blocks + at, k, &li);
    if (!multiproof_rows_fit(n + n_rows, li.size() / 2)) return refuse();
    sent[g] = n + n_rows;
    for (size_t r = 0; r < li.size() / 2; ++r) {
      p->row_group.push_back((uint32_t)g);
      p->row_level.push_back((uint32_t)li[2 * r]);
      p->row_index.push_back(li[2 * r + 1]);
    }
    n_rows += li.size() / 2;
    cur[g].resize(k);
    for (size_t j = 0; j < k; ++j) cur[g][j] = Node{blocks[at + j], (uint32_t)(at + j)};
    m[g] = n_blocks_of[g];
    depth[g] = block_proof_depth(n_blocks_of[g]);
    if (depth[g] > max_depth) max_depth = depth[g];
    at += k;
  }
  p->n = (size_t)n;
  p->n_rows = (size_t)n_rows;
  uint64_t base = n + n_rows;
  std::vector<Node> next;
  for (size_t l = 0; l < max_depth; ++l) {
    p->level_base.push_back(base);
    p->level_off.push_back(p->jobs.size());
    for (size_t g = 0; g < n_groups; ++g) {
      if (depth[g] <= l) continue;
      const std::vector<Node>& c = cur[g];
      const uint32_t last = l + 1 == depth[g] ? 1u : 0u;
      next.clear();
      for (size_t t = 0; t < c.size(); ++t) {
        const uint64_t i = c[t].index;
        MultiproofJob j;
        uint32_t tail = 0;
        if (i & 1) {                                             // the left sibling is not held (it would have taken this node with it)
          j.left = (uint32_t)sent[g]++;
          j.right = c[t].row;
        } else {
          j.left = c[t].row;
          if (t + 1 < c.size() && c[t + 1].index == i + 1) j.right = c[++t].row;
          else if (i + 1 < m[g]) j.right = (uint32_t)sent[g]++;
          else {
            j.right = MULTIPROOF_ZERO;
            tail = 2;
          }
        }
        j.key_last = ((l == 0 ? 1u : 0u) + tail) | last << 8;
        j.group = (uint32_t)g;
        if (!multiproof_rows_fit(base, 1)) return refuse();
        next.push_back(Node{i >> 1, (uint32_t)base});
        ++base;
        p->jobs.push_back(j);
        p->row_group.push_back((uint32_t)g);
        p->row_level.push_back((uint32_t)l + 1);
        p->row_index.push_back(i >> 1);
      }
      cur[g] = next;
      m[g] = (m[g] + 1) >> 1;
    }
  }
  p->level_off.push_back(p->jobs.size());
  p->n_work = (size_t)base;
  return true;
}

}  // namespace cp2i
