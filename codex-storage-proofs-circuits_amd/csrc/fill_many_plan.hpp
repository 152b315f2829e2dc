// The host side of cp2_fills_add_many (csrc/fill_many.cpp): proved blocks added to many fill sessions in one pass.  The call is defined by
// the calls that exist -- per session cp2_fill_add / cp2_fill_add_anchored on the subsequence of the requests that name it -- so everything
// here is FillPlan's (fill_plan.hpp) applied per subsequence: the requests grouped by session, each session's own validation with the
// refusal's index turned back into the call's, the session table and the request arrays k_block_path_commit_many reads, the packed path
// offsets and the per-chunk maxima of path rows, and after the verdicts mark / resolve / write mask / roll-back / commit per session and
// the statuses scattered back.  Every step is linear in n + n_fills: no step scans all requests once per session.  No HIP in here:
// tests/host_check/fill_many_check.cpp walks it over seeded random calls on the CPU, under AddressSanitizer + UBSan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_set>
#include <vector>

#include "fill_plan.hpp"

namespace cp2i {

// one descriptor of the device's session table: cp2k::FillManySession (kernels.hpp) restated, field by field
struct FillManyDesc {
  uint64_t tree, n_rows, slot_roots, n_local, layer_tab, n_blocks;
  uint32_t depth, reserved;
};

// a session as the plan takes it: its FillPlan and the device addresses of its compact buffer, its stated roots and (keeping nodes) its
// layer tables
struct FillManyIn {
  FillPlan* plan = nullptr;
  uint64_t tree = 0, slot_roots = 0, layer_tab = 0;
};

// a refusal: which entry of `fills` (request == false) or which request of the call (request == true) broke a rule, and the text
struct FillManyRefusal {
  bool request = false;
  size_t index = 0;
  std::string text;
};

// the same session listed twice would be two writers to one file set: the later of the first such pair, or n_fills when all differ
inline size_t fill_many_listed_twice(const void* const* fills, size_t n_fills) {
  std::unordered_set<const void*> seen;
  for (size_t k = 0; k < n_fills; ++k)
    if (!seen.insert(fills[k]).second) return k;
  return n_fills;
}

struct FillManyPlan {
  size_t n = 0, n_fills = 0;
  bool whole = false;                     // levels == NULL: every request brings its session's whole path (cp2_fill_add per session)
  // R_k, the subsequence of the requests that name fills[k] in request order: order[start[k]] ... order[start[k + 1] - 1]
  std::vector<size_t> start, order;
  std::vector<uint64_t> pairs;            // (dataset slot, block) in grouped order: session k's own slot_block array at pairs[2 start[k]]
  std::vector<uint32_t> sub_levels;       // the levels in grouped order (the session's depth throughout when whole)
  // what the device reads: the table, and per request in REQUEST order the arrays of FillPlan::device_requests_anchored plus the session
  std::vector<FillManyDesc> table;
  std::vector<uint64_t> session_of, local_block, dest, path_off, anchor_row;
  std::vector<uint32_t> levels;

  size_t count(size_t k) const { return start[k + 1] - start[k]; }
  const uint64_t* pairs_of(size_t k) const { return pairs.data() + 2 * start[k]; }
  const uint32_t* levels_of(size_t k) const { return sub_levels.data() + start[k]; }
  const size_t* rows_of(size_t k) const { return order.data() + start[k]; }

  // ---- grouping ------------------------------------------------------------------------------------------------------------------------
  // req: n x 3 (index into fills, dataset slot, block).  A counting sort by session, stable, so every R_k is in request order.  false
  // with the lowest request whose session index is not below n_fills.
  bool group(const uint64_t* req, size_t n_req, size_t fills, FillManyRefusal* why) {
    n = n_req; n_fills = fills;
    start.assign(n_fills + 1, 0);
    for (size_t i = 0; i < n; ++i) {
      if (req[3 * i] >= n_fills) {
        *why = {true, i, "fills: request " + std::to_string(i) + ": session index " + std::to_string(req[3 * i]) + " is not below n_fills = " +
                             std::to_string(n_fills)};
        return false;
      }
      ++start[(size_t)req[3 * i] + 1];
    }
    for (size_t k = 0; k < n_fills; ++k) start[k + 1] += start[k];
    order.resize(n);
    pairs.resize(2 * n);
    std::vector<size_t> at(start.begin(), start.end() - 1);
    for (size_t i = 0; i < n; ++i) {
      const size_t g = at[(size_t)req[3 * i]]++;
      order[g] = i;
      pairs[2 * g] = req[3 * i + 1];
      pairs[2 * g + 1] = req[3 * i + 2];
    }
    return true;
  }

  // ---- validation ----------------------------------------------------------------------------------------------------------------------
  // A session's own refusal as the call's.  The index never comes out of the text: the session's rules run request by request, so the
  // failing request j of R_k is known and the call's index is order[start[k] + j]; of FillPlan's text only the reason is kept (what
  // follows its own "request <j>:").  A refusal that names no request (a finished session) names fills[k].
  FillManyRefusal refuse_session(size_t k, const std::string& err) const { return {false, k, "fills: fills[" + std::to_string(k) + "]: " + err}; }
  FillManyRefusal refuse_request(size_t k, size_t j, const std::string& err) const {
    const size_t i = order[start[k] + j], colon = err.find(": ", err.find("request "));
    const std::string reason = err.find("request ") != std::string::npos && colon != std::string::npos ? err.substr(colon + 2) : err;
    return {true, i, "fills: request " + std::to_string(i) + " (of fills[" + std::to_string(k) + "]): " + reason};
  }
  // Sessions in `fills` order, each over its own subsequence (an empty one too: a finished session is refused whether or not a request
  // names it).  whole: FillPlan::validate's rules.  With levels: a session that keeps nodes runs validate_anchored; one that keeps none
  // accepts whole paths only -- its depth exactly -- since a shorter walk ends at a node it does not hold.  Then `paths`: NULL only when
  // every level is 0.  Fills sub_levels.  false with the first refusal.
  bool validate(const FillManyIn* in, const uint32_t* lv, bool have_paths, FillManyRefusal* why) {
    whole = lv == nullptr;
    sub_levels.resize(n);
    for (size_t k = 0; k < n_fills; ++k) {
      const FillPlan& p = *in[k].plan;
      const size_t cnt = count(k), depth = p.depth();
      const uint64_t* sb = pairs_of(k);
      uint32_t* sl = sub_levels.data() + start[k];
      for (size_t j = 0; j < cnt; ++j) sl[j] = whole ? (uint32_t)depth : lv[order[start[k] + j]];
      std::string err;
      const bool anchored = !whole && p.keeps_nodes;
      if (!(anchored ? p.validate_anchored(sb, sl, 0, &err) : p.validate(sb, 0, &err))) {   // the session's own state: finished
        *why = refuse_session(k, err);
        return false;
      }
      for (size_t j = 0; j < cnt; ++j) {
        if (anchored) {
          if (!p.validate_anchored(sb + 2 * j, sl + j, 1, &err)) { *why = refuse_request(k, j, err); return false; }
          continue;
        }
        if (!p.validate_pair(j, sb[2 * j], sb[2 * j + 1], &err)) { *why = refuse_request(k, j, err); return false; }
        if (sl[j] > depth) {
          *why = refuse_request(k, j, "level " + std::to_string(sl[j]) + " is above the depth " + std::to_string(depth));
          return false;
        }
        if (sl[j] < depth) {
          *why = refuse_request(k, j, "level " + std::to_string(sl[j]) + " is below the depth " + std::to_string(depth) +
                                          " of a session that does not keep the nodes of the paths it proves: call cp2_fill_keep_nodes first");
          return false;
        }
      }
    }
    levels.resize(n);
    for (size_t g = 0; g < n; ++g) levels[order[g]] = sub_levels[g];
    for (size_t i = 0; !have_paths && i < n; ++i)      // in request order: the lowest request that brings a sibling
      if (levels[i]) {
        *why = {true, i, "fills: request " + std::to_string(i) + ": paths must not be NULL when a level is not 0"};
        return false;
      }
    return true;
  }

  // ---- what the device reads -------------------------------------------------------------------------------------------------------------
  // after validate: the session table and the request arrays; path_off has n + 1 entries, rows of the call's packed `paths`
  void tables(const FillManyIn* in, const uint64_t* req) {
    table.resize(n_fills);
    for (size_t k = 0; k < n_fills; ++k) {
      const FillPlan& p = *in[k].plan;
      table[k] = {in[k].tree, (uint64_t)p.rows, in[k].slot_roots, p.n_local, p.keeps_nodes ? in[k].layer_tab : 0, p.n_blocks, (uint32_t)p.depth(), 0};
    }
    session_of.resize(n); local_block.resize(2 * n); dest.resize(n); anchor_row.resize(n);
    path_off.resize(n + 1);
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) {
      const size_t k = (size_t)req[3 * i];
      const FillPlan& p = *in[k].plan;
      const uint64_t s = req[3 * i + 1], b = req[3 * i + 2];
      const size_t a = levels[i];
      session_of[i] = k;
      local_block[2 * i] = s - p.first_slot;
      local_block[2 * i + 1] = b;
      dest[i] = p.dest_row(s, b);
      anchor_row[i] = a >= p.depth() ? FillPlan::ANCHOR_SLOT_ROOT : p.node_row(a, s - p.first_slot, b >> a);
      path_off[i] = at;
      at += a;
    }
    path_off[n] = at;
  }
  // a chunk's packed paths are one contiguous range, rows [path_off[c0], path_off[c0 + m]): the most any chunk of `chunk` requests holds
  // (at least 1), which sizes the device's path buffer (x 32 bytes) and the walk's staging (x 64)
  uint64_t most_path_rows(size_t chunk) const {
    uint64_t most = 1;
    for (size_t c0 = 0; c0 < n; c0 += chunk) most = std::max(most, path_off[std::min(n, c0 + chunk)] - path_off[c0]);
    return most;
  }

  // ---- after the verdicts ------------------------------------------------------------------------------------------------------------------
  // Session k's share of the call, exactly fill_add_checked's sequence on R_k: the rows a proved path made known (mark_proved when whole,
  // mark_proved_anchored with levels, for a session that keeps nodes), NEW / DUPLICATE by the lowest proved index of R_k, the writer
  // (write(k, mask): repair_write's contract on the session's mask, FILL_WRITE in, FILL_WRITE_FAILED left where a file failed; not called
  // for the fake source, write_files == false), its roll-back, presence.  verdict and status are the call's arrays, in request order;
  // returns the number of bits set.
  template <class Write>
  size_t apply(size_t k, FillPlan& p, const uint32_t* verdict, bool write_files, Write write, uint32_t* status) const {
    const size_t cnt = count(k);
    if (cnt == 0) return 0;
    const size_t* rows = rows_of(k);
    const uint64_t* sb = pairs_of(k);
    std::vector<uint32_t> v(cnt), st(cnt);
    for (size_t j = 0; j < cnt; ++j) v[j] = verdict[rows[j]];
    if (p.keeps_nodes) {
      if (whole) p.mark_proved(sb, v.data(), cnt);
      else p.mark_proved_anchored(sb, levels_of(k), v.data(), cnt);
    }
    p.resolve(sb, v.data(), cnt, st.data());
    if (write_files) {
      std::vector<uint32_t> w = FillPlan::write_mask(st.data(), cnt);
      write(k, w);
      FillPlan::roll_back(sb, w, st.data());
    }
    const size_t set = p.commit(sb, st.data(), cnt);
    for (size_t j = 0; j < cnt; ++j) status[rows[j]] = st[j];
    return set;
  }
};

}  // namespace cp2i
