// The host side of cp2_fills_finish_many (csrc/fill_finish_many.cpp): many fill sessions finished in one pass.  The call is defined by the
// call that exists -- cp2_fill_finish per session -- so the rules are FillPlan::may_finish's (fill_plan.hpp) with the index into `fills`
// in front.  Here: the checks over plain inputs, the tables k_finish_layer_many reads (the session table, the verdict offsets, per level
// the sessions that still have that level with the running sum of their lanes), the turn from a verdict index back to (fills index,
// dataset slot), and the order of what follows the verdicts -- saves, then objects, then hand-over -- as a function over callbacks, so
// that "all or nothing" is checked without a device.  Every step is linear in the sum of the sessions' depths.  No HIP in here:
// tests/host_check/fill_finish_many_check.cpp walks it on the CPU, under AddressSanitizer + UBSan, and tests/fill_finish_many_models.py
// restates it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fill_many_plan.hpp"

namespace cp2i {

// a session as the checks and the tables take it: plan == nullptr is a NULL entry of `fills`
struct FillFinishIn {
  const FillPlan* plan = nullptr;
  bool same_ctx = true;                  // the session belongs to the call's context
  uint64_t tree = 0, slot_roots = 0;     // device addresses of its compact buffer and its stated roots
};

// which entry of `fills` broke a rule, and the text
struct FillFinishRefusal {
  size_t index = 0;
  std::string text;
};

// Every rule of the call, before any device or file work: per entry NULL, another context, finished; then an entry listed twice; then
// per entry a block that is absent, in may_finish's words.  false with the first refusal in that order.
inline bool fill_finish_check(const void* const* fills, const FillFinishIn* in, size_t n_fills, FillFinishRefusal* why) {
  const auto refuse = [&](size_t k, const std::string& what) {
    *why = {k, "fills: fills[" + std::to_string(k) + "]" + what};
    return false;
  };
  std::string err;
  for (size_t k = 0; k < n_fills; ++k) {
    if (!in[k].plan) return refuse(k, " is NULL");
    if (!in[k].same_ctx) return refuse(k, " belongs to another context");
    if (in[k].plan->finished) {
      (void)in[k].plan->may_finish(&err);
      return refuse(k, ": " + err);
    }
  }
  const size_t twice = fill_many_listed_twice(fills, n_fills);
  if (twice < n_fills) return refuse(twice, " is listed twice: one session is finished once");
  for (size_t k = 0; k < n_fills; ++k)
    if (!in[k].plan->may_finish(&err)) return refuse(k, ": " + err);
  return true;
}

// What the device reads.  table: one descriptor per session (layer_tab 0: the kernel derives every row from n_blocks and n_local).
// voff: n_fills + 1 entries, the prefix sum of n_local: verdict voff[k] + s belongs to local slot s of fills[k].  Level l: the sessions
// with depth > l, in `fills` order, are entries [level_off[l], level_off[l] + level_cnt[l]) of sess_of (the index into fills) and of
// prefix (the running sum of n_local * csizes[l + 1], this session's included); level_work[l] is the last prefix, the lanes of the launch.
struct FillFinishPlan {
  std::vector<FillManyDesc> table;
  std::vector<uint64_t> voff, prefix;
  std::vector<uint32_t> sess_of;
  std::vector<uint64_t> level_off, level_cnt, level_work;
  uint64_t rows_built = 0;               // rows above layer 0, all sessions: the lanes of all launches
  size_t launches = 0;                   // levels with work

  size_t n_fills() const { return table.size(); }
  size_t n_levels() const { return level_off.size(); }
  uint64_t n_verdicts() const { return voff.empty() ? 0 : voff.back(); }

  void tables(const FillFinishIn* in, size_t n) {
    table.resize(n);
    voff.assign(n + 1, 0);
    prefix.clear(); sess_of.clear(); level_off.clear(); level_cnt.clear(); level_work.clear();
    rows_built = 0; launches = 0;
    std::vector<uint32_t> active;        // the sessions that still have the level, shrinking: the loops below are linear in the depths' sum
    for (size_t k = 0; k < n; ++k) {
      const FillPlan& p = *in[k].plan;
      table[k] = {in[k].tree, (uint64_t)p.rows, in[k].slot_roots, p.n_local, 0, p.n_blocks, (uint32_t)p.depth(), 0};
      voff[k + 1] = voff[k] + p.n_local;
      if (p.depth() > 0) active.push_back((uint32_t)k);
    }
    for (size_t l = 0; !active.empty(); ++l) {
      level_off.push_back(prefix.size());
      uint64_t sum = 0;
      size_t kept = 0;
      for (const uint32_t k : active) {
        const FillPlan& p = *in[k].plan;
        sum += p.n_local * (uint64_t)p.csizes[l + 1];
        prefix.push_back(sum);
        sess_of.push_back(k);
        if (p.depth() > l + 1) active[kept++] = k;
      }
      active.resize(kept);
      level_cnt.push_back(prefix.size() - level_off.back());
      level_work.push_back(sum);
      rows_built += sum;
      launches += sum != 0;
    }
  }

  // the kernel's search, as the host runs it: the entry of lane t < level_work[l] among the level's cnt entries, in `trips` steps whatever t is
  static uint32_t trips(uint64_t cnt) {
    uint32_t s = 0;
    while (s < 63 && ((uint64_t)1 << s) < cnt) ++s;
    return s;
  }
  // lane t of level l: which session, which local slot, which node of layer l + 1, and the rows it reads from and writes
  struct Lane {
    uint32_t session = 0;
    uint64_t slot = 0, node = 0, src = 0, dst = 0;
    bool pair = false, last = false;
  };
  Lane lane(size_t l, uint64_t t) const {
    const uint64_t* pre = prefix.data() + level_off[l];
    const uint64_t cnt = level_cnt[l];
    uint32_t lo = 0;
    for (uint32_t s = trips(cnt); s-- > 0;) {
      const uint64_t mid = (uint64_t)lo + ((uint64_t)1 << s);
      if (mid < cnt && pre[mid - 1] <= t) lo = (uint32_t)mid;
    }
    const uint64_t j = t - (lo ? pre[lo - 1] : 0);
    Lane r;
    r.session = sess_of[level_off[l] + lo];
    const FillManyDesc& d = table[r.session];
    uint64_t off = 0;
    for (size_t i = 0; i < l; ++i) off += ((d.n_blocks - 1) >> i) + 1;
    off *= d.n_local;
    const uint64_t m_in = ((d.n_blocks - 1) >> l) + 1, m_out = (m_in + 1) / 2;
    r.slot = j / m_out;
    r.node = j - r.slot * m_out;
    r.src = off + r.slot * m_in + 2 * r.node;
    r.dst = off + d.n_local * m_in + r.slot * m_out + r.node;
    r.pair = 2 * r.node + 1 < m_in;
    r.last = l + 1 == d.depth;
    return r;
  }

  // verdict index v < n_verdicts() back to (index into fills, local slot): the last k with voff[k] <= v (sessions always have slots)
  void where(uint64_t v, size_t* k, uint64_t* local) const {
    const size_t at = (size_t)(std::upper_bound(voff.begin(), voff.end(), v) - voff.begin()) - 1;
    *k = at;
    *local = v - voff[at];
  }
  // the first non-zero verdict in order, which is the first fills[k] in order and its lowest slot; false when all are 0
  bool first_mismatch(const uint32_t* verdict, const FillFinishIn* in, FillFinishRefusal* why) const {
    for (uint64_t v = 0; v < n_verdicts(); ++v)
      if (verdict[v] != 0) {
        size_t k = 0;
        uint64_t local = 0;
        where(v, &k, &local);
        *why = {k, "fills: fills[" + std::to_string(k) + "]: fill: the tree over the kept block roots of slot " +
                       std::to_string(in[k].plan->first_slot + local) + " does not end in the stated slot root"};
        return true;
      }
    return false;
  }
};

// What follows clean verdicts, in the order that keeps the call all or nothing: the kept forms of the sessions that have a path, serially
// in `fills` order, the first failing save ending the call with its status (kept files of earlier k stay: valid caches of complete
// sessions); then the n objects, a failed allocation ending it with alloc_failed; only then the n hand-overs, which cannot fail.
// save(k) -> status (0: written), make(k) -> bool, hand_over(k).  *saved counts the kept forms written.
template <class HasPath, class Save, class Make, class HandOver>
inline int fill_finish_commit(size_t n_fills, HasPath has_path, Save save, Make make, HandOver hand_over, int alloc_failed, size_t* saved) {
  *saved = 0;
  for (size_t k = 0; k < n_fills; ++k) {
    if (!has_path(k)) continue;
    const int st = save(k);
    if (st != 0) return st;
    ++*saved;
  }
  for (size_t k = 0; k < n_fills; ++k)
    if (!make(k)) return alloc_failed;
  for (size_t k = 0; k < n_fills; ++k) hand_over(k);
  return 0;
}

}  // namespace cp2i
