// The host side of cp2_fill_adopt (csrc/fill.cpp): which blocks of the slot files are read, the flag byte per row of the compact layout
// that travels to the device, a host model of what k_adopt_layer and k_adopt_resolve make of those bytes, and how the bytes that come back
// change the session (FillPlan: known rows, presence).  No HIP in here: tests/host_check/adopt_plan_check.cpp walks it over random
// geometries, known sets, candidate sets and corruptions on the CPU, under AddressSanitizer + UBSan.
//
// The rule.  A row is DEFINED when the session knows it or a value was computed for it; its value is the kept one where it is known, the
// computed one otherwise.  A node above layer 0 gets a computed value when all its children are defined (two, or one for the last node of
// an odd layer and for the one-block slot, which take a zero sibling and key + 2).  A known node whose computed value equals its kept
// value MATCHES; the top row is always known, its kept value is the stated slot root.  A row that is not known and has a computed value is
// PROVED when the first known node on its way up matches and every row between has a computed value: the computed value of that node was
// made from this row's, so by the collision argument every walk rests on, this row's value is the authentic one.  A block is ADOPTED when
// its layer-0 row is proved, or is known and its candidate equals the kept row.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fill_plan.hpp"

namespace cp2i {

// the bits of a flag byte: the values of cp2k::ADOPT_* (kernels.hpp)
constexpr uint8_t ADOPT_F_KNOWN = 1, ADOPT_F_CAND = 2, ADOPT_F_MATCH = 4, ADOPT_F_PROVED = 8, ADOPT_F_ADOPTED = 16;

inline bool adopt_bit(const std::vector<uint64_t>& bits, uint64_t g) { return (bits[(size_t)(g >> 6)] >> (g & 63)) & 1; }
inline void adopt_set_bit(std::vector<uint64_t>* bits, uint64_t g, bool on) {
  uint64_t& w = (*bits)[(size_t)(g >> 6)];
  w = on ? w | (1ULL << (g & 63)) : w & ~(1ULL << (g & 63));
}

// ---- what is read ------------------------------------------------------------------------------------------------------------------
// The blocks of local slots [s0, s0 + ns) that are absent and that their file covers completely, as a bitmap over local x n_blocks +
// block (fill_read_plan's input).  whole_blocks[i]: how many whole blocks the file of local slot s0 + i holds (0: no file).
inline std::vector<uint64_t> adopt_read_bits(const FillPlan& p, uint64_t s0, uint64_t ns, const std::vector<uint64_t>& whole_blocks) {
  std::vector<uint64_t> want(p.bits.size(), 0);
  for (uint64_t i = 0; i < ns; ++i)
    for (uint64_t b = 0; b < p.n_blocks && b < whole_blocks[(size_t)i]; ++b)
      if (!p.present(s0 + i, b)) adopt_set_bit(&want, (s0 + i) * p.n_blocks + b, true);
  return want;
}

// A read refreshes what is remembered of the selected slots: exactly the blocks just read hold a candidate there, other slots keep theirs.
inline void adopt_remember(const FillPlan& p, uint64_t s0, uint64_t ns, const std::vector<uint64_t>& read_bits, std::vector<uint64_t>* have) {
  have->resize(p.bits.size(), 0);
  for (uint64_t g = s0 * p.n_blocks; g < (s0 + ns) * p.n_blocks; ++g) adopt_set_bit(have, g, adopt_bit(read_bits, g));
}

// ---- what the device reads -------------------------------------------------------------------------------------------------------------
// One byte per row of the compact layout: ADOPT_F_KNOWN where the session knows the row and on every top row, ADOPT_F_CAND on the layer-0
// rows of the selected slots whose block is remembered and still absent.  A remembered block that has become present is forgotten here.
inline std::vector<uint8_t> adopt_flags(const FillPlan& p, uint64_t s0, uint64_t ns, std::vector<uint64_t>* have, uint64_t* n_cand) {
  std::vector<uint8_t> f(p.rows, 0);
  for (uint64_t r = 0; r < p.rows; ++r)
    if (p.is_known(r)) f[(size_t)r] = ADOPT_F_KNOWN;
  for (uint64_t s = 0; s < p.n_local; ++s) f[(size_t)p.node_row(p.depth(), s, 0)] |= ADOPT_F_KNOWN;
  have->resize(p.bits.size(), 0);
  uint64_t n = 0;
  for (uint64_t g = 0; g < p.total(); ++g) {
    if (!adopt_bit(*have, g)) continue;
    if (adopt_bit(p.bits, g)) { adopt_set_bit(have, g, false); continue; }
    const uint64_t s = g / p.n_blocks;
    if (s < s0 || s - s0 >= ns) continue;
    f[(size_t)p.node_row(0, s, g % p.n_blocks)] |= ADOPT_F_CAND;
    ++n;
  }
  *n_cand = n;
  return f;
}

// ---- the model of the two kernels --------------------------------------------------------------------------------------------------------
// k_adopt_layer over every layer: `kept` and `cand` hold one value per row, `roots` one per local slot; compress(left, right, key) with
// key = (layer 0 ? 1 : 0) + (single child ? 2 : 0) and `zero` for the missing sibling.  Writes rows of `cand` and bytes of `flags` above
// layer 0 of the selected slots, nothing else.
template <class V, class Compress>
void adopt_model_layers(const FillPlan& p, uint64_t s0, uint64_t ns, const std::vector<V>& kept, const std::vector<V>& roots, const V& zero,
                        std::vector<V>* cand, std::vector<uint8_t>* flags, Compress compress) {
  const uint8_t defined = ADOPT_F_KNOWN | ADOPT_F_CAND;
  for (size_t l = 0; l < p.depth(); ++l)
    for (uint64_t s = s0; s < s0 + ns; ++s)
      for (uint64_t j = 0; j < p.csizes[l + 1]; ++j) {
        const uint64_t rl = p.node_row(l, s, 2 * j), rp = p.node_row(l + 1, s, j);
        const bool pair = 2 * j + 1 < p.csizes[l];
        const uint8_t fl = (*flags)[(size_t)rl], fr = pair ? (*flags)[(size_t)rl + 1] : ADOPT_F_KNOWN;
        uint8_t& fp = (*flags)[(size_t)rp];
        fp &= ADOPT_F_KNOWN;
        if (!(fl & defined) || !(fr & defined)) continue;
        const V& left = (fl & ADOPT_F_KNOWN) ? kept[(size_t)rl] : (*cand)[(size_t)rl];
        const V& right = !pair ? zero : (fr & ADOPT_F_KNOWN) ? kept[(size_t)rl + 1] : (*cand)[(size_t)rl + 1];
        const V v = compress(left, right, (uint32_t)((l == 0 ? 1 : 0) + (pair ? 0 : 2)));
        (*cand)[(size_t)rp] = v;
        const bool top = l + 1 == p.depth();
        if (fp && v == (top ? roots[(size_t)s] : kept[(size_t)rp])) fp |= ADOPT_F_MATCH;
        fp |= ADOPT_F_CAND;
      }
}

// k_adopt_resolve: the byte per row below the top that comes back (rows of other slots and the top rows: 0).  Changes nothing.
template <class V>
std::vector<uint8_t> adopt_model_resolve(const FillPlan& p, uint64_t s0, uint64_t ns, const std::vector<V>& kept, const std::vector<V>& cand,
                                         const std::vector<uint8_t>& flags) {
  std::vector<uint8_t> out(p.rows, 0);
  for (size_t l = 0; l < p.depth(); ++l)
    for (uint64_t s = s0; s < s0 + ns; ++s)
      for (uint64_t k = 0; k < p.csizes[l]; ++k) {
        const uint64_t r = p.node_row(l, s, k);
        uint8_t f = flags[(size_t)r] & (ADOPT_F_KNOWN | ADOPT_F_CAND | ADOPT_F_MATCH);
        if (!(f & ADOPT_F_CAND)) { out[(size_t)r] = f; continue; }
        if (f & ADOPT_F_KNOWN) {
          if (l == 0) f = (uint8_t)((f & ~ADOPT_F_MATCH) | (cand[(size_t)r] == kept[(size_t)r] ? ADOPT_F_MATCH | ADOPT_F_ADOPTED : 0));
          out[(size_t)r] = f;
          continue;
        }
        bool proved = false;
        uint64_t idx = k;
        for (size_t up = l + 1; up <= p.depth(); ++up) {
          idx >>= 1;
          const uint8_t fa = flags[(size_t)p.node_row(up, s, idx)];
          if (!(fa & ADOPT_F_CAND)) break;
          if (fa & ADOPT_F_KNOWN) { proved = (fa & ADOPT_F_MATCH) != 0; break; }
        }
        if (proved) f |= ADOPT_F_PROVED | (l == 0 ? ADOPT_F_ADOPTED : 0);
        out[(size_t)r] = f;
      }
  return out;
}

// ---- what comes back ---------------------------------------------------------------------------------------------------------------------
struct AdoptVerdict {
  uint64_t rows_proved = 0;
  std::vector<std::vector<uint64_t>> adopted;   // per selected slot: the adopted blocks as local x n_blocks + block, ascending
};
// The proved rows become known at once (they are authentic and stored, whatever happens to the files); the adopted blocks are handed back
// per file and become present only through adopt_commit.  A byte that claims what the bytes sent up rule out -- a proved row that is known
// or is a top row, an adopted block that is present -- is ignored.
inline AdoptVerdict adopt_apply(FillPlan* p, uint64_t s0, uint64_t ns, const std::vector<uint8_t>& out) {
  AdoptVerdict v;
  v.adopted.resize((size_t)ns);
  for (size_t l = 0; l < p->depth(); ++l)
    for (uint64_t s = s0; s < s0 + ns; ++s)
      for (uint64_t k = 0; k < p->csizes[l]; ++k) {
        const uint64_t r = p->node_row(l, s, k);
        const uint8_t f = out[(size_t)r];
        if ((f & ADOPT_F_PROVED) && !p->is_known(r)) {
          p->set_known(r);
          ++v.rows_proved;
        }
        if (l == 0 && (f & ADOPT_F_ADOPTED) && !p->present(s, k)) v.adopted[(size_t)(s - s0)].push_back(s * p->n_blocks + k);
      }
  return v;
}
// the presence bits of one file's adopted blocks, after the file was synced: returns how many were set
inline size_t adopt_commit(FillPlan* p, const std::vector<uint64_t>& global) { return p->set_present(global.data(), global.size()); }

}  // namespace cp2i
