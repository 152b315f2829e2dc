// One function per primitive of csrc/fr_gfx950.hpp and csrc/poseidon2_dev.hpp, on RAW words: limb vectors go in and come
// out exactly as the function under test takes and returns them (no canonical bytes, no to_mont in front).  The same table
// is compiled twice: by fr_unit.hip for gfx950 (one case per lane) and by fr_unit_host.cpp with CP2_HOST_CHECK (128-bit
// shadow accumulator, asserted bounds).  tests/fr_model.py builds the cases and judges the results with big-int arithmetic.
//
// A case is one record of REC 32-bit words in and one of REC words out; words an op does not write are zero.
//   Fe   : 9 words                       Wide : 5 x 64 bits = 10 words, low word first
//   one / two Fe operands                in[0..8], in[9..17]            -> out[0..8]
//   to_wide                              in[0..8]                       -> out[0..9]
//   from_wide, reduce_wide               in[0..9]                       -> out[0..8] / out[0..9]
//   wide_half_round, internal_round_pair xin in[0..8], Y in[10..19], Z in[20..29], index in[30]   -> the same layout
//       (index: the row of P2_RCW_MONT a half round adds, 0..56; the r of a pair, 0..54)
//   external_round<M>, permute           x in[0..8], y in[9..17], z in[18..26], rc_base in[30]    -> the same layout
//   from_words                           in[0..7] -> out[0..8];   to_canonical_words  in[0..8] -> out[0..7]
// The index words select a row of a constant table, so they are clamped to the table here: every input is only data.
#pragma once
#include "../../codex-storage-proofs-circuits_amd/csrc/poseidon2_dev.hpp"

namespace fru {

constexpr int REC = 32;

enum Op : int {
  OP_NORM = 0, OP_NORM_FULL, OP_ADD_LAZY, OP_MUL_MASKED, OP_MUL_UNMASKED, OP_SQR_MASKED, OP_SQR_UNMASKED, OP_SBOX_MASKED,
  OP_SBOX_UNMASKED, OP_TO_WIDE, OP_FROM_WIDE, OP_REDUCE_WIDE, OP_HALF_ROUND, OP_ROUND_PAIR, OP_EXT_UNMASKED, OP_EXT_MASKED,
  OP_FROM_WORDS, OP_TO_MONT, OP_TO_CANONICAL, OP_PERMUTE, N_OPS
};

__device__ __forceinline__ fr::Fe ld_fe(const uint32_t* p) {
  fr::Fe r;
#pragma unroll
  for (int i = 0; i < fr::NL; ++i) r.l[i] = p[i];
  return r;
}
__device__ __forceinline__ void st_fe(uint32_t* p, const fr::Fe& a) {
#pragma unroll
  for (int i = 0; i < fr::NL; ++i) p[i] = a.l[i];
}
__device__ __forceinline__ fr::Wide ld_wide(const uint32_t* p) {
  fr::Wide r;
#pragma unroll
  for (int j = 0; j < fr::NW; ++j) r.w[j] = (uint64_t)p[2 * j] | ((uint64_t)p[2 * j + 1] << 32);
  return r;
}
__device__ __forceinline__ void st_wide(uint32_t* p, const fr::Wide& a) {
#pragma unroll
  for (int j = 0; j < fr::NW; ++j) {
    p[2 * j] = (uint32_t)a.w[j];
    p[2 * j + 1] = (uint32_t)(a.w[j] >> 32);
  }
}

template <int OP>
__device__ __forceinline__ void run(const uint32_t* in, uint32_t* out, const fr::QTab& qtab) {
  using namespace fr;
  uint32_t o[REC];
#pragma unroll
  for (int i = 0; i < REC; ++i) o[i] = 0;
  if constexpr (OP == OP_NORM) st_fe(o, norm(ld_fe(in)));
  else if constexpr (OP == OP_NORM_FULL) st_fe(o, norm_full(ld_fe(in)));
  else if constexpr (OP == OP_ADD_LAZY) st_fe(o, add_lazy(ld_fe(in), ld_fe(in + 9)));
  else if constexpr (OP == OP_MUL_MASKED) st_fe(o, mont_mul<true>(ld_fe(in), ld_fe(in + 9)));
  else if constexpr (OP == OP_MUL_UNMASKED) st_fe(o, mont_mul<false>(ld_fe(in), ld_fe(in + 9)));
  else if constexpr (OP == OP_SQR_MASKED) st_fe(o, mont_sqr<true>(ld_fe(in)));
  else if constexpr (OP == OP_SQR_UNMASKED) st_fe(o, mont_sqr<false>(ld_fe(in)));
  else if constexpr (OP == OP_SBOX_MASKED) st_fe(o, sbox<true>(ld_fe(in)));
  else if constexpr (OP == OP_SBOX_UNMASKED) st_fe(o, sbox<false>(ld_fe(in)));
  else if constexpr (OP == OP_TO_WIDE) st_wide(o, to_wide(ld_fe(in)));
  else if constexpr (OP == OP_FROM_WIDE) st_fe(o, from_wide(ld_wide(in)));
  else if constexpr (OP == OP_REDUCE_WIDE) st_wide(o, reduce_wide(ld_wide(in), qtab));
  else if constexpr (OP == OP_HALF_ROUND || OP == OP_ROUND_PAIR) {
    Fe xin = ld_fe(in);
    Wide Y = ld_wide(in + 10), Z = ld_wide(in + 20);
    if constexpr (OP == OP_HALF_ROUND) {
      const uint32_t row = in[30] < 56u ? in[30] : 56u;
      p2::wide_half_round(xin, Y, Z, P2_RCW_MONT[row]);
    } else {
      const uint32_t r = in[30] < 54u ? in[30] : 54u;
      p2::internal_round_pair(xin, Y, Z, (int)r, qtab);
    }
    st_fe(o, xin);
    st_wide(o + 10, Y);
    st_wide(o + 20, Z);
  } else if constexpr (OP == OP_EXT_UNMASKED || OP == OP_EXT_MASKED || OP == OP_PERMUTE) {
    p2::State s;
    s.x = ld_fe(in);
    s.y = ld_fe(in + 9);
    s.z = ld_fe(in + 18);
    const uint32_t base = in[30] < 77u ? in[30] : 77u;
    if constexpr (OP == OP_EXT_UNMASKED) p2::external_round<false>(s, (int)base);
    else if constexpr (OP == OP_EXT_MASKED) p2::external_round<true>(s, (int)base);
    else p2::permute(s, qtab);
    st_fe(o, s.x);
    st_fe(o + 9, s.y);
    st_fe(o + 18, s.z);
  } else if constexpr (OP == OP_FROM_WORDS) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = in[i];
    st_fe(o, from_words(w));
  } else if constexpr (OP == OP_TO_MONT) st_fe(o, to_mont(ld_fe(in)));
  else if constexpr (OP == OP_TO_CANONICAL) {
    uint32_t w[8];
    to_canonical_words(ld_fe(in), w);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = w[i];
  }
#pragma unroll
  for (int i = 0; i < REC; ++i) out[i] = o[i];
}

}  // namespace fru
