// HIP kernels (gfx950 only) for the Codex storage-proof hot path.  One field element per lane.
//
//   k_permute_batch   a1  Permutation.hs:40-45                       192 algorithmic B / permutation
//   k_hash_cells      a5  blocks/bn254.nim:23-29 (= Slot.hs:222-270 + Sponge.hs:30-43)   cellSize+32 B / cell
//   k_compress_layer  a7  merkle/bn254.nim:24-58 (one tree layer, many trees at once)    96 B / node
//   k_compress_layer_ragged   the same layer for trees of different leaf counts, tree-major, through a prefix table (set_roots_many.cpp)
//   k_finish_layer_many       the same layer for the slot trees of many fill sessions, each in its own layer-major buffer, with the
//                             comparison against the stated roots on each tree's last level (fill_finish_many.cpp)
//   k_sponge2_felts   a3  Sponge.hs:30-43 over field elements (sampling, generic byte strings)
//   k_gen_fake_cells  a10 slot.nim:22-32
//   k_gather_rows         path / cell gather for proof inputs (merkle.nim:21-42 does this on the host; gather_body)
//   k_sample_many, k_gather_addr, k_gen_fake_cells_many   the same across datasets (proof_many.cpp); k_gather_addr over gather_body too
//   k_verify_samples      what SampleAndProve accepts: sample_cells.circom:58-148, single_cell.circom:30-73, merkle.circom:44-114
//   k_scrub_compare       a rebuilt layer against the kept one, mismatch bitmap + per-workgroup counts (scrub.cpp)
//   k_scrub_compare_many  the same with the kept rows of every item behind an address table (many datasets in one batch)
//   k_repair_compare      candidate block roots against the kept rows they would replace, one verdict per request (repair.cpp)
//   k_repair_compare_addr the same with the kept row of every request at an absolute address (read_blocks.cpp: many datasets)
//   k_scatter_rows_addr   a batch's layer written to where every item's dataset keeps it, through an address table (build_many.cpp)
//   k_block_path_roots    a13 candidate block roots walked up their Merkle paths to the slot root, merkle.nim:51-74 (block_proofs.cpp)
//   k_repair_judge_many   the same walk over 0 or depth levels per lane, against a row at an absolute address (repair_many.cpp: many datasets)
//   k_block_path_commit   the same walk; a proved block root is also stored into layer 0 of a fill session's compact buffer (fill.cpp)
//   k_block_path_commit_nodes   the same walk; a proved path's 2 x depth + 1 nodes are stored where the session's tree has them (fill.cpp)
//   k_block_path_commit_anchored   the same walk, stopped per lane at a node the session's tree already holds (fill.cpp)
//   k_block_path_commit_many   the anchored walk with the session taken per lane from a descriptor table (fill_many.cpp)
//   k_block_root_recheck  re-read block roots against layer 0 of a resumed fill session; a row the disk no longer backs is zeroed (fill.cpp)
//   k_block_root_recheck_addr the same with the kept row of every block at an absolute address (fills_resume_many.cpp: many sessions)
//   k_adopt_layer, k_adopt_resolve   the tree over block roots read back from disk, judged against the nodes a fill session keeps (fill.cpp)
//   k_nodes_restore_layer   the kept nodes a checkpoint states, authenticated top-down from the stated slot roots (fill.cpp)
//   k_multiproof_layer    one level of the induced subtrees of many block multiproofs, one host-made job per inner node (multiproofs.cpp)
//   k_multiproof_commit   the rows of the proved groups copied into a fill session's compact buffer (fill.cpp)
//   k_multiproof_tops, k_multiproof_fold   the tops of multiproofs that stop at kept nodes compared with those nodes, one verdict per group (fill.cpp)
//
// All global-memory field elements are 32-byte little-endian canonical integers (the ABI format).
#include "kernels.hpp"

#include <algorithm>
#include <cstdlib>
#include <string>

#include "poseidon2_dev.hpp"

namespace cp2k {
using fr::Fe;
using p2::State;

constexpr int TPB = 256;
// minimum waves per SIMD the register allocator must leave room for (tuning knobs)
#ifndef CP2_PERM_WAVES
#define CP2_PERM_WAVES 1
#endif
#ifndef CP2_HASH_WAVES
#define CP2_HASH_WAVES 3
#endif

__device__ __forceinline__ Fe load_fe_canonical(const uint4* p) {
  uint4 a = p[0], b = p[1];
  uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return fr::to_mont(fr::from_words(w));
}

__device__ __forceinline__ void store_fe_canonical(uint4* p, const Fe& v) {
  uint32_t w[8];
  fr::to_canonical_words(v, w);
  p[0] = make_uint4(w[0], w[1], w[2], w[3]);
  p[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// a 32-byte row as it stands: two 16-byte loads, two 16-byte stores
__device__ __forceinline__ void copy_row(uint4* __restrict__ to, const uint4* from) {
  const uint4 a = from[0], b = from[1];
  to[0] = a;
  to[1] = b;
}

// two 32-byte rows, each held as two loaded uint4, compared byte for byte
__device__ __forceinline__ bool rows_equal(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return ((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) | (a1.w ^ b1.w)) == 0;
}

// nodeKey (Merkle.hs:162-165) in Montgomery form, lane-varying key in {0,1,2,3}: mont(1)*bit0 + mont(2)*bit1
// with and-masks (v_cndmask_b32 costs ~23 cycles on gfx950).  The sum for key 3 is a
// lazy value < 2N with limbs < 2U, inside permute()'s input bounds.
__device__ __forceinline__ Fe key_fe(uint32_t key) {
  const Fe k1 = fr::fe_const(fr::FR_KEY1_MONT), k2 = fr::fe_const(fr::FR_KEY2_MONT);
  const uint32_t m1 = 0u - (key & 1u), m2 = 0u - ((key >> 1) & 1u);
  Fe r;
#pragma unroll
  for (int i = 0; i < fr::NL; ++i) r.l[i] = (k1.l[i] & m1) + (k2.l[i] & m2);
  return r;
}

// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB, CP2_PERM_WAVES) k_permute_batch(const uint4* __restrict__ in, uint4* __restrict__ out, size_t n) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  State s;
  s.x = load_fe_canonical(in + 6 * i);
  s.y = load_fe_canonical(in + 6 * i + 2);
  s.z = load_fe_canonical(in + 6 * i + 4);
  p2::permute(s, qtab);
  store_fe_canonical(out + 6 * i, s.x);
  store_fe_canonical(out + 6 * i + 2, s.y);
  store_fe_canonical(out + 6 * i + 4, s.z);
}

// ------------------------------------------------------------------------------------------------
// One Merkle layer for nseg independent trees: out[seg][j] = compress(in[seg][2j], in[seg][2j+1], key)
// with the odd-tail rule of merkle/bn254.nim:47-53 (compress(last, 0) with key+2).
__global__ void __launch_bounds__(TPB) k_compress_layer(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                          size_t m_in, size_t m_out, size_t nseg, uint32_t bottom,
                                                          size_t in_seg_stride, size_t out_seg_stride) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= m_out * nseg) return;
  size_t seg = t / m_out, j = t - seg * m_out;
  const uint4* src = in + 2 * (seg * in_seg_stride + 2 * j);
  bool pair = (2 * j + 1 < m_in);
  State s;
  s.x = load_fe_canonical(src);
  s.y = pair ? load_fe_canonical(src + 2) : fr::fe_zero();
  s.z = key_fe((bottom ? 1u : 0u) + (pair ? 0u : 2u));
  p2::permute(s, qtab);
  store_fe_canonical(out + 2 * (seg * out_seg_stride + j), s.x);
}

// ------------------------------------------------------------------------------------------------
// The same layer for trees of DIFFERENT leaf counts (set_roots_many.cpp: the dataset trees of many datasets).  The trees lie tree-major in
// `rows`: tree r owns its layers, bottom first, from row tree_tab[2 r], over tree_tab[2 r + 1] leaves (set_roots_plan.hpp).  Level `level`
// of the trees that still have one: lane t belongs to the first of the cnt entries whose prefix (the running sum of the entries' layer
// level + 1 sizes) is > t -- found in `trips` steps whatever t is, 2^trips >= cnt, so a wave's lanes stay together -- and is node
// j = t - (the prefix before it) of tree tree_of[entry].  It reads rows of layer `level` and writes one row of layer level + 1 of the same
// tree: disjoint sets, nothing else is written.  Per node k_compress_layer's rule, unchanged.  LDS is the QTab only; no atomics.
// The register bound names k_compress_layer's 5 waves per SIMD: left alone the allocator settles at 127 VGPRs and 4 waves, with it at
// 73 and no scratch (profiles/set_roots_many_kernel_resources.txt).
__global__ void __launch_bounds__(TPB, 5) k_compress_layer_ragged(uint4* __restrict__ rows, const uint64_t* __restrict__ tree_tab,
                                                                 const uint64_t* __restrict__ prefix, const uint32_t* __restrict__ tree_of,
                                                                 uint32_t cnt, uint32_t trips, uint32_t level, size_t work) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= work) return;
  uint32_t lo = 0;
  for (uint32_t s = trips; s-- > 0;) {
    const uint32_t mid = lo + (1u << s);
    if (mid < cnt && prefix[mid - 1] <= t) lo = mid;
  }
  const size_t j = t - (lo ? prefix[lo - 1] : 0);
  const uint32_t r = tree_of[lo];
  const uint64_t n = tree_tab[2 * (size_t)r + 1];
  uint64_t off = tree_tab[2 * (size_t)r];                      // of layer `level`: the tree's first row + the layers below
  for (uint32_t i = 0; i < level; ++i) off += ((n - 1) >> i) + 1;
  const uint64_t m_in = ((n - 1) >> level) + 1;
  const uint4* src = rows + 2 * (off + 2 * j);
  const bool pair = (2 * j + 1 < m_in);
  State s;
  s.x = load_fe_canonical(src);
  s.y = pair ? load_fe_canonical(src + 2) : fr::fe_zero();
  s.z = key_fe((level == 0 ? 1u : 0u) + (pair ? 0u : 2u));
  p2::permute(s, qtab);
  store_fe_canonical(rows + 2 * (off + m_in + j), s.x);
}

// ------------------------------------------------------------------------------------------------
// The same layer for the slot trees of MANY FILL SESSIONS (fill_finish_many.cpp: cp2_fills_finish_many).  A session's compact buffer is
// layer-major over its n_local slots -- layer l of slot s starts at row coff[l] + s * csizes[l], coff[l + 1] = coff[l] + n_local *
// csizes[l], csizes[0] = n_blocks -- and every session lies in an allocation of its own, so neither kernel above fits: the lane takes its
// session from the FillManySession table (tree, n_rows, slot_roots, n_local, n_blocks, depth; layer_tab is not read, a session that keeps
// no nodes has none).  Level `level` over the sessions with depth > level: entry e of the level's tables is session sess_of[e] with
// n_local * m_out lanes, m_in = csizes[level], m_out = (m_in + 1) / 2; the lane finds its entry as k_compress_layer_ragged does, in `trips`
// uniform steps.  Inside the entry j = t - (the prefix before it), s = j / m_out, node = j - s * m_out; the layer's first row is n_local
// times the sum of the sizes below, in closed form.  The lane reads rows off + s * m_in + 2 node (+ 1) and writes row off + n_local * m_in
// + s * m_out + node: per level disjoint sets.  Per node k_compress_layer's rule, unchanged (a one-block slot is one level with key 3).
//   On its session's LAST level (level + 1 == depth) the lane's row is the slot root: besides storing it, it compares the canonical words
//   with slot_roots[s], byte for byte as k_repair_compare does, and writes verdict[voff[session] + s] = 0 or 1.  Every verdict entry has
//   exactly one such lane, so nothing is cleared beforehand and there are no atomics.
//   Defensive (the host never produces them): a destination row at or past n_rows is neither read for nor stored, and on the last level
//   its verdict is 1 -- the rows of a slot ascend with the level, so a tree that leaves its buffer anywhere ends in a 1 --; a level at or
//   past the session's depth, a session at or past n_sessions and a slot at or past n_local store nothing.
// LDS is the QTab only.  The register bound names k_compress_layer's 5 waves per SIMD, as k_compress_layer_ragged's does
// (profiles/fill_finish_many_kernel_resources.txt: 77 VGPRs, no scratch).  Measured over 4096 sessions x 1 slot x 4096 block roots, all 12
// levels: 1.005 times k_compress_layer layer by layer over the same leaves (profiles/fill_finish_many_rate.txt); the search, the descriptor
// loads and the 64-bit division stay below what a 50 k-instruction permutation shows.
__global__ void __launch_bounds__(TPB, 5) k_finish_layer_many(const FillManySession* __restrict__ sessions, uint64_t n_sessions,
                                                             const uint64_t* __restrict__ voff,
                                                             const uint64_t* __restrict__ prefix, const uint32_t* __restrict__ sess_of,
                                                             uint32_t cnt, uint32_t trips, uint32_t level, size_t work,
                                                             uint32_t* __restrict__ verdict) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= work) return;
  uint32_t lo = 0;
  for (uint32_t s = trips; s-- > 0;) {
    const uint32_t mid = lo + (1u << s);
    if (mid < cnt && prefix[mid - 1] <= t) lo = mid;
  }
  const size_t j = t - (lo ? prefix[lo - 1] : 0);
  const uint32_t k = sess_of[lo];
  if (k >= n_sessions) return;
  const FillManySession* d = sessions + k;
  const uint64_t n = d->n_blocks, n_local = d->n_local;
  const uint32_t depth = d->depth;
  if (level >= depth || n == 0) return;
  uint64_t off = 0;                                            // of layer `level`: n_local x the sizes of the layers below
  for (uint32_t i = 0; i < level; ++i) off += ((n - 1) >> i) + 1;
  off *= n_local;
  const uint64_t m_in = ((n - 1) >> level) + 1, m_out = (m_in + 1) / 2;
  const uint64_t s = j / m_out, node = j - s * m_out;
  if (s >= n_local) return;
  const bool last = level + 1 == depth;
  const uint64_t dst = off + n_local * m_in + s * m_out + node;
  if (dst >= d->n_rows) {                                      // (never: the host sized the buffer by the same rule)
    if (last) verdict[voff[k] + s] = 1u;
    return;
  }
  uint4* rows = reinterpret_cast<uint4*>(d->tree);
  const uint4* src = rows + 2 * (off + s * m_in + 2 * node);
  const bool pair = (2 * node + 1 < m_in);
  State st;
  st.x = load_fe_canonical(src);
  st.y = pair ? load_fe_canonical(src + 2) : fr::fe_zero();
  st.z = key_fe((level == 0 ? 1u : 0u) + (pair ? 0u : 2u));
  p2::permute(st, qtab);
  uint32_t w[8];
  fr::to_canonical_words(st.x, w);
  const uint4 r0 = make_uint4(w[0], w[1], w[2], w[3]), r1 = make_uint4(w[4], w[5], w[6], w[7]);
  rows[2 * dst] = r0;
  rows[2 * dst + 1] = r1;
  if (!last) return;
  const uint4* want = reinterpret_cast<const uint4*>(d->slot_roots) + 2 * s;
  verdict[voff[k] + s] = rows_equal(r0, r1, want[0], want[1]) ? 0u : 1u;
}

// ------------------------------------------------------------------------------------------------
// compress(x, y, key) for n independent pairs (merkle/bn254.nim:18): the seam call `compressWithKey`, batched.
__global__ void __launch_bounds__(TPB) k_compress_pairs(const uint4* __restrict__ xy, uint32_t key, uint4* __restrict__ out, size_t n) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= n) return;
  State s;
  s.x = load_fe_canonical(xy + 4 * t);
  s.y = load_fe_canonical(xy + 4 * t + 2);
  s.z = key_fe(key);
  p2::permute(s, qtab);
  store_fe_canonical(out + 2 * t, s.x);
}

// ------------------------------------------------------------------------------------------------
// Batched rate-2 sponge over field elements (Sponge.hs:30-43): item i hashes felts[i*nf .. i*nf+nf).
__global__ void __launch_bounds__(TPB) k_sponge2_felts(const uint4* __restrict__ felts, size_t nf, size_t nitems,
                                                         uint4* __restrict__ out) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= nitems) return;
  const uint4* src = felts + 2 * t * nf;
  State s;
  s.x = fr::fe_zero();
  s.y = fr::fe_zero();
  s.z = fr::fe_const(fr::FR_CIV_RATE2_MONT);
  const Fe one = fr::fe_const(fr::FR_R1);
  size_t padded = (nf + 2) & ~(size_t)1;   // nf odd: +1 ("1"); nf even: +2 ("1","0")
#pragma unroll 1
  for (size_t k = 0; k < padded; k += 2) {
    Fe a = (k < nf) ? load_fe_canonical(src + 2 * k) : (k == nf ? one : fr::fe_zero());
    Fe b = (k + 1 < nf) ? load_fe_canonical(src + 2 * (k + 1)) : (k + 1 == nf ? one : fr::fe_zero());
    s.x = fr::norm(fr::add_lazy(s.x, a));
    s.y = fr::norm(fr::add_lazy(s.y, b));
    p2::permute(s, qtab);
  }
  store_fe_canonical(out + 2 * t, s.x);
}

// ------------------------------------------------------------------------------------------------
// hashCell for a contiguous array of cells: one cell per lane.
//
// The byte stream a lane absorbs is  cell || 0x01 || 0-pad to 31*nfelts || sponge pad, where the
// sponge's "1" pad element is itself the chunk {0x01,0,...} and the optional "0" element a zero
// chunk (Slot.hs:243-250 then Sponge.hs:36-39).  So the whole padded input is one byte stream cut
// into 31-byte little-endian chunks, two per permutation (62 bytes).
//
// Staging: the stream is fetched in whole 128-byte lines, each exactly once.  Per stage a wave copies one
// line of each of its 64 cells into a per-cell LDS ring: lane-linear dword loads, 32 consecutive lanes read
// one full line (perfectly coalesced), and the ring row stride of 47 dwords is odd, so the per-lane reads
// are bank-conflict free.  The sponge consumes 62 bytes per permutation, the producer adds 128 per stage,
// so at most 60 bytes wait in the ring when the next line lands (what is left is even and below 62): 188 bytes, the ring's size.
// A lane's 17-dword read window (68 bytes for 62) may run a few bytes past the valid data; chunk_pair uses 512 bits of it.  (The first
// version staged 124-byte tiles, which touches most lines twice: FETCH_SIZE showed 2x the algorithmic
// bytes, calibrated with tools/fetch_calib.hip.)
#ifndef CP2_RING_WORDS
#define CP2_RING_WORDS 47
#define CP2_RING_STRIDE 47
#endif
#ifndef CP2_HASH_BT
#define CP2_HASH_BT 256
#endif
// 47 words = 188 bytes per cell: exactly the 60 bytes that can still wait plus the 128 of a new line.  Round 5: with 48 words and a
// row stride of 49 (round 1) a 256-thread workgroup held 54 016 B of LDS and only TWO of them fitted a CU -- SQ_WAVE_CYCLES showed
// 1.94 waves per SIMD where the registers allow 3; at 47 / 47 it holds 51 968 B, three fit, and the kernel is 1.1 % faster
// (tools/ab_hash_kernel.py, profiles/r05_ab_hash_ring.txt).  The stride stays odd: the per-lane reads are bank-conflict free.
constexpr int RING_WORDS = CP2_RING_WORDS;
constexpr int RING_STRIDE = CP2_RING_STRIDE;
constexpr int LINE_WORDS = 32;             // 128 bytes

// two 31-byte chunks from a 17-dword window whose first chunk starts SH bits into w[0] (SH = 0 or 16)
template <int SH>
__device__ __forceinline__ void chunk_pair(const uint32_t (&w)[17], Fe& a, Fe& b) {
#pragma unroll
  for (int i = 0; i < fr::NL; ++i) {
    const int width = (i == fr::NL - 1) ? 16 : 29;
    {
      const int bit = SH + 29 * i, k = bit / 32, sh = bit % 32;
      uint32_t v = w[k] >> sh;
      if (sh + width > 32) v |= w[k + 1] << (32 - sh);
      a.l[i] = v & ((1u << width) - 1);
    }
    {
      const int bit = SH + 248 + 29 * i, k = bit / 32, sh = bit % 32;
      uint32_t v = w[k] >> sh;
      if (sh + width > 32) v |= w[k + 1] << (32 - sh);
      b.l[i] = v & ((1u << width) - 1);
    }
  }
}

// LDS allows three workgroups per CU = three waves per SIMD: tell the register allocator that is also the MOST it will
// ever get, so that it uses the registers (up to 168) instead of squeezing the staging loops for an occupancy it cannot have
//
// BT = threads per workgroup: 256 (four waves share one reduction table: 51 968 B of LDS with the 47-word ring, three workgroups
// per CU -- two when a launch leaves room; what the product launches) or 64 (one wave per workgroup: 16 384 B, ten per CU; kept for tools/hash_block_sweep.cpp, which showed
// that the workgroup shape does not matter below 256 MiB and that 64 lanes lose above: profiles/r03_hash_block_sweep.txt).
template <int BT>
__global__ void __launch_bounds__(BT, CP2_HASH_WAVES) __attribute__((amdgpu_waves_per_eu(CP2_HASH_WAVES, CP2_HASH_WAVES))) k_hash_cells(const uint8_t* __restrict__ cells, size_t cell_size,
                                                                      size_t n_cells, uint4* __restrict__ out) {
  __shared__ fr::QTab qtab;
  __shared__ uint32_t ring[BT / 64][64 * RING_STRIDE];
  fr::qtab_fill(qtab, threadIdx.x, BT);

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t cell0 = (size_t)blockIdx.x * BT + (size_t)wave * 64;
  const size_t my_cell = cell0 + lane;
  const size_t nfelts = (cell_size + 31) / 31;            // chunks of cell || 0x01
  const size_t total = (nfelts + 2) & ~(size_t)1;          // + sponge pad, even
  const size_t sponge_pad_pos = 31 * nfelts;               // byte position of the sponge's "1"
  const size_t stream_len = 31 * total;                    // multiple of 62
  const size_t nlines = (stream_len + 127) / 128;
  const bool aligned4 = ((cell_size & 3) == 0) && ((reinterpret_cast<uintptr_t>(cells) & 3) == 0);

  State s;
  s.x = fr::fe_zero();
  s.y = fr::fe_zero();
  s.z = fr::fe_const(fr::FR_CIV_RATE2_MONT);

  uint32_t* my_ring = ring[wave];
  const uint32_t* my_row = my_ring + lane * RING_STRIDE;
  size_t cons = 0;                                          // bytes absorbed so far (wave-uniform)
#pragma unroll 1
  for (size_t line = 0; line < nlines; ++line) {
    __syncthreads();   // every lane is done reading what this stage overwrites (and, first pass, the qtab fill)
    const int ring_base = (int)((line * LINE_WORDS) % RING_WORDS);
    // Word w of line `line` of 32 cells per lane: lane = (cell parity, w), cell = cell0 + 2k + (lane >> 5) for k = 0..31.
    // Everything but the cell is the same for all 32 loads of a lane, so it is worked out once per line: the byte offset
    // p0, whether the dword lies inside the cell, the padding bit it may carry, its slot in the ring.
    {
      const int w = lane & 31, half = lane >> 5;
      const size_t p0 = line * 128 + (size_t)w * 4;
      const uint32_t padmask = (sponge_pad_pos >= p0 && sponge_pad_pos < p0 + 4) ? 1u << (8 * (sponge_pad_pos - p0)) : 0u;
      int slot = ring_base + w;
      if (slot >= RING_WORDS) slot -= RING_WORDS;
      uint32_t* dst = my_ring + half * RING_STRIDE + slot;                     // + 2 * RING_STRIDE per k
      const size_t first = cell0 + (size_t)half;
      const int kmax = first < n_cells ? (int)((n_cells - first + 1) / 2 < 32 ? (n_cells - first + 1) / 2 : 32) : 0;   // cells that exist
      const uint8_t* ptr = cells + first * cell_size + p0;
      const size_t step = 2 * cell_size;
      if (aligned4 && p0 + 4 <= cell_size) {            // a whole dword of cell data: the common case
#pragma unroll 8
        for (int k = 0; k < LINE_WORDS; ++k) {
          uint32_t val = padmask;
          if (k < kmax) val |= *reinterpret_cast<const uint32_t*>(ptr);
          dst[k * 2 * RING_STRIDE] = val;
          ptr += step;
        }
      } else if (p0 <= cell_size) {                      // the dword straddles the end of the cell (or cells are not 4-byte aligned)
#pragma unroll 1
        for (int k = 0; k < LINE_WORDS; ++k) {
          uint32_t val = padmask;
          if (k < kmax) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const size_t p = p0 + b;
              const uint32_t byte = (p < cell_size) ? ptr[b] : (p == cell_size ? 1u : 0u);   // 0x01 ends the data (Slot.hs:243-250)
              val |= byte << (8 * b);
            }
          }
          dst[k * 2 * RING_STRIDE] = val;
          ptr += step;
        }
      } else {                                           // past the data: zero padding, possibly the sponge's own "1"
#pragma unroll 8
        for (int k = 0; k < LINE_WORDS; ++k) dst[k * 2 * RING_STRIDE] = padmask;
      }
    }
    __syncthreads();
    const size_t avail = (line + 1) * 128 < stream_len ? (line + 1) * 128 : stream_len;
#pragma unroll 1
    while (cons + 62 <= avail) {
      const int off = (int)(cons % (RING_WORDS * 4));
      int d = off >> 2;
      uint32_t w[17];
#pragma unroll
      for (int j = 0; j < 17; ++j) {
        w[j] = my_row[d];
        d = (d + 1 == RING_WORDS) ? 0 : d + 1;
      }
      Fe a, b;
      if (off & 2) chunk_pair<16>(w, a, b);
      else chunk_pair<0>(w, a, b);
      a = fr::to_mont(a);
      b = fr::to_mont(b);
      s.x = fr::norm(fr::add_lazy(s.x, a));
      s.y = fr::norm(fr::add_lazy(s.y, b));
      p2::permute(s, qtab);
      cons += 62;
    }
  }
  if (my_cell < n_cells) store_fe_canonical(out + 2 * my_cell, s.x);
}

// ------------------------------------------------------------------------------------------------
// genFakeCell (slot.nim:22-32): sequential in a cell, independent across cells; one cell per lane.
// Thread t makes "global cell" g = list ? list[t] : first + t.  With cells_per_slot != 0 the global
// index spans several slots: slot = g / cells_per_slot uses seed0 + 1001*slot (dataset.nim:32, seed0
// already holding the "+72" of the first slot) and the cell index inside the slot is g % cells_per_slot.
// Slots cut into units (units_per_slot > 1: a slot's cells spread over several devices, `cells_per_slot` then counts
// the cells of ONE unit): unit = first_unit + g / cells_per_slot, slot = unit / units_per_slot (seed0 = the seed of
// slot 0 of the dataset) and the cell index inside the slot is (unit % units_per_slot) * cells_per_slot + g % cells_per_slot.
__global__ void __launch_bounds__(TPB) k_gen_fake_cells(uint64_t seed0, uint64_t cells_per_slot, uint64_t first,
                                                          const uint64_t* __restrict__ list, size_t n_cells,
                                                          size_t cell_size, uint8_t* __restrict__ out,
                                                          uint64_t units_per_slot, uint64_t first_unit) {
  __shared__ uint4 gen_stage[TPB / 64][64 * 9];
  size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  const bool active = t < n_cells;
  if (!active && ((cell_size & 127) != 0 || (reinterpret_cast<uintptr_t>(out) & 15) != 0)) return;
  const uint64_t g = active ? (list ? list[t] : first + t) : 0;   // idle tail lanes only take part in the write-out
  uint64_t slot = cells_per_slot ? g / cells_per_slot : 0;
  uint64_t idx = cells_per_slot ? g - slot * cells_per_slot : g;
  if (units_per_slot > 1) {          // `slot` so far is the unit's index inside this batch
    const uint64_t unit = first_unit + slot;
    slot = unit / units_per_slot;
    idx += (unit - slot * units_per_slot) * cells_per_slot;
  }
  const uint64_t seed1 = (seed0 + 1001 * slot) + 0xdeadcafeULL;
  const uint64_t seed2 = idx + 0x98765432ULL;
  uint64_t state = 1;
  uint8_t* dst = out + t * cell_size;
  const bool wide = ((cell_size & 127) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  if (wide) {
    // Each lane makes 128 bytes of its cell, parks them in LDS, then the wave writes them out so that 8
    // consecutive lanes store one cell's full 128-byte line (a lane storing 16 bytes at a 2 KiB stride made
    // WRITE_SIZE 2.7x the data: partial-line writes).
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint4* my = gen_stage[wave];
    const size_t wave_cell0 = (size_t)blockIdx.x * TPB + (size_t)wave * 64;
#pragma unroll 1
    for (size_t i = 0; i < cell_size; i += 128) {
#pragma unroll 1
      for (int piece = 0; piece < 8; ++piece) {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          state = state * (state + seed1) * (state + seed2) + state * (state ^ 0x5a5a5a5aULL) + seed1 * state + (seed2 + 17);
          state = state % 1698428844001831ULL;
          w[b >> 2] |= (uint32_t)(state & 0xff) << (8 * (b & 3));
        }
        my[lane * 9 + piece] = make_uint4(w[0], w[1], w[2], w[3]);   // row stride 9 x 16 B: conflict-free both ways
      }
      // wave-private region: order this wave's LDS writes before its cross-lane reads (no instructions on wave64,
      // but the compiler may not move the reads up)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = k * 8 + (lane >> 3), piece = lane & 7;
        const size_t cell = wave_cell0 + c;
        uint4 v = my[c * 9 + piece];
        if (cell < n_cells) *reinterpret_cast<uint4*>(out + cell * cell_size + i + 16 * piece) = v;
      }
      // ... and the next round's writes after these reads
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    return;
  }
#pragma unroll 1
  for (size_t i = 0; i < cell_size; ++i) {
    state = state * (state + seed1) * (state + seed2) + state * (state ^ 0x5a5a5a5aULL) + seed1 * state + (seed2 + 17);
    state = state % 1698428844001831ULL;
    dst[i] = (uint8_t)state;
  }
}

// ------------------------------------------------------------------------------------------------
// cellIndex (sample/bn254.nim:16-24) + merged, padded path rows (merkle.nim:21-42,86-100; types.nim:27-37) for
// one (slot, counter) pair per lane.  The sponge input [entropy, slotRoot, counter] pads to 4 elements with the
// "1" (Sponge.hs:36-39): two permutations.
__global__ void __launch_bounds__(TPB) k_sample_paths(TreeGeom g, const uint4* __restrict__ nodes, const uint4* __restrict__ entropy,
                                                        const uint64_t* __restrict__ slots, uint64_t slot0, size_t n_items,
                                                        uint32_t ns, uint32_t md, uint64_t* __restrict__ indices,
                                                        uint64_t* __restrict__ gcell, uint64_t* __restrict__ rows) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= n_items * ns) return;
  const size_t item = t / ns;
  const uint32_t counter = (uint32_t)(t - item * ns) + 1;            // sample/bn254.nim:27
  const uint64_t slot = slots ? slots[item] : slot0 + item;
  State s;
  s.x = load_fe_canonical(entropy);
  s.y = load_fe_canonical(nodes + 2 * (g.toff[g.nt - 1] + slot));  // treeRoot(bigTree)
  s.z = fr::fe_const(fr::FR_CIV_RATE2_MONT);
  p2::permute(s, qtab);
  Fe c = fr::fe_zero();
  c.l[0] = counter & fr::MASK;
  c.l[1] = counter >> 29;
  s.x = fr::norm(fr::add_lazy(s.x, fr::to_mont(c)));
  s.y = fr::norm(fr::add_lazy(s.y, fr::fe_const(fr::FR_R1)));
  p2::permute(s, qtab);
  uint32_t w[8];
  fr::to_canonical_words(s.x, w);
  const uint64_t cell = (((uint64_t)w[1] << 32) | w[0]) & (g.n_cells - 1);   // extractLowBits, types/bn254.nim:47-59
  indices[t] = cell;
  gcell[t] = slot * g.n_cells + cell;
  uint64_t* r = rows + t * md;
  uint32_t d = 0;
  const uint64_t b = cell / g.cpb;
  uint64_t j = cell - b * g.cpb, m = g.cpb;
  for (uint32_t k = 0; k + 1 < g.nb && d < md; ++k, ++d) {           // bottom proof inside the block tree
    const uint64_t sib = j ^ 1;
    r[d] = (sib < m) ? g.boff[k] + (slot * g.nblocks + b) * g.bsz[k] + sib : ~0ULL;
    j >>= 1;
    m = (m + 1) >> 1;
  }
  j = b;
  m = g.nblocks;
  for (uint32_t k = 0; k + 1 < g.nt && d < md; ++k, ++d) {           // top proof inside the slot's big tree
    const uint64_t sib = j ^ 1;
    r[d] = (sib < m) ? g.toff[k] + slot * g.tsz[k] + sib : ~0ULL;
    j >>= 1;
    m = (m + 1) >> 1;
  }
  for (; d < md; ++d) r[d] = ~0ULL;                                   // padMerkleProof
}

// ------------------------------------------------------------------------------------------------
// Gather nrows rows of row_bytes bytes in words of W, shared by k_gather_rows and k_gather_addr: out row r = the row at src_of(r), zeros
// where that is null (the reference pads paths with zero, merkle.nim:33-34, types.nim:27-37).  Grid-stride over the words.
template <typename W, typename Src>
__device__ __forceinline__ void gather_body(size_t nrows, size_t row_bytes, uint8_t* __restrict__ out, Src src_of) {
  const size_t words_per_row = row_bytes / sizeof(W);
  size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * TPB;
  for (; t < nrows * words_per_row; t += stride) {
    const size_t r = t / words_per_row, w = t - r * words_per_row;
    const W* from = reinterpret_cast<const W*>(src_of(r));
    W v = 0;
    if (from) v = from[w];
    reinterpret_cast<W*>(out + r * row_bytes)[w] = v;
  }
}

// Row index[r] of src; ~0 is none.
__global__ void __launch_bounds__(TPB) k_gather_rows(const uint8_t* __restrict__ src, const uint64_t* __restrict__ index,
                                                       size_t nrows, size_t row_bytes, uint8_t* __restrict__ out) {
  gather_body<uint32_t>(nrows, row_bytes, out, [=](size_t r) -> const uint8_t* {
    const uint64_t idx = index[r];
    return idx != ~0ULL ? src + idx * row_bytes : nullptr;
  });
}

// ------------------------------------------------------------------------------------------------
// Proof inputs across datasets (proof_many.cpp).  k_sample_many is k_sample_paths with the per-request inputs -- entropy, slot root,
// slot geometry, node buffer -- read from a descriptor instead of kernel arguments, and ABSOLUTE node addresses written instead of
// row indices, so that one launch serves the requests of every dataset and one k_gather_addr launch fetches all their paths.
__global__ void __launch_bounds__(TPB) k_sample_many(const ManyReq* __restrict__ reqs, const TreeGeom* __restrict__ geoms, size_t n_req,
                                                       uint32_t ns, uint32_t md, uint64_t* __restrict__ indices,
                                                       uint64_t* __restrict__ blocks, uint64_t* __restrict__ addr) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t total = n_req * ns;
  size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= total) return;
  const size_t item = t / ns;
  const uint32_t counter = (uint32_t)(t - item * ns) + 1;            // sample/bn254.nim:27
  const ManyReq& q = reqs[item];
  State s;
  s.x = load_fe_canonical(reinterpret_cast<const uint4*>(q.entropy));
  s.y = load_fe_canonical(reinterpret_cast<const uint4*>(q.slot_root));
  s.z = fr::fe_const(fr::FR_CIV_RATE2_MONT);
  p2::permute(s, qtab);
  Fe c = fr::fe_zero();
  c.l[0] = counter & fr::MASK;
  c.l[1] = counter >> 29;
  s.x = fr::norm(fr::add_lazy(s.x, fr::to_mont(c)));
  s.y = fr::norm(fr::add_lazy(s.y, fr::fe_const(fr::FR_R1)));
  p2::permute(s, qtab);
  uint32_t w[8];
  fr::to_canonical_words(s.x, w);
  const uint64_t cell = (((uint64_t)w[1] << 32) | w[0]) & (q.n_cells - 1);   // extractLowBits, types/bn254.nim:47-59
  indices[t] = cell;
  const uint64_t b = cell / q.cpb;
  if (!q.nodes) {                                                     // compact: the host rebuilds the touched block
    blocks[t] = b;
    return;
  }
  const TreeGeom& g = geoms[q.geom];
  const uint64_t base = q.nodes, slot = q.slot;
  addr[total * md + t] = base + (slot * g.n_cells + cell) * 32;      // the leaf: layer 0 row slot * nCells + cell
  uint64_t* r = addr + t * md;
  uint32_t d = 0;
  uint64_t j = cell - b * g.cpb, m = g.cpb;
  for (uint32_t k = 0; k + 1 < g.nb && d < md; ++k, ++d) {           // bottom proof inside the block tree
    const uint64_t sib = j ^ 1;
    r[d] = (sib < m) ? base + (g.boff[k] + (slot * g.nblocks + b) * g.bsz[k] + sib) * 32 : 0;
    j >>= 1;
    m = (m + 1) >> 1;
  }
  j = b;
  m = g.nblocks;
  for (uint32_t k = 0; k + 1 < g.nt && d < md; ++k, ++d) {           // top proof inside the slot's big tree
    const uint64_t sib = j ^ 1;
    r[d] = (sib < m) ? base + (g.toff[k] + slot * g.tsz[k] + sib) * 32 : 0;
    j >>= 1;
    m = (m + 1) >> 1;
  }
  for (; d < md; ++d) r[d] = 0;                                       // padMerkleProof
}

// The row at the absolute device address addr[r] (W: the widest word the row length allows); 0 is none.
template <typename W>
__global__ void __launch_bounds__(TPB) k_gather_addr(const uint64_t* __restrict__ addr, size_t nrows, size_t row_bytes,
                                                       uint8_t* __restrict__ out) {
  gather_body<W>(nrows, row_bytes, out, [=](size_t r) { return reinterpret_cast<const uint8_t*>(addr[r]); });
}

// genFakeCell (slot.nim:22-32) with a seed per group of `per` rows: row i is cell firsts[i / per] + i % per of the slot seeded
// seeds[i / per] (cp2_slot_seed).  The generator and the write-out through LDS are those of k_gen_fake_cells.
__global__ void __launch_bounds__(TPB) k_gen_fake_cells_many(const uint64_t* __restrict__ seeds, const uint64_t* __restrict__ firsts,
                                                               uint64_t per, size_t n_rows, size_t cell_size, uint8_t* __restrict__ out) {
  __shared__ uint4 gen_stage[TPB / 64][64 * 9];
  size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  const bool active = t < n_rows;
  const bool wide = ((cell_size & 127) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  if (!active && !wide) return;
  const size_t grp = active ? t / per : 0;                           // idle tail lanes only take part in the write-out
  const uint64_t seed1 = (active ? seeds[grp] : 0) + 0xdeadcafeULL;
  const uint64_t seed2 = (active ? firsts[grp] + (t - grp * per) : 0) + 0x98765432ULL;
  uint64_t state = 1;
  if (wide) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint4* my = gen_stage[wave];
    const size_t wave_row0 = (size_t)blockIdx.x * TPB + (size_t)wave * 64;
#pragma unroll 1
    for (size_t i = 0; i < cell_size; i += 128) {
#pragma unroll 1
      for (int piece = 0; piece < 8; ++piece) {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          state = state * (state + seed1) * (state + seed2) + state * (state ^ 0x5a5a5a5aULL) + seed1 * state + (seed2 + 17);
          state = state % 1698428844001831ULL;
          w[b >> 2] |= (uint32_t)(state & 0xff) << (8 * (b & 3));
        }
        my[lane * 9 + piece] = make_uint4(w[0], w[1], w[2], w[3]);   // row stride 9 x 16 B: conflict-free both ways
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = k * 8 + (lane >> 3), piece = lane & 7;
        const size_t row = wave_row0 + c;
        uint4 v = my[c * 9 + piece];
        if (row < n_rows) *reinterpret_cast<uint4*>(out + row * cell_size + i + 16 * piece) = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    return;
  }
  uint8_t* dst = out + t * cell_size;
#pragma unroll 1
  for (size_t i = 0; i < cell_size; ++i) {
    state = state * (state + seed1) * (state + seed2) + state * (state ^ 0x5a5a5a5aULL) + seed1 * state + (seed2 + 17);
    state = state % 1698428844001831ULL;
    dst[i] = (uint8_t)state;
  }
}

// ------------------------------------------------------------------------------------------------
// Scrub (scrub.cpp): a batch's freshly built layer -- cell hashes, block roots or slot roots -- against the layer the dataset keeps for
// the same slots, 32-byte rows, two 16-byte loads a side.  A wave covers 64 consecutive rows per step and writes their mismatch bitmap
// (__ballot) as one plain 64-bit store; the workgroup's tile of SCRUB_TILE rows ends with one count, summed in LDS: no atomics, and
// the host reads the counts of a clean batch (4 bytes per 4096 rows) and bitmap words only where a count is non-zero.  Every word of the
// tile is written (zeros past the last row), so the host never reads a word the kernel did not write.
constexpr int SCRUB_STEPS = (int)(SCRUB_TILE / TPB);
static_assert(SCRUB_TILE % TPB == 0 && TPB % 64 == 0, "a tile is whole workgroup steps of whole waves");
__global__ void __launch_bounds__(TPB) k_scrub_compare(const uint4* __restrict__ fresh, size_t fstride, const uint4* __restrict__ kept,
                                                         size_t kstride, size_t rows, size_t total, unsigned long long* __restrict__ bits,
                                                         uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_count[TPB / 64];
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t tile0 = (size_t)blockIdx.x * SCRUB_TILE;
  const bool dense = fstride == rows && kstride == rows;            // layer-major layouts: the batch's rows are one contiguous run on both sides
  uint32_t n = 0;
  for (int j = 0; j < SCRUB_STEPS; ++j) {
    const size_t g = tile0 + (size_t)j * TPB + threadIdx.x;
    bool diff = false;
    if (g < total) {
      size_t fo = g, ko = g;
      if (!dense) {
        const size_t item = g / rows, r = g - item * rows;
        fo = item * fstride + r;
        ko = item * kstride + r;
      }
      const uint4 a0 = fresh[2 * fo], a1 = fresh[2 * fo + 1], b0 = kept[2 * ko], b1 = kept[2 * ko + 1];
      diff = !rows_equal(a0, a1, b0, b1);
    }
    const unsigned long long m = __ballot(diff);
    if (lane == 0) bits[(tile0 + (size_t)j * TPB) / 64 + wave] = m;
    n += (uint32_t)__popcll(m);
  }
  if (lane == 0) wave_count[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < TPB / 64; ++w) s += wave_count[w];
    counts[blockIdx.x] = s;
  }
}

// The same over items whose kept layers lie anywhere (scrub.cpp, cp2_datasets_scrub_many: the slots of many datasets in one batch): the
// kept row of global row g is at kept_addr[g / rows] + (g % rows) * 32, kept_addr holding one device address per item -- row 0 of that
// item's kept layer, 16-byte aligned like every 32-byte row.  The fresh side, the 64-row ballot words, the one count per tile and the zero
// words past the last row are k_scrub_compare's; so is what the host reads of them.  The 64 lanes of a wave read one table entry (rows
// >= 64) or a few neighbouring ones: 8 bytes per item beside 64 bytes per row.
__global__ void __launch_bounds__(TPB) k_scrub_compare_many(const uint4* __restrict__ fresh, size_t fstride, const uint64_t* __restrict__ kept_addr,
                                                              size_t rows, size_t total, unsigned long long* __restrict__ bits,
                                                              uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_count[TPB / 64];
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t tile0 = (size_t)blockIdx.x * SCRUB_TILE;
  uint32_t n = 0;
  for (int j = 0; j < SCRUB_STEPS; ++j) {
    const size_t g = tile0 + (size_t)j * TPB + threadIdx.x;
    bool diff = false;
    if (g < total) {
      const size_t item = g / rows, r = g - item * rows;
      const size_t fo = item * fstride + r;
      const uint4* k = reinterpret_cast<const uint4*>(kept_addr[item]) + 2 * r;
      const uint4 a0 = fresh[2 * fo], a1 = fresh[2 * fo + 1], b0 = k[0], b1 = k[1];
      diff = !rows_equal(a0, a1, b0, b1);
    }
    const unsigned long long m = __ballot(diff);
    if (lane == 0) bits[(tile0 + (size_t)j * TPB) / 64 + wave] = m;
    n += (uint32_t)__popcll(m);
  }
  if (lane == 0) wave_count[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < TPB / 64; ++w) s += wave_count[w];
    counts[blockIdx.x] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// Building many datasets in one pass (build_many.cpp): the mirror image of k_scrub_compare_many, a WRITE through an address table.  Row g
// of the launch is row g % rows of item g / rows: the 32 bytes at src + (item * sstride + row) * 32 go to dst_addr[item] + row * 32,
// dst_addr holding one absolute device address per item -- row 0 of what that item's dataset keeps of this layer, 16-byte aligned like
// every 32-byte row; 0 = the item keeps nothing here, its rows are neither read nor written.  One lane per row, two 16-byte loads and two
// 16-byte stores; consecutive lanes take consecutive rows, so with a layer-major source and rows >= 64 a wave reads and writes whole
// contiguous runs and one table entry.  No LDS, no atomics; nothing but the rows is written.  A launch covers rows [g0, g0 + m).
__global__ void __launch_bounds__(TPB) k_scatter_rows_addr(const uint4* __restrict__ src, size_t sstride, const uint64_t* __restrict__ dst_addr,
                                                             size_t rows, size_t g0, size_t m) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= m) return;
  const size_t g = g0 + i;
  const size_t item = g / rows, r = g - item * rows;
  const uint64_t a = dst_addr[item];
  if (a == 0) return;
  const size_t so = item * sstride + r;
  const uint4 v0 = src[2 * so], v1 = src[2 * so + 1];
  uint4* d = reinterpret_cast<uint4*>(a) + 2 * r;
  d[0] = v0;
  d[1] = v1;
}

// ------------------------------------------------------------------------------------------------
// Block repair (repair.cpp): lane i takes request i's freshly built block root (fresh row i, the roots of a chunk are one contiguous
// layer) and the kept row the dataset holds for that block, two 16-byte loads a side, and writes one verdict word: 0 the roots are
// equal, 1 they differ.  No atomics, no LDS, no permutation.  The index form and the address form share this body; kept_of(i) is the
// kept row of request i, or null (never: the host validated every request), which is a mismatch and is not read.
template <typename Kept>
__device__ __forceinline__ void repair_compare_body(const uint4* __restrict__ fresh, size_t n, uint32_t* __restrict__ verdict, Kept kept_of) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint4* k = kept_of(i);
  uint32_t v = 1;
  if (k) v = rows_equal(fresh[2 * i], fresh[2 * i + 1], k[0], k[1]) ? 0u : 1u;
  verdict[i] = v;
}

// The kept row is row rows[i] of the kept node buffer, computed on the host from the dataset's layout; a row at or past kept_rows is none.
__global__ void __launch_bounds__(TPB) k_repair_compare(const uint4* __restrict__ fresh, const uint4* __restrict__ kept, size_t kept_rows,
                                                          const uint64_t* __restrict__ rows, size_t n, uint32_t* __restrict__ verdict) {
  repair_compare_body(fresh, n, verdict, [=](size_t i) -> const uint4* {
    const uint64_t r = rows[i];
    return r < kept_rows ? kept + 2 * r : nullptr;
  });
}

// Reading blocks back across datasets (read_blocks.cpp): the kept row of request i is the 32 bytes at the absolute device address
// kept_addr[i], 16-byte aligned like every 32-byte row (k_scrub_compare_many's table, one entry per request instead of one per item);
// 0 is none.  The fresh side is coalesced (64 lanes, 2 KiB in a run); the kept side is one 32-byte row wherever the request points, 8
// bytes of table beside it.  Where the time of a read-back goes is not here: a block costs 1119 permutations in k_hash_cells and the
// block-tree layer launches before its root reaches this kernel, which moves 72 bytes and writes 4 for it.
__global__ void __launch_bounds__(TPB) k_repair_compare_addr(const uint4* __restrict__ fresh, const uint64_t* __restrict__ kept_addr, size_t n,
                                                               uint32_t* __restrict__ verdict) {
  repair_compare_body(fresh, n, verdict, [=](size_t i) { return reinterpret_cast<const uint4*>(kept_addr[i]); });
}

// ------------------------------------------------------------------------------------------------
// What SampleAndProve accepts (circuit/codex/sample_cells.circom:58-148, single_cell.circom:30-73, merkle.circom:44-114), checked
// in one launch: lane t < n*ns takes sample t % ns of input t / ns from its cell felts to the slot-root comparison (index sponge,
// leaf sponge, bottom and middle reconstructions); lane n*ns + i checks input i's slot root against its dataset root.  One byte per
// lane: 1 = that equation holds.  Inputs whose shape the circuit's witness generation refuses (VerifyGeom: prm[3] == 0) get 0.

// RootFromMerklePath(depth) (merkle.circom:44-114) for the masks SampleAndProve feeds it: after maskBitsCorrected[0] = 1 they are
// [1,..,1,0,..,0], so recRoot is aux[sel] with sel = the number of ones, and only sel compressions are needed (depth 0: the empty
// sum, 0).  isLast[i] = bits i..depth-1 of the index equal those of the last index (diff >> i == 0); the switch by the path bit
// and the key bottom + 2*odd are selects, not branches.
struct PathWalk {
  uint64_t bits, diff;   // index bits; (index ^ last index) over the tree's depth
  const uint4* path;
  uint32_t sel;          // compressions up to the selected layer
};

__device__ __forceinline__ uint64_t shr64(uint64_t x, uint32_t s) { return s >= 64 ? 0 : x >> s; }
__device__ __forceinline__ uint64_t low_bits(uint64_t x, uint32_t depth) { return depth >= 64 ? x : x & ((1ULL << depth) - 1); }
__device__ __forceinline__ uint32_t clamp_sel(uint32_t ones, uint32_t depth) { return depth == 0 ? 0u : (ones < 1u ? 1u : (ones < depth ? ones : depth)); }

// field equality (the circuit's ===): both sides as canonical words
__device__ __forceinline__ bool fe_equal(const Fe& a, const Fe& b) {
  uint32_t wa[8], wb[8];
  fr::to_canonical_words(a, wa);
  fr::to_canonical_words(b, wb);
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= wa[i] ^ wb[i];
  return d == 0;
}

// One loop, one permutation per step, for every lane: a sample lane runs 2 index steps (sponge over [entropy, slotRoot, counter]),
// ceil((nf+1)/2) leaf steps, then the bottom walk and the middle walk; a top lane runs the top walk only.  Whole batches share the
// circuit parameters, so the step counts and the phase tests are uniform across a wave except where inputs state other nCellsPerSlot
// or nSlotsPerDataSet.
__global__ void __launch_bounds__(TPB) k_verify_samples(VerifyGeom g, const uint64_t* __restrict__ prm, const uint4* __restrict__ heads,
                                                          const uint4* __restrict__ cells, const uint4* __restrict__ paths,
                                                          uint8_t* __restrict__ ok) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  const size_t nst = g.n * g.ns;
  if (t >= nst + g.n) return;
  const bool top = t >= nst;
  const size_t item = top ? t - nst : t / g.ns;
  const uint64_t* q = prm + 4 * item;
  if (q[3] == 0) {                                                     // shape refused by witness generation
    ok[t] = 0;
    return;
  }
  const uint4* head = heads + 2 * (size_t)(3 + g.m) * item;          // dataSetRoot, entropy, slotRoot, slotProof[m]
  const Fe slot_root = load_fe_canonical(head + 4);
  const Fe one = fr::fe_const(fr::FR_R1);
  const uint4* src = cells + 2 * t * g.nf;
  const uint64_t n_cells = q[0], lastc = n_cells - 1;
  const uint32_t k = (uint32_t)__builtin_ctzll(n_cells);              // Log2: nCells = 2^k, 1 <= k <= maxDepth (checked on the host)
  const uint32_t dm = g.md - g.bd;
  PathWalk wa, wb;                                                     // sample: bottom, middle (single_cell.circom:41-60); top: top, -
  uint32_t n_pre, depth_last;
  Fe cur;
  State s;
  if (top) {                                                           // sample_cells.circom:95-109
    const uint64_t last = q[1] - 1;                                    // CeilingLog2: bits of nSlots - 1, mask = its bit length
    const uint32_t bl = last ? 64u - (uint32_t)__builtin_clzll(last) : 0u;
    wa = PathWalk{q[2], low_bits(q[2] ^ last, g.m), head + 6, clamp_sel(bl, g.m)};
    wb = PathWalk{0, 0, head, 0};
    n_pre = 0;
    depth_last = g.m;
    cur = slot_root;
    s.x = s.y = s.z = fr::fe_zero();
  } else {                                                             // CalculateCellIndexBits, sample_cells.circom:23-48
    const uint4* path = paths + 2 * t * g.md;
    wa = PathWalk{0, 0, path, k < g.bd ? k : g.bd};
    wb = PathWalk{0, 0, path + 2 * g.bd, clamp_sel(k > g.bd ? k - g.bd : 0u, dm)};
    n_pre = 2 + ((g.nf + 2) >> 1);
    depth_last = dm;
    cur = fr::fe_zero();
    s.x = load_fe_canonical(head + 2);
    s.y = slot_root;
    s.z = fr::fe_const(fr::FR_CIV_RATE2_MONT);
  }
  const uint32_t total = n_pre + wa.sel + wb.sel;
#pragma unroll 1
  for (uint32_t step = 0; step < total; ++step) {
    if (step < n_pre) {
      if (step == 1) {                                                 // counter cnt + 1, then the sponge's "1" pad
        const uint32_t counter = (uint32_t)(t - item * g.ns) + 1;
        Fe c = fr::fe_zero();
        c.l[0] = counter & fr::MASK;
        c.l[1] = counter >> 29;
        s.x = fr::norm(fr::add_lazy(s.x, fr::to_mont(c)));
        s.y = fr::norm(fr::add_lazy(s.y, one));
      } else if (step >= 2) {                                          // Poseidon2_hash_rate2(cellData), single_cell.circom:63-65
        const uint32_t j = 2 * (step - 2);
        Fe a = (j < g.nf) ? load_fe_canonical(src + 2 * j) : (j == g.nf ? one : fr::fe_zero());
        Fe b = (j + 1 < g.nf) ? load_fe_canonical(src + 2 * (j + 1)) : (j + 1 == g.nf ? one : fr::fe_zero());
        s.x = fr::norm(fr::add_lazy(s.x, a));
        s.y = fr::norm(fr::add_lazy(s.y, b));
      }
    } else {
      const uint32_t lvl = step - n_pre;
      const bool in_a = lvl < wa.sel;
      const uint32_t i = in_a ? lvl : lvl - wa.sel;
      const uint64_t bits = in_a ? wa.bits : wb.bits, diff = in_a ? wa.diff : wb.diff;
      const uint32_t b = (uint32_t)(bits >> i) & 1u;
      const uint32_t key = (i == 0 ? 1u : 0u) + 2u * (((diff >> i) == 0 ? 1u : 0u) & (b ^ 1u));
      const Fe sib = load_fe_canonical((in_a ? wa.path : wb.path) + 2 * i);
      const uint32_t sw = 0u - b;
#pragma unroll
      for (int l = 0; l < fr::NL; ++l) {
        s.x.l[l] = (cur.l[l] & ~sw) | (sib.l[l] & sw);
        s.y.l[l] = (sib.l[l] & ~sw) | (cur.l[l] & sw);
      }
      s.z = key_fe(key);
    }
    p2::permute(s, qtab);
    if (step == 1 && !top) {                                           // the index: low bits & (nCells - 1); the leaf sponge starts
      uint32_t w[8];
      fr::to_canonical_words(s.x, w);
      const uint64_t idx = (((uint64_t)w[1] << 32) | w[0]) & lastc;
      wa.bits = idx;                                                   // lastBits = the Log2 mask (sample_cells.circom:117-123)
      wa.diff = low_bits(idx ^ lastc, g.bd);
      wb.bits = shr64(idx, g.bd);
      wb.diff = low_bits(shr64(idx ^ lastc, g.bd), dm);
      s.x = fr::fe_zero();
      s.y = fr::fe_zero();
      s.z = fr::fe_const(fr::FR_CIV_RATE2_MONT);
    } else if (step + 1 >= n_pre) {                                    // the leaf, then each reconstructed layer
      cur = fr::norm(s.x);
    }
  }
  const Fe want = top ? load_fe_canonical(head) : slot_root;           // dataSetRoot / slotRoot (single_cell.circom:71)
  ok[t] = fe_equal(depth_last ? cur : fr::fe_zero(), want) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// The block-path walk, shared by the four k_block_path_* kernels: reconstructRoot (merkle.nim:51-74) from a block root up `len` levels,
// the schedule of block_proof_schedule (block_proof_plan.hpp).  j is the running index and m the layer size, both carried from level 0;
// the node goes right where j is odd (left / right by limb masks), the key is (level 0 ? 1 : 0) + 2 where j is the even last node of its
// layer (by arithmetic), one permutation per level.  Level l reads row l of `path`.  Returns the node reached; len == 0 returns `cur`.
//   STAGE: lane-private staging.  For every level l the canonical sibling (a value of at least r lands as its residue) and the canonical
//   ancestor (`cur` after level l) go to rows 2 l and 2 l + 1 of `mine`, two uint4 a row: staging memory, never the tree, so unproved
//   data goes nowhere else, and the walk holds none of the 2 x len rows in registers.  Without STAGE `mine` is not used and nothing is
//   stored.
template <bool STAGE>
__device__ __forceinline__ Fe walk_block_path(Fe cur, const uint4* __restrict__ path, uint4* mine, uint64_t j, uint64_t m, uint32_t len,
                                              const fr::QTab& qtab) {
  State s;
#pragma unroll 1
  for (uint32_t lvl = 0; lvl < len; ++lvl) {
    const Fe sib = load_fe_canonical(path + 2 * lvl);
    if constexpr (STAGE) store_fe_canonical(mine + 4 * lvl, sib);
    const uint32_t b = (uint32_t)j & 1u;
    const uint32_t key = (lvl == 0 ? 1u : 0u) + 2u * ((j == m - 1 ? 1u : 0u) & (b ^ 1u));
    const uint32_t sw = 0u - b;
#pragma unroll
    for (int l = 0; l < fr::NL; ++l) {
      s.x.l[l] = (cur.l[l] & ~sw) | (sib.l[l] & sw);
      s.y.l[l] = (sib.l[l] & ~sw) | (cur.l[l] & sw);
    }
    s.z = key_fe(key);
    p2::permute(s, qtab);
    cur = fr::norm(s.x);
    if constexpr (STAGE) store_fe_canonical(mine + 4 * lvl + 2, cur);
    j >>= 1;
    m = (m + 1) >> 1;
  }
  return cur;
}

// What a staged walk keeps after a match: a loop with no permutation in it that copies rows of `mine` into the session's compact buffer,
// two 16-byte loads and two 16-byte stores each.  Sibling l goes to layer l, index (blk >> l) ^ 1, for l < len; ancestor l to layer l + 1,
// index blk >> (l + 1), for l < n_anc only.  The row of (layer l, index) is layer_off[l] + slot * layer_size[l] + index (FillPlan::node_row,
// fill_plan.hpp), from two device tables of depth + 1 entries.  An index at or past layer_size[l] -- the ZERO sibling of an odd layer's
// last node, or of the one-block slot -- is skipped, and so is a row at or past n_rows (never: the host validated every request and made
// the tables).  Nothing at layer n_anc + 1 or above is written, and above layer len - 1 no sibling either.
__device__ __forceinline__ void keep_path_rows(uint4* tree, const uint4* mine, const uint64_t* __restrict__ layer_off,
                                               const uint64_t* __restrict__ layer_size, uint64_t slot, uint64_t blk, uint32_t len,
                                               uint32_t n_anc, uint64_t n_rows) {
#pragma unroll 1
  for (uint32_t lvl = 0; lvl < len; ++lvl) {
    const uint64_t size = layer_size[lvl], sib = (blk >> lvl) ^ 1;
    const uint64_t rs = layer_off[lvl] + slot * size + sib;
    if (sib < size && rs < n_rows) copy_row(tree + 2 * rs, mine + 4 * lvl);
    if (lvl >= n_anc) break;
    const uint64_t up = layer_size[lvl + 1], anc = blk >> (lvl + 1);
    const uint64_t ra = layer_off[lvl + 1] + slot * up + anc;
    if (anc < up && ra < n_rows) copy_row(tree + 2 * ra, mine + 4 * lvl + 2);
  }
}

// ------------------------------------------------------------------------------------------------
// Block proofs (block_proofs.cpp): lane i takes request i's freshly built block root (fresh row i, where k_repair_compare reads it), its
// (slot root index, block) pair and its path of `depth` siblings, and walks up to the slot root.  The result is compared with
// slot_roots[root] as canonical words; one verdict word: 0 equal, 1 not.  depth is uniform over the launch, j and m are per lane.  The
// host validated every request (root < n_roots, block < n_blocks).  roots_out (may be NULL) receives the block root each candidate
// hashed to.
__global__ void __launch_bounds__(TPB) k_block_path_roots(const uint4* __restrict__ fresh, const uint4* __restrict__ paths,
                                                            const uint64_t* __restrict__ root_block, const uint4* __restrict__ slot_roots,
                                                            uint64_t n_blocks, uint32_t depth, size_t n, uint32_t* __restrict__ verdict,
                                                            uint4* __restrict__ roots_out) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  if (roots_out) copy_row(roots_out + 2 * i, fresh + 2 * i);
  const Fe cur = walk_block_path<false>(load_fe_canonical(fresh + 2 * i), paths + 2 * i * depth, nullptr, root_block[2 * i + 1], n_blocks,
                                        depth, qtab);
  const Fe want = load_fe_canonical(slot_roots + 2 * root_block[2 * i]);
  verdict[i] = fe_equal(cur, want) ? 0u : 1u;
}

// ------------------------------------------------------------------------------------------------
// Repair across many datasets (repair_many.cpp): k_block_path_roots' walk and k_repair_compare_addr's table in one kernel, everything per
// lane.  Lane i takes request i's freshly built block root (fresh row i) and its descriptor: it walks len levels (0, or its dataset's
// depth) from j = blk over a first layer of n_blocks nodes, reading its siblings at row path_at of the chunk's staged paths, and compares
// what it reaches with the 32-byte row at the absolute address `want` as canonical words -- the kept block root where len is 0 (the walk
// returns the row itself), the dataset's own slot root otherwise.  One verdict word: 0 equal, 1 not; want == 0 or not 16-byte aligned is a
// mismatch and is not read (never: the host made the table).  No other store, no atomics.  A wave that mixes depths and path-less
// requests runs to its longest walk.
__global__ void __launch_bounds__(TPB) k_repair_judge_many(const uint4* __restrict__ fresh, const uint4* __restrict__ paths,
                                                             const RepairManyReq* __restrict__ reqs, size_t n, uint32_t* __restrict__ verdict) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const RepairManyReq q = reqs[i];
  const Fe cur = walk_block_path<false>(load_fe_canonical(fresh + 2 * i), paths + 2 * q.path_at, nullptr, q.blk, q.n_blocks, q.len, qtab);
  uint32_t v = 1;
  if (q.want != 0 && (q.want & 15) == 0) v = fe_equal(cur, load_fe_canonical(reinterpret_cast<const uint4*>(q.want))) ? 0u : 1u;
  verdict[i] = v;
}

// ------------------------------------------------------------------------------------------------
// Slot filling (fill.cpp): the same walk, with what a fill session keeps of a proved block.  Lane i takes request i's freshly built block
// root, its (local slot, block) pair and its path, and compares the result with slot_roots[slot] as canonical words.  Where they are equal
// it also copies the canonical block root (row i of `fresh`, as the layer kernel wrote it) to row dest[i] of `layer0`, the session's
// compact buffer: the host computed dest[i] = coff[0] + local_slot * csizes[0] + block, a row of layer 0.  Two 16-byte vector stores; the
// row is read again from `fresh` after the walk instead of being held in registers across it.  No atomics and no device bitmap: the host's
// bitmap is the authority on presence.  Two matching requests for the same (slot, block) in one launch store identical bytes to one row,
// which is benign: a block root that reconstructs the slot root at that position is the one block root the tree has there.  A row at or
// past n_rows (never: the host validated every request) is a mismatch and nothing is stored.
__global__ void __launch_bounds__(TPB) k_block_path_commit(const uint4* __restrict__ fresh, const uint4* __restrict__ paths,
                                                             const uint64_t* __restrict__ slot_block, const uint4* __restrict__ slot_roots,
                                                             const uint64_t* __restrict__ dest, uint64_t n_blocks, uint32_t depth, size_t n,
                                                             uint32_t* __restrict__ verdict, uint4* __restrict__ layer0, uint64_t n_rows) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const Fe cur = walk_block_path<false>(load_fe_canonical(fresh + 2 * i), paths + 2 * i * depth, nullptr, slot_block[2 * i + 1], n_blocks,
                                        depth, qtab);
  const Fe want = load_fe_canonical(slot_roots + 2 * slot_block[2 * i]);
  const uint64_t r = dest[i];
  const bool keep = fe_equal(cur, want) && r < n_rows;
  verdict[i] = keep ? 0u : 1u;
  if (keep) {                                          // load, store, load, store.  Not copy_row: with its two loads first this kernel
    layer0[2 * r] = fresh[2 * i];                      // compiles to 133 VGPRs and three waves per SIMD instead of 82 and five
    layer0[2 * r + 1] = fresh[2 * i + 1];
  }
}

// ------------------------------------------------------------------------------------------------
// Slot filling with the nodes kept (fill.cpp, a session after cp2_fill_keep_nodes): k_block_path_commit's walk and comparison with
// slot_roots[slot], staged, with what a serving session keeps of a proved path: all of it.  A path that ends in the stated slot root
// proves every node on it, the `depth` siblings the peer sent and the `depth` ancestors the walk computed (were one of them wrong,
// another root would have come out), and the session's compact buffer has a row for each.  Lane i stages into its own `depth` x 2 rows
// of `scratch`.  After the verdict, on a match only, it copies the block root to layer 0, row dest[i] (as k_block_path_commit), and every
// sibling and ancestor where the tables put them.  On a mismatch nothing outside the lane's scratch rows and its verdict word is written.
// No atomics: two proved requests that name the same node store identical bytes, the argument k_block_path_commit makes for layer 0, which
// holds for every authentic node.  LDS is the QTab only.
__global__ void __launch_bounds__(TPB) k_block_path_commit_nodes(const uint4* __restrict__ fresh, const uint4* __restrict__ paths,
                                                                   const uint64_t* __restrict__ slot_block, const uint4* __restrict__ slot_roots,
                                                                   const uint64_t* __restrict__ dest, const uint64_t* __restrict__ layer_off,
                                                                   const uint64_t* __restrict__ layer_size, uint64_t n_blocks, uint32_t depth,
                                                                   size_t n, uint32_t* __restrict__ verdict, uint4* __restrict__ tree,
                                                                   uint64_t n_rows, uint4* scratch) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  uint4* mine = scratch + 4 * i * depth;
  const uint64_t slot = slot_block[2 * i], blk = slot_block[2 * i + 1];
  const Fe cur = walk_block_path<true>(load_fe_canonical(fresh + 2 * i), paths + 2 * i * depth, mine, blk, n_blocks, depth, qtab);
  const Fe want = load_fe_canonical(slot_roots + 2 * slot);
  const uint64_t r = dest[i];
  const bool keep = fe_equal(cur, want) && r < n_rows;
  verdict[i] = keep ? 0u : 1u;
  if (!keep) return;
  copy_row(tree + 2 * r, fresh + 2 * i);
  keep_path_rows(tree, mine, layer_off, layer_size, slot, blk, depth, depth, n_rows);
}

// ------------------------------------------------------------------------------------------------
// Slot filling with paths that stop at a kept node (fill.cpp, cp2_fill_add_anchored): the staged walk with a per-lane length and a
// per-lane target.  A computed node that equals an authentic node proves everything below it -- the collision argument the whole walk
// rests on -- so a block whose ancestor at level a the session already knows needs its a lowest siblings only.  Lane i takes fresh block
// root i, levels[i] (at most depth; anything above is a mismatch), its (local slot, block) pair and its levels[i] siblings at row
// path_off[i] - path_base of the PACKED path buffer `paths` (path_off is the prefix sum of levels over the whole call, path_base the
// entry of the first request whose siblings `paths` holds).  It stages into its own 2 x levels[i] rows of `scratch`, which start at row
// 2 (path_off[i] - path_base).
//   The result is compared with row anchor_row[i] of `tree`, loaded as a canonical element; anchor_row[i] == UINT64_MAX stands for
//   slot_roots[slot]; any other row at or past n_rows is a mismatch.  levels[i] == 0 runs no permutation: the fresh root against the kept row.
//   On a match only, rows are copied: the block root to row dest[i] (unless levels[i] == 0, where that row is the anchor), every sibling,
//   and the ancestors below the last level's, which is the anchor and already there.  The anchor row and every row above it are never
//   written.  On a mismatch nothing outside the lane's scratch rows and its verdict word is.
// The host states only anchors that were known before the launch (FillPlan::validate_anchored), so an anchor row that another lane of the
// launch rewrites is rewritten with the value it holds: a known row can only be proved equal to itself.  No atomics, as in
// k_block_path_commit_nodes; LDS is the QTab only.  Lanes of a wave walk different lengths; a wave lasts as long as its longest lane.
__global__ void __launch_bounds__(TPB) k_block_path_commit_anchored(const uint4* __restrict__ fresh, const uint4* __restrict__ paths,
                                                                      const uint32_t* __restrict__ levels, const uint64_t* __restrict__ path_off,
                                                                      uint64_t path_base, const uint64_t* __restrict__ slot_block,
                                                                      const uint4* __restrict__ slot_roots, const uint64_t* __restrict__ dest,
                                                                      const uint64_t* __restrict__ anchor_row,
                                                                      const uint64_t* __restrict__ layer_off,
                                                                      const uint64_t* __restrict__ layer_size, uint64_t n_blocks, uint32_t depth,
                                                                      size_t n, uint32_t* __restrict__ verdict, uint4* tree, uint64_t n_rows,
                                                                      uint4* scratch) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint32_t len = levels[i];
  if (len > depth) {                                   // (never: the host validated every level)
    verdict[i] = 1u;
    return;
  }
  const uint64_t at = path_off[i] - path_base;
  uint4* mine = scratch + 4 * at;
  const uint64_t slot = slot_block[2 * i], blk = slot_block[2 * i + 1];
  const Fe cur = walk_block_path<true>(load_fe_canonical(fresh + 2 * i), paths + 2 * at, mine, blk, n_blocks, len, qtab);
  const uint64_t target = anchor_row[i];
  const bool stated = target == ~(uint64_t)0;
  if (!stated && target >= n_rows) {
    verdict[i] = 1u;
    return;
  }
  const Fe want = load_fe_canonical(stated ? slot_roots + 2 * slot : tree + 2 * target);
  const uint64_t r = dest[i];
  const bool keep = fe_equal(cur, want) && r < n_rows;
  verdict[i] = keep ? 0u : 1u;
  if (!keep || len == 0) return;
  copy_row(tree + 2 * r, fresh + 2 * i);
  keep_path_rows(tree, mine, layer_off, layer_size, slot, blk, len, len - 1, n_rows);
}

// ------------------------------------------------------------------------------------------------
// Slot filling across many sessions (fill_many.cpp, cp2_fills_add_many): k_block_path_commit_anchored with the session taken per lane.
// What the three kernels above take as launch arguments -- the compact buffer and its n_rows, the stated roots, the layer tables, n_blocks
// and depth -- lane i reads from descriptor session_of[i] of `sessions` (FillManySession, kernels.hpp; the host uploads the table once per
// call).  The request arrays are device_requests_anchored's: levels, path_off (absolute; path_base as above), (local slot, block), dest
// and anchor_row, the rows being rows of the lane's OWN session's buffer.  The walk is walk_block_path<true> from fresh row i with j =
// block, m = the session's n_blocks, staged into the lane's 2 x levels[i] rows of `scratch` at row 2 (path_off[i] - path_base); the result
// is compared with the anchor row of the session's buffer, or, anchor_row[i] == UINT64_MAX, with the session's stated root of the slot.
//   On a match only, and unless levels[i] == 0, the block root goes to row dest[i] of the session's buffer.  A session that keeps nodes
//   (layer_tab != 0: layer_off at that address, layer_size depth + 1 entries behind it) also receives the siblings and the ancestors
//   strictly below the anchor through keep_path_rows with ITS tables; with keep_top != 0 (a call of whole paths, which is cp2_fill_add per
//   session) a path of the session's full depth leaves its last ancestor, the slot root's row, as k_block_path_commit_nodes does.  A session
//   that keeps none gets the block root alone.
//   Defensive mismatches (the host never produces them; each writes the verdict word and nothing else, not even scratch): a session index
//   at or past n_sessions, a level above the session's depth, a level below it in a session that keeps no nodes, a slot at or past n_local,
//   a dest or anchor row at or past n_rows.
// No atomics; plain 16-byte loads and stores; LDS is the QTab only.  Two sessions never share a buffer, and inside one session the argument
// of k_block_path_commit_anchored holds: identical bytes to one row, and only anchors known before the launch.  Lanes of a wave now differ
// in DEPTH as well as in level (neighbouring requests belong to different sessions): a wave lasts as long as its longest lane, the
// deepest session's whole path at worst.  The one staged walk serves every lane, so a lane of a session that keeps no nodes also writes
// its 64 x levels[i] bytes of staging, which nothing reads (k_block_path_commit stages nothing).  Measured with every session plain, 4096
// sessions x 4 whole paths of depth 4 beside 64 KiB blocks: the whole call, this traffic, the descriptor loads and the host grouping
// included, takes 1.02 times the one-session k_block_path_commit call (profiles/fill_many_rate.txt); 256 B staged against 65 536 B hashed.
__global__ void __launch_bounds__(TPB) k_block_path_commit_many(const uint4* __restrict__ fresh, const uint4* __restrict__ paths,
                                                                  const FillManySession* __restrict__ sessions, uint64_t n_sessions,
                                                                  const uint64_t* __restrict__ session_of,
                                                                  const uint32_t* __restrict__ levels, const uint64_t* __restrict__ path_off,
                                                                  uint64_t path_base, const uint64_t* __restrict__ slot_block,
                                                                  const uint64_t* __restrict__ dest, const uint64_t* __restrict__ anchor_row,
                                                                  uint32_t keep_top, size_t n, uint32_t* __restrict__ verdict, uint4* scratch) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = session_of[i];
  if (k >= n_sessions) {                               // (never, like everything refused below: the host validated every request)
    verdict[i] = 1u;
    return;
  }
  const FillManySession* d = sessions + k;
  const uint64_t n_rows = d->n_rows, tab = d->layer_tab;
  const uint32_t depth = d->depth, len = levels[i];
  const uint64_t slot = slot_block[2 * i], blk = slot_block[2 * i + 1];
  const uint64_t r = dest[i], target = anchor_row[i];
  const bool stated = target == ~(uint64_t)0;
  if (len > depth || (len < depth && tab == 0) || slot >= d->n_local || r >= n_rows || (!stated && target >= n_rows)) {
    verdict[i] = 1u;
    return;
  }
  uint4* tree = reinterpret_cast<uint4*>(d->tree);
  const uint64_t at = path_off[i] - path_base;
  uint4* mine = scratch + 4 * at;
  const Fe cur = walk_block_path<true>(load_fe_canonical(fresh + 2 * i), paths + 2 * at, mine, blk, d->n_blocks, len, qtab);
  const Fe want = load_fe_canonical(stated ? reinterpret_cast<const uint4*>(d->slot_roots) + 2 * slot : tree + 2 * target);
  const bool keep = fe_equal(cur, want);
  verdict[i] = keep ? 0u : 1u;
  if (!keep || len == 0) return;
  copy_row(tree + 2 * r, fresh + 2 * i);
  if (tab == 0) return;
  const uint64_t* layer_off = reinterpret_cast<const uint64_t*>(tab);
  keep_path_rows(tree, mine, layer_off, layer_off + depth + 1, slot, blk, len, keep_top && len == depth ? len : len - 1, n_rows);
}

// ------------------------------------------------------------------------------------------------
// Resuming a fill session (fill.cpp): k_repair_compare's comparison, with what a resumed session does about a block whose bytes on disk no
// longer hash to the root the checkpoint kept -- as k_block_path_commit is k_block_path_roots' walk with what a session keeps of a proved
// block.  Lane i takes the freshly built block root of re-read block i (fresh row i) and row dest[i] of `layer0`, the session's compact
// buffer (the host computed dest[i] inside layer 0), two 16-byte loads a side, and writes one verdict word: 0 equal, 1 not.  Where they
// differ it overwrites the row of layer 0 with zeros, two 16-byte vector stores, so that the buffer never keeps a root the disk does not
// back; the host clears the block's presence bit from the verdict.  The rows of one launch are distinct (the read plan names every present
// block once), so no lane reads a row another lane zeroes.  A row at or past n_rows (never: the host computed every row) is a mismatch
// and is neither read nor written.  No atomics, no LDS, no permutation.
// The row form and the address form share this step: fresh row i against the kept row at k (never null here), which is zeroed where they differ.
__device__ __forceinline__ uint32_t block_root_recheck_row(const uint4* __restrict__ fresh, size_t i, uint4* k) {
  const uint32_t v = rows_equal(fresh[2 * i], fresh[2 * i + 1], k[0], k[1]) ? 0u : 1u;
  if (v) {
    k[0] = make_uint4(0, 0, 0, 0);
    k[1] = make_uint4(0, 0, 0, 0);
  }
  return v;
}

__global__ void __launch_bounds__(TPB) k_block_root_recheck(const uint4* __restrict__ fresh, const uint64_t* __restrict__ dest, size_t n,
                                                              uint32_t* __restrict__ verdict, uint4* __restrict__ layer0, uint64_t n_rows) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint64_t r = dest[i];
  uint32_t v = 1;
  if (r < n_rows) v = block_root_recheck_row(fresh, i, layer0 + 2 * r);
  verdict[i] = v;
}

// Resuming many fill sessions in one pass (fills_resume_many.cpp): the kept row of re-read block i is the 32 bytes at the absolute device
// address addr[i] -- layer 0 of the session the block belongs to, plus its row x 32 --, as k_repair_compare_addr takes the kept row of a
// request, so that the present blocks of every session share each launch.  The fresh side is coalesced (64 lanes, 2 KiB in a run); the
// kept side is one 32-byte row wherever the block's session lies, 8 bytes of table beside it.  A differing row is zeroed in its own
// session's buffer, two 16-byte vector stores.  The addresses of one launch are distinct (the plan names every present block of every
// session once, and every session owns its buffer), so no lane reads a row another lane zeroes.  addr[i] == 0, or an address that is not
// 16-byte aligned (never: the host made the table from allocation bases and rows), is a mismatch and is neither read nor written.  No
// atomics, no LDS, no permutation.
__global__ void __launch_bounds__(TPB) k_block_root_recheck_addr(const uint4* __restrict__ fresh, const uint64_t* __restrict__ addr, size_t n,
                                                                   uint32_t* __restrict__ verdict) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint64_t a = addr[i];
  uint32_t v = 1;
  if (a != 0 && (a & 15) == 0) v = block_root_recheck_row(fresh, i, reinterpret_cast<uint4*>(a));
  verdict[i] = v;
}

// ------------------------------------------------------------------------------------------------
// One level of the induced subtrees of many block multiproofs (multiproofs.cpp; the tables are multiproof_plan.hpp's).  `work` is the
// call's work table of 32-byte rows: leaf rows, sent rows, then the computed rows level after level.  Lane t < n_jobs runs job t of the
// level: it reads rows `left` and `right` (right == MULTIPROOF_ZERO: the zero beside an odd layer's last node), compresses them under the
// job's key -- k_compress_layer's rule, the key made by the host -- and stores the result at row out_base + t.  Every row a job names
// lies below out_base (an earlier level's output, a leaf or a sent row), so the rows a launch reads and the rows it writes are disjoint.
//   A job with `last` set produces its group's top node: besides storing it, the lane compares it as a field element (fe_equal: a stated
//   root >= r counts mod r, as every path row does) with the 32 bytes at want_addr[group] and writes verdict[group] = 0 or 1.  Every group
//   has exactly one such job in a call, so nothing is cleared beforehand and there are no atomics.
//   Defensive (the host never produces them): a want_addr that is 0 or not 16-byte aligned is a mismatch and is not read; a job whose
//   left or right row is at or past out_base reads and stores nothing, and with `last` set its verdict is 1.
// LDS is the QTab only; the register bound names k_compress_layer's 5 waves per SIMD, as k_finish_layer_many's does
// (profiles/multiproof_kernel_resources.txt).
__global__ void __launch_bounds__(TPB, 5) k_multiproof_layer(uint4* __restrict__ work, const MultiproofJob* __restrict__ jobs, size_t n_jobs,
                                                            uint64_t out_base, const uint64_t* __restrict__ want_addr,
                                                            uint32_t* __restrict__ verdict) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= n_jobs) return;
  const MultiproofJob j = jobs[t];
  const bool pair = j.right != MULTIPROOF_ZERO, last = (j.key_last >> 8) & 1u;
  if (j.left >= out_base || (pair && j.right >= out_base)) {   // (never: the host numbers the rows level by level)
    if (last) verdict[j.group] = 1u;
    return;
  }
  State st;
  st.x = load_fe_canonical(work + 2 * (size_t)j.left);
  st.y = pair ? load_fe_canonical(work + 2 * (size_t)j.right) : fr::fe_zero();
  st.z = key_fe(j.key_last & 3u);
  p2::permute(st, qtab);
  store_fe_canonical(work + 2 * (out_base + t), st.x);
  if (!last) return;
  const uint64_t a = want_addr[j.group];
  uint32_t v = 1u;
  if (a != 0 && (a & 15) == 0) v = fe_equal(st.x, load_fe_canonical(reinterpret_cast<const uint4*>(a))) ? 0u : 1u;
  verdict[j.group] = v;
}

// ------------------------------------------------------------------------------------------------
// What a fill session keeps of proved multiproofs (fill.cpp, cp2_fill_add_multi): lane i copies row src_row[i] of the work table to the
// absolute address dst_addr[i] -- a row of the session's compact buffer -- when its group proved (verdict[group_of[i]] == 0), and does
// nothing otherwise: a group that fails leaves nothing behind.  A row as it stands, two 16-byte loads and two 16-byte stores (the work
// table holds canonical rows: k_multiproof_layer's stores, the block roots of the hashing, and sent rows, which the host made canonical).
// Two lanes that name one destination carry identical bytes, k_block_path_commit's argument: every row of a proved group is the authentic
// node of its place in the tree, and a place has one node.  Defensive (the host never produces them): a source row at or past n_work, a
// group at or past n_groups and a destination that is 0 or not 16-byte aligned copy nothing.  No permutation, no LDS, no atomics.
__global__ void __launch_bounds__(TPB) k_multiproof_commit(const uint4* __restrict__ work, uint64_t n_work, const uint32_t* __restrict__ src_row,
                                                             const uint64_t* __restrict__ dst_addr, const uint32_t* __restrict__ group_of,
                                                             const uint32_t* __restrict__ verdict, uint32_t n_groups, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = group_of[i], r = src_row[i];
  const uint64_t a = dst_addr[i];
  if (g >= n_groups || r >= n_work || a == 0 || (a & 15) != 0) return;
  if (verdict[g] != 0) return;
  copy_row(reinterpret_cast<uint4*>(a), work + 2 * (size_t)r);
}

// ------------------------------------------------------------------------------------------------
// The verdicts of multiproofs that stop at nodes a fill session holds (fill.cpp, cp2_fill_add_multi_anchored;
// multiproof_anchor_plan.hpp).  A group of such a call has one or more TOPS: rows of the work table -- a fresh block root or a node
// k_multiproof_layer computed -- that must equal an authentic row the session keeps.  Lane t compares row tops[t].row with the 32 bytes
// at want_addr[t] as field elements (fe_equal on canonical loads, as k_multiproof_layer compares its top) and writes top_verdict[t] = 0
// or 1.  No permutation, no LDS, no atomics.  Defensive (the host never produces them): a row at or past n_work and an address that is 0
// or not 16-byte aligned are a mismatch and are not read.
__global__ void __launch_bounds__(TPB) k_multiproof_tops(const uint4* __restrict__ work, uint64_t n_work, const MultiproofTop* __restrict__ tops,
                                                           const uint64_t* __restrict__ want_addr, size_t n_tops, uint32_t* __restrict__ top_verdict) {
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= n_tops) return;
  const uint32_t r = tops[t].row;
  const uint64_t a = want_addr[t];
  uint32_t v = 1u;
  if (r < n_work && a != 0 && (a & 15) == 0)
    v = fe_equal(load_fe_canonical(work + 2 * (size_t)r), load_fe_canonical(reinterpret_cast<const uint4*>(a))) ? 0u : 1u;
  top_verdict[t] = v;
}

// ... and the group's verdict: lane g ORs top_verdict over its group's range [top_off[g], top_off[g + 1]) (the tops are group-major)
// into verdict[g]; a group without a top has nothing that vouches for it and gets 1.  Every word has one writer; nothing is cleared
// beforehand.  A range that descends or ends past n_tops (the launcher refuses them) reads nothing and gives 1.
__global__ void __launch_bounds__(TPB) k_multiproof_fold(const uint32_t* __restrict__ top_verdict, size_t n_tops, const uint64_t* __restrict__ top_off,
                                                           size_t n_groups, uint32_t* __restrict__ verdict) {
  const size_t g = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (g >= n_groups) return;
  const uint64_t t0 = top_off[g], t1 = top_off[g + 1];
  uint32_t v = t1 <= t0 || t1 > n_tops ? 1u : 0u;
  if (v == 0u)
    for (uint64_t t = t0; t < t1; ++t) v |= top_verdict[t] != 0u ? 1u : 0u;
  verdict[g] = v;
}

// ------------------------------------------------------------------------------------------------
// The children of one node of a fill session's tree, ready for the keyed compression: rows rl and rl + 1 of the compact layout, each from
// `tree` where the session knows it (known_l / known_r: the child's KNOWN bit, 0 or 1) and from `cand` otherwise.  The base address is
// picked with an integer mask: the two bases differ in the bits the mask lets through.  Without a pair (the last node of an odd layer,
// the one-block slot) the right child is the left row once more, cleared by a limb mask, and the key gets + 2: k_compress_layer's rule.
static_assert(ADOPT_KNOWN == 1 && NODE_KNOWN == 1, "load_children takes the KNOWN bit as 0 or 1");
__device__ __forceinline__ State load_children(const uint4* tree, const uint4* cand, uint32_t known_l, uint32_t known_r, uint64_t rl, bool pair,
                                               uint32_t bottom) {
  const uintptr_t bt = (uintptr_t)tree, bc = (uintptr_t)cand;
  const uintptr_t kl = (uintptr_t)0 - (uintptr_t)known_l, kr = (uintptr_t)0 - (uintptr_t)known_r;
  State s;
  s.x = load_fe_canonical((const uint4*)((bt & kl) | (bc & ~kl)) + 2 * rl);
  s.y = load_fe_canonical((const uint4*)((bt & kr) | (bc & ~kr)) + 2 * (rl + (pair ? 1u : 0u)));
  const uint32_t have = 0u - (pair ? 1u : 0u);
#pragma unroll
  for (int l = 0; l < fr::NL; ++l) s.y.l[l] &= have;
  s.z = key_fe((bottom ? 1u : 0u) + (pair ? 0u : 2u));
  return s;
}

// ------------------------------------------------------------------------------------------------
// Adopting blocks from disk (fill.cpp, cp2_fill_adopt): the tree over the block roots of blocks read back from the slot files, built with
// the session's authentic nodes wherever it has them, and judged against those nodes.  One flag byte per row of the compact layout travels
// with the values: bit 0 the session knows the row (the host sets it, and sets it for every top row: that is the stated slot root), bit 1
// the row has a computed value in `cand`, bit 2 that value equals the kept one.  A node is DEFINED when bit 0 or bit 1 is set; its value is
// the kept row where it is known, the computed one otherwise -- a known node never passes a computed value upward.
//
// k_adopt_layer: one lane per node of layer l + 1 of the n_sel selected slots, one launch per layer (the flags and candidates of layer l
// come from the launch before, earlier on the same stream).  Lane (slot, j) reads the flag bytes of children 2 j and 2 j + 1 of its slot;
// the last node of an odd layer and the one-block slot have one child, a zero sibling and key + 2 (k_compress_layer's rule, key = 1 at
// layer 0 and 0 above).  With both children defined it loads each from `tree` or `cand` (load_children), runs one keyed compression, stores
// the canonical result to its row of `cand` and writes its flag byte: bit 0 as it was, bit 1, and bit 2 where the node is known and the
// result equals its kept row (the top layer: the stated root of its slot).  With an undefined child it writes the flag byte with bits 1 and
// 2 clear and nothing else.  A lane whose rows do not all lie below n_rows (never: the host made the tables) reads and writes
// nothing.  `tree` is only read.  LDS is the QTab only; no atomics.
//
// k_adopt_resolve: one lane per row below the top layer, no permutation, no LDS.  It reads `flags`, `cand` and, for a known row of layer
// 0, that row of `tree`; it writes its own byte of `out` (bits 0-2 as judged, bit 3 proved, bit 4 adopted) and, for a proved row, that
// row of `tree`.  THE LAYER-0 MATCH IS SET HERE: a layer-0 row that is known and has a candidate gets bit 2, and with it bit 4, when its
// 32 candidate bytes equal the kept row; nobody else reads that bit.  A row that is not known and has a candidate walks up its ancestors'
// flag bytes, at most `depth` of them: an ancestor without a computed value ends the walk unproved; the first known one decides it by its
// bit 2.  A proved row is copied from `cand` into `tree` (two 16-byte loads, two 16-byte stores) and gets bit 3, at layer 0 also bit 4.
// Only rows that are not known are written and only known rows of `tree` are read, so no lane reads what another writes.  Rows of slots
// outside the selection, and rows at or past n_rows, are left alone.
__global__ void __launch_bounds__(TPB) k_adopt_layer(const uint4* __restrict__ tree, uint4* cand, uint8_t* flags,
                                                       const uint4* __restrict__ slot_roots, uint64_t off_in, uint64_t m_in, uint64_t off_out,
                                                       uint64_t m_out, uint64_t first_sel, uint64_t n_sel, uint32_t bottom, uint32_t top,
                                                       uint64_t n_rows) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= m_out * n_sel) return;
  const uint64_t seg = t / m_out, j = t - seg * m_out, slot = first_sel + seg;
  const uint64_t rl = off_in + slot * m_in + 2 * j, rp = off_out + slot * m_out + j;
  const bool pair = 2 * j + 1 < m_in;
  if (rl + (pair ? 1u : 0u) >= n_rows || rp >= n_rows) return;
  const uint32_t fl = flags[rl], fr_ = pair ? (uint32_t)flags[rl + 1] : ADOPT_KNOWN;
  const uint32_t fp = flags[rp] & ADOPT_KNOWN;
  if (!(fl & (ADOPT_KNOWN | ADOPT_CAND)) || !(fr_ & (ADOPT_KNOWN | ADOPT_CAND))) {
    flags[rp] = (uint8_t)fp;
    return;
  }
  State s = load_children(tree, cand, fl & ADOPT_KNOWN, fr_ & ADOPT_KNOWN, rl, pair, bottom);
  p2::permute(s, qtab);
  const Fe cur = fr::norm(s.x);
  store_fe_canonical(cand + 2 * rp, cur);
  uint32_t f = fp | ADOPT_CAND;
  if (fp) {
    const Fe want = load_fe_canonical(top ? slot_roots + 2 * slot : tree + 2 * rp);
    f |= fe_equal(cur, want) ? ADOPT_MATCH : 0u;
  }
  flags[rp] = (uint8_t)f;
}

__global__ void __launch_bounds__(TPB) k_adopt_resolve(uint4* tree, const uint4* __restrict__ cand, const uint8_t* __restrict__ flags,
                                                         uint8_t* __restrict__ out, const uint64_t* __restrict__ layer_off,
                                                         const uint64_t* __restrict__ layer_size, uint32_t depth, uint64_t n_local,
                                                         uint64_t first_sel, uint64_t n_sel, uint64_t n_below, uint64_t n_rows) {
  const size_t r = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (r >= n_below || r >= n_rows) return;
  uint32_t lvl = 0;
#pragma unroll 1
  while (lvl + 1 < depth && r >= layer_off[lvl + 1]) ++lvl;   // layer_off ascends; n_below == layer_off[depth]
  uint64_t size = layer_size[lvl];
  const uint64_t in_layer = r - layer_off[lvl], slot = in_layer / size;
  if (slot < first_sel || slot - first_sel >= n_sel || slot >= n_local) return;
  uint64_t k = in_layer - slot * size;
  const uint32_t f = flags[r] & (ADOPT_KNOWN | ADOPT_CAND | ADOPT_MATCH);
  if (!(f & ADOPT_CAND)) {
    out[r] = (uint8_t)f;
    return;
  }
  if (f & ADOPT_KNOWN) {
    uint32_t g = f;
    if (lvl == 0) {
      const bool same = rows_equal(cand[2 * r], cand[2 * r + 1], tree[2 * r], tree[2 * r + 1]);
      g = (f & ~ADOPT_MATCH) | (same ? ADOPT_MATCH | ADOPT_ADOPTED : 0u);
    }
    out[r] = (uint8_t)g;
    return;
  }
  bool proved = false;
#pragma unroll 1
  for (uint32_t up = lvl + 1; up <= depth; ++up) {
    k >>= 1;
    size = layer_size[up];
    const uint64_t ra = layer_off[up] + slot * size + k;
    if (k >= size || ra >= n_rows) break;              // (never: the host made the tables)
    const uint32_t fa = flags[ra];
    if (!(fa & ADOPT_CAND)) break;
    if (fa & ADOPT_KNOWN) {
      proved = (fa & ADOPT_MATCH) != 0;
      break;
    }
  }
  if (proved) copy_row(tree + 2 * r, cand + 2 * r);
  out[r] = (uint8_t)(f | (proved ? ADOPT_PROVED | (lvl == 0 ? ADOPT_ADOPTED : 0u) : 0u));
}

// ------------------------------------------------------------------------------------------------
// Restoring kept nodes from a checkpoint (fill.cpp, cp2_fill_resume_nodes): the rows a checkpoint calls known are candidates until a node
// the resumed session knows vouches for them.  One flag byte per row of the compact layout travels with the values, a row being in one
// state: NODE_KNOWN (the session knows it -- the host sets it, and sets it for every top row: that is the stated slot root), NODE_CAND
// (the row of `cand` holds what the file states), NODE_RESTORED, NODE_REJECTED, or 0 (undefined).
//
// k_nodes_restore_layer: one lane per node p of layer l + 1 of every local slot, one launch per layer, TOP FIRST (the flags and rows of
// layer l + 1 come from the launch before, earlier on the same stream).  p must be known or restored; each child known or a candidate (the
// last node of an odd layer and the one-block slot have one child, a zero sibling and key + 2: k_compress_layer's rule, key = 1 at layer 0
// and 0 above), at least one of them a candidate: a lane with nothing to restore returns before the permutation.  It loads each child from
// `tree` where it is known and from `cand` otherwise (load_children, as k_adopt_layer does), runs one keyed compression and compares the
// canonical result with p's row of `tree` (the top layer: the stated root of its slot).  Equal: every candidate child is stored into `tree`
// in canonical form (two 16-byte stores) and flagged NODE_RESTORED; unequal: flagged NODE_REJECTED, nothing stored.  Only the parent's lane
// writes its children's rows and flag bytes, and a lane reads rows of `tree` only where they are known or restored, so no lane reads what
// another writes in the same launch.  A lane whose rows do not all lie below n_rows (never: the host made the tables) reads and writes
// nothing.  LDS is the QTab only; no atomics.
__global__ void __launch_bounds__(TPB) k_nodes_restore_layer(uint4* tree, const uint4* __restrict__ cand, uint8_t* flags,
                                                               const uint4* __restrict__ slot_roots, uint64_t off_in, uint64_t m_in,
                                                               uint64_t off_out, uint64_t m_out, uint64_t n_local, uint32_t bottom, uint32_t top,
                                                               uint64_t n_rows) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= m_out * n_local) return;
  const uint64_t slot = t / m_out, j = t - slot * m_out;
  const uint64_t rl = off_in + slot * m_in + 2 * j, rp = off_out + slot * m_out + j;
  const bool pair = 2 * j + 1 < m_in;
  const uint64_t rr = rl + (pair ? 1u : 0u);
  if (rr >= n_rows || rp >= n_rows) return;
  if (!(flags[rp] & (NODE_KNOWN | NODE_RESTORED))) return;
  const uint32_t fl = flags[rl], fr_ = pair ? (uint32_t)flags[rr] : NODE_KNOWN;
  if (!(fl & (NODE_KNOWN | NODE_CAND)) || !(fr_ & (NODE_KNOWN | NODE_CAND)) || !((fl | fr_) & NODE_CAND)) return;
  State s = load_children(tree, cand, fl & NODE_KNOWN, fr_ & NODE_KNOWN, rl, pair, bottom);
  p2::permute(s, qtab);
  const Fe cur = fr::norm(s.x);
  const Fe want = load_fe_canonical(top ? slot_roots + 2 * slot : (const uint4*)tree + 2 * rp);
  const bool ok = fe_equal(cur, want);
  if (fl & NODE_CAND) {
    if (ok) store_fe_canonical(tree + 2 * rl, load_fe_canonical(cand + 2 * rl));
    flags[rl] = ok ? NODE_RESTORED : NODE_REJECTED;
  }
  if (pair && (fr_ & NODE_CAND)) {
    if (ok) store_fe_canonical(tree + 2 * rr, load_fe_canonical(cand + 2 * rr));
    flags[rr] = ok ? NODE_RESTORED : NODE_REJECTED;
  }
}

// ------------------------------------------------------------------------------------------------
// Workgroups for n work items.  A grid holds at most 2^31 - 1 workgroups in x; the per-item kernels are launched in slices of
// at most MAX_ITEMS items (every item is independent and addressed from a base pointer), the layer / sampling kernels, whose
// item index is decomposed inside the kernel, refuse what does not fit one grid (2^38 nodes: far beyond any HBM).
// hipGetLastError() returns (and clears) the last error of ANY earlier runtime call of this thread, e.g. a hipMalloc that failed
// and was already reported to the caller: clear it before a launch so that the status read after the launch is the launch's own.
#define CP2K_LAUNCH(...) do { (void)hipGetLastError(); hipLaunchKernelGGL(__VA_ARGS__); } while (0)
constexpr size_t MAX_BLOCKS = (size_t)1 << 30;
constexpr size_t MAX_ITEMS = MAX_BLOCKS * TPB;
static inline bool fits_one_grid(size_t n) { return (n + TPB - 1) / TPB <= MAX_BLOCKS; }
static inline unsigned grid_for(size_t n) { return (unsigned)((n + TPB - 1) / TPB); }   // n <= MAX_ITEMS

// launch(i0, m) for every slice [i0, i0 + m) of n items, m <= max_items; each launch between a cleared error and a read of its own, as in
// CP2K_LAUNCH.  Stops at the first launch that fails.
template <typename F>
static inline hipError_t for_slices(size_t n, F launch, size_t max_items = MAX_ITEMS) {
  for (size_t i0 = 0; i0 < n; i0 += max_items) {
    (void)hipGetLastError();
    launch(i0, n - i0 < max_items ? n - i0 : max_items);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Whether host tables of depth + 1 entries describe a compact layout of n_local slots, which the layer kernels derive every row from:
// each layer half the one below (rounded up) down to a single root, the layers of all slots one after the other.
static inline bool is_compact_layout(const uint64_t* layer_off_host, const uint64_t* layer_size_host, uint32_t depth, uint64_t n_local) {
  for (uint32_t l = 0; l < depth; ++l) {
    const uint64_t m_in = layer_size_host[l];
    if (m_in == 0 || layer_size_host[l + 1] != (m_in + 1) / 2 || layer_off_host[l + 1] != layer_off_host[l] + n_local * m_in) return false;
  }
  return layer_size_host[depth] == 1;
}

hipError_t launch_permute_batch(const void* in, void* out, size_t n, hipStream_t st) {
  return for_slices(n, [&](size_t i0, size_t m) {
    hipLaunchKernelGGL(k_permute_batch, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)in + 6 * i0, (uint4*)out + 6 * i0, m);
  });
}

hipError_t launch_compress_layer(const void* in, void* out, size_t m_in, size_t nseg, bool bottom,
                                 size_t in_seg_stride, size_t out_seg_stride, hipStream_t st) {
  size_t m_out = (m_in + 1) / 2;
  if (m_out * nseg == 0) return hipSuccess;
  if (!fits_one_grid(m_out * nseg)) return hipErrorInvalidValue;
  CP2K_LAUNCH(k_compress_layer, dim3(grid_for(m_out * nseg)), dim3(TPB), 0, st, (const uint4*)in, (uint4*)out,
                     m_in, m_out, nseg, bottom ? 1u : 0u, in_seg_stride, out_seg_stride);
  return hipGetLastError();
}

hipError_t launch_compress_layers_ragged(void* rows, const uint64_t* tree_tab, const uint64_t* prefix, const uint32_t* tree_of,
                                         const uint64_t* level_off, const uint64_t* level_cnt, const uint64_t* level_work, size_t n_levels,
                                         hipStream_t st) {
  size_t work = 0;
  if (n_levels && (!level_off || !level_cnt || !level_work)) return hipErrorInvalidValue;
  for (size_t k = 0; k < n_levels; ++k) {
    if (level_work[k] && (level_cnt[k] == 0 || level_cnt[k] > 0xffffffffull || !fits_one_grid(level_work[k]))) return hipErrorInvalidValue;
    work += level_work[k];
  }
  if (work == 0) return hipSuccess;
  if (!rows || !tree_tab || !prefix || !tree_of || n_levels > 63) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(rows) & 15) || (reinterpret_cast<uintptr_t>(tree_tab) & 7) || (reinterpret_cast<uintptr_t>(prefix) & 7) ||
      (reinterpret_cast<uintptr_t>(tree_of) & 3))
    return hipErrorInvalidValue;
  for (size_t k = 0; k < n_levels; ++k) {                    // in order on st: level k + 1 reads what level k wrote
    if (level_work[k] == 0) continue;
    uint32_t trips = 0;
    while (((uint64_t)1 << trips) < level_cnt[k]) ++trips;
    CP2K_LAUNCH(k_compress_layer_ragged, dim3(grid_for(level_work[k])), dim3(TPB), 0, st, (uint4*)rows, tree_tab, prefix + level_off[k],
                tree_of + level_off[k], (uint32_t)level_cnt[k], trips, (uint32_t)k, (size_t)level_work[k]);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_finish_layers_many(const FillManySession* sessions, uint64_t n_sessions, const uint64_t* voff, const uint64_t* prefix,
                                     const uint32_t* sess_of, const uint64_t* level_off, const uint64_t* level_cnt, const uint64_t* level_work,
                                     size_t n_levels, uint32_t* verdict, hipStream_t st) {
  size_t work = 0;
  if (n_levels && (!level_off || !level_cnt || !level_work)) return hipErrorInvalidValue;
  for (size_t k = 0; k < n_levels; ++k) {
    if (level_work[k] && (level_cnt[k] == 0 || level_cnt[k] > 0xffffffffull || !fits_one_grid(level_work[k]))) return hipErrorInvalidValue;
    work += level_work[k];
  }
  if (work == 0) return hipSuccess;
  if (!sessions || !voff || !prefix || !sess_of || !verdict || n_sessions == 0 || n_sessions > 0xffffffffull || n_levels > 63)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(sessions) & 7) || (reinterpret_cast<uintptr_t>(voff) & 7) || (reinterpret_cast<uintptr_t>(prefix) & 7) ||
      (reinterpret_cast<uintptr_t>(sess_of) & 3) || (reinterpret_cast<uintptr_t>(verdict) & 3))
    return hipErrorInvalidValue;
  for (size_t k = 0; k < n_levels; ++k) {                    // in order on st: level k + 1 reads what level k wrote
    if (level_work[k] == 0) continue;
    uint32_t trips = 0;
    while (((uint64_t)1 << trips) < level_cnt[k]) ++trips;
    CP2K_LAUNCH(k_finish_layer_many, dim3(grid_for(level_work[k])), dim3(TPB), 0, st, sessions, n_sessions, voff, prefix + level_off[k],
                sess_of + level_off[k], (uint32_t)level_cnt[k], trips, (uint32_t)k, (size_t)level_work[k], verdict);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_multiproof_layers(void* work, uint64_t n_work, const MultiproofJob* jobs, const uint64_t* level_off, const uint64_t* level_base,
                                    size_t n_levels, const uint64_t* want_addr, uint32_t* verdict, hipStream_t st) {
  if (n_levels == 0) return hipSuccess;
  if (!level_off || !level_base || n_levels > 63) return hipErrorInvalidValue;
  uint64_t top = 0;                                           // the rows below every level's output: no level writes what it may read
  for (size_t k = 0; k < n_levels; ++k) {
    if (level_off[k + 1] < level_off[k]) return hipErrorInvalidValue;
    const uint64_t cnt = level_off[k + 1] - level_off[k];
    if (cnt == 0) continue;
    if (!fits_one_grid(cnt) || level_base[k] < top || level_base[k] >= MULTIPROOF_ZERO || cnt >= MULTIPROOF_ZERO - level_base[k])
      return hipErrorInvalidValue;
    top = level_base[k] + cnt;
  }
  if (top == 0) return hipSuccess;
  if (!work || !jobs || !want_addr || !verdict || top > n_work) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(work) & 15) || (reinterpret_cast<uintptr_t>(jobs) & 15) || (reinterpret_cast<uintptr_t>(want_addr) & 7) ||
      (reinterpret_cast<uintptr_t>(verdict) & 3))
    return hipErrorInvalidValue;
  for (size_t k = 0; k < n_levels; ++k) {                    // in order on st: level k + 1 reads what level k wrote
    const uint64_t cnt = level_off[k + 1] - level_off[k];
    if (cnt == 0) continue;
    CP2K_LAUNCH(k_multiproof_layer, dim3(grid_for(cnt)), dim3(TPB), 0, st, (uint4*)work, jobs + level_off[k], (size_t)cnt, level_base[k], want_addr,
                verdict);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_multiproof_commit(const void* work, uint64_t n_work, const uint32_t* src_row, const uint64_t* dst_addr, const uint32_t* group_of,
                                    const uint32_t* verdict, uint32_t n_groups, size_t n, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!work || !src_row || !dst_addr || !group_of || !verdict) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(work) & 15) || (reinterpret_cast<uintptr_t>(src_row) & 3) || (reinterpret_cast<uintptr_t>(dst_addr) & 7) ||
      (reinterpret_cast<uintptr_t>(group_of) & 3) || (reinterpret_cast<uintptr_t>(verdict) & 3))
    return hipErrorInvalidValue;
  return for_slices(n, [&](size_t i0, size_t m) {
    hipLaunchKernelGGL(k_multiproof_commit, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)work, n_work, src_row + i0, dst_addr + i0, group_of + i0,
                       verdict, n_groups, m);
  });
}

hipError_t launch_multiproof_tops(const void* work, uint64_t n_work, const MultiproofTop* tops, const uint64_t* want_addr, size_t n_tops,
                                  const uint64_t* top_off, const uint64_t* d_top_off, size_t n_groups, uint32_t* top_verdict, uint32_t* verdict,
                                  hipStream_t st) {
  if (n_groups == 0) return hipSuccess;
  if (!top_off || !d_top_off || !verdict || !fits_one_grid(n_groups) || (n_tops && !fits_one_grid(n_tops))) return hipErrorInvalidValue;
  for (size_t g = 0; g < n_groups; ++g)
    if (top_off[g + 1] < top_off[g]) return hipErrorInvalidValue;
  if (top_off[n_groups] > n_tops) return hipErrorInvalidValue;
  if (n_tops && (!work || !tops || !want_addr || !top_verdict)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(work) & 15) || (reinterpret_cast<uintptr_t>(tops) & 7) || (reinterpret_cast<uintptr_t>(want_addr) & 7) ||
      (reinterpret_cast<uintptr_t>(d_top_off) & 7) || (reinterpret_cast<uintptr_t>(top_verdict) & 3) || (reinterpret_cast<uintptr_t>(verdict) & 3))
    return hipErrorInvalidValue;
  if (n_tops) {
    CP2K_LAUNCH(k_multiproof_tops, dim3(grid_for(n_tops)), dim3(TPB), 0, st, (const uint4*)work, n_work, tops, want_addr, n_tops, top_verdict);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  CP2K_LAUNCH(k_multiproof_fold, dim3(grid_for(n_groups)), dim3(TPB), 0, st, top_verdict, n_tops, d_top_off, n_groups, verdict);
  return hipGetLastError();
}

hipError_t launch_compress_pairs(const void* xy, uint32_t key, void* out, size_t n, hipStream_t st) {
  return for_slices(n, [&](size_t i0, size_t m) {
    hipLaunchKernelGGL(k_compress_pairs, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)xy + 4 * i0, key, (uint4*)out + 2 * i0, m);
  });
}

hipError_t launch_sponge2_felts(const void* felts, size_t nf, size_t nitems, void* out, hipStream_t st) {
  return for_slices(nitems, [&](size_t i0, size_t m) {
    hipLaunchKernelGGL(k_sponge2_felts, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)felts + 2 * nf * i0, nf, m, (uint4*)out + 2 * i0);
  });
}

// Workgroup size of k_hash_cells: 256 unless CP2_HASH_BLOCK=64 is in the environment (A/B tooling only).
static int hash_block_override() {
  static const int v = [] {
    const char* e = std::getenv("CP2_HASH_BLOCK");
    const int x = e ? std::atoi(e) : 0;
    return (x == 64 || x == 256) ? x : 0;
  }();
  return v;
}

// leave_room: 28 KiB of dynamic LDS nobody uses, so that TWO workgroups fit a CU instead of three.  The kernel itself loses under 1 %
// (issue bound from two waves per SIMD up), and the third of every CU it no longer holds is where the small dependent kernels of the
// streamed build -- a group's layer passes, its sampling and gathers -- run beside it: next to a launch that holds every workgroup
// slot such a chain finishes only when the launch drains (tools/coresidency_probe.cpp, profiles/r05_coresidency_probe.txt).
// Whether a device takes the larger request is decided ONCE, when a context is made on it (hash_cells_can_leave_room, called by
// cp2_init; the callers pass leave_room only where it said yes): a launch is never retried, so an error at a launch is that launch's.
constexpr unsigned HASH_ROOM_BYTES = 28672;

bool hash_cells_can_leave_room(size_t lds_cap, std::string* why) {
  int dev = 0, max_lds = 0;
  hipFuncAttributes fa;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
  if (e == hipSuccess) e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_hash_cells<CP2_HASH_BT>));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (why) *why = std::string("the device could not be asked (") + hipGetErrorString(e) + ")";
    return false;
  }
  const size_t limit = lds_cap ? std::min<size_t>(lds_cap, (size_t)max_lds) : (size_t)max_lds;
  if (fa.sharedSizeBytes + HASH_ROOM_BYTES > limit) {
    if (why) *why = "the kernel's " + std::to_string(fa.sharedSizeBytes) + " B of LDS + " + std::to_string(HASH_ROOM_BYTES) + " B exceed the " + std::to_string(limit) + " B a workgroup may hold";
    return false;
  }
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_hash_cells<CP2_HASH_BT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)HASH_ROOM_BYTES);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (why) *why = std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize) refused (") + hipGetErrorString(e) + ")";
    return false;
  }
  if (why) *why = std::to_string(fa.sharedSizeBytes) + " + " + std::to_string(HASH_ROOM_BYTES) + " B of " + std::to_string(limit) + " B per workgroup";
  return true;
}

hipError_t launch_hash_cells_block(int block, const void* cells, size_t cell_size, size_t n_cells, void* out, hipStream_t st, bool leave_room) {
  if (block != 64 && block != 256) return hipErrorInvalidValue;
  if (block == 256) block = CP2_HASH_BT;
  const unsigned dyn = (leave_room && block != 64) ? HASH_ROOM_BYTES : 0u;
  return for_slices(n_cells, [&](size_t i0, size_t m) {
    const unsigned grid = (unsigned)((m + block - 1) / block);
    const uint8_t* src = (const uint8_t*)cells + i0 * cell_size;
    if (block == 64) hipLaunchKernelGGL(k_hash_cells<64>, dim3(grid), dim3(64), 0, st, src, cell_size, m, (uint4*)out + 2 * i0);
    else hipLaunchKernelGGL(k_hash_cells<CP2_HASH_BT>, dim3(grid), dim3(CP2_HASH_BT), dyn, st, src, cell_size, m, (uint4*)out + 2 * i0);
  }, MAX_BLOCKS * (size_t)block);
}

hipError_t launch_hash_cells(const void* cells, size_t cell_size, size_t n_cells, void* out, hipStream_t st, bool leave_room) {
  const int block = hash_block_override();
  return launch_hash_cells_block(block ? block : 256, cells, cell_size, n_cells, out, st, leave_room);
}

hipError_t launch_gen_fake_cells(uint64_t seed0, uint64_t cells_per_slot, uint64_t first, const uint64_t* list,
                                 size_t n_cells, size_t cell_size, void* out, hipStream_t st, uint64_t units_per_slot, uint64_t first_unit) {
  if (n_cells == 0 || cell_size == 0) return hipSuccess;
  if (!fits_one_grid(n_cells)) return hipErrorInvalidValue;
  CP2K_LAUNCH(k_gen_fake_cells, dim3(grid_for(n_cells)), dim3(TPB), 0, st, seed0, cells_per_slot, first, list,
                     n_cells, cell_size, (uint8_t*)out, units_per_slot, first_unit);
  return hipGetLastError();
}

hipError_t launch_sample_paths(const TreeGeom& g, const void* nodes, const void* d_entropy, const uint64_t* slots, uint64_t slot0,
                               size_t n_items, uint32_t ns, uint32_t md, uint64_t* indices, uint64_t* gcell, uint64_t* rows,
                               hipStream_t st) {
  if (n_items == 0 || ns == 0) return hipSuccess;
  if (!fits_one_grid(n_items * ns)) return hipErrorInvalidValue;
  CP2K_LAUNCH(k_sample_paths, dim3(grid_for(n_items * ns)), dim3(TPB), 0, st, g, (const uint4*)nodes, (const uint4*)d_entropy,
                     slots, slot0, n_items, ns, md, indices, gcell, rows);
  return hipGetLastError();
}

// the gathers' grid: one lane per word up to 4096 workgroups, round the grid-stride loop above that
static inline unsigned gather_grid(size_t words) { return words > (size_t)4096 * TPB ? 4096u : grid_for(words); }

hipError_t launch_gather_rows(const void* src, const uint64_t* index, size_t nrows, size_t row_bytes, void* out, hipStream_t st) {
  if (nrows == 0) return hipSuccess;
  // the kernel moves whole 32-bit words: a row length or a pointer that is no multiple of four is refused, not truncated
  if ((row_bytes & 3) != 0 || ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 3) != 0) return hipErrorInvalidValue;
  CP2K_LAUNCH(k_gather_rows, dim3(gather_grid(nrows * (row_bytes / 4))), dim3(TPB), 0, st, (const uint8_t*)src, index, nrows, row_bytes, (uint8_t*)out);
  return hipGetLastError();
}

hipError_t launch_sample_many(const ManyReq* reqs, const TreeGeom* geoms, size_t n_req, uint32_t ns, uint32_t md, uint64_t* indices,
                              uint64_t* blocks, uint64_t* addr, hipStream_t st) {
  if (n_req == 0 || ns == 0) return hipSuccess;
  if (!fits_one_grid(n_req * ns)) return hipErrorInvalidValue;
  CP2K_LAUNCH(k_sample_many, dim3(grid_for(n_req * ns)), dim3(TPB), 0, st, reqs, geoms, n_req, ns, md, indices, blocks, addr);
  return hipGetLastError();
}

hipError_t launch_gather_addr(const uint64_t* addr, size_t nrows, size_t row_bytes, void* out, hipStream_t st) {
  if (nrows == 0 || row_bytes == 0) return hipSuccess;
  const bool words = (row_bytes & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;   // (the callers' addresses are row multiples)
  const unsigned grid = gather_grid(nrows * (words ? row_bytes / 4 : row_bytes));
  if (words) CP2K_LAUNCH(k_gather_addr<uint32_t>, dim3(grid), dim3(TPB), 0, st, addr, nrows, row_bytes, (uint8_t*)out);
  else CP2K_LAUNCH(k_gather_addr<uint8_t>, dim3(grid), dim3(TPB), 0, st, addr, nrows, row_bytes, (uint8_t*)out);
  return hipGetLastError();
}

hipError_t launch_gen_fake_cells_many(const uint64_t* seeds, const uint64_t* firsts, uint64_t per, size_t n_rows, size_t cell_size,
                                      void* out, hipStream_t st) {
  if (n_rows == 0 || cell_size == 0) return hipSuccess;
  if (per == 0 || !fits_one_grid(n_rows)) return hipErrorInvalidValue;
  CP2K_LAUNCH(k_gen_fake_cells_many, dim3(grid_for(n_rows)), dim3(TPB), 0, st, seeds, firsts, per, n_rows, cell_size, (uint8_t*)out);
  return hipGetLastError();
}

hipError_t launch_scrub_compare(const void* fresh, size_t fstride, const void* kept, size_t kstride, size_t rows, size_t n_items,
                                uint64_t* bits, uint32_t* counts, hipStream_t st) {
  if (n_items == 0 || rows == 0) return hipSuccess;
  if (!fresh || !kept || !bits || !counts || fstride < rows || kstride < rows) return hipErrorInvalidValue;
  const size_t total = n_items * rows, groups = scrub_groups(total);
  if (groups > MAX_BLOCKS) return hipErrorInvalidValue;
  CP2K_LAUNCH(k_scrub_compare, dim3((unsigned)groups), dim3(TPB), 0, st, (const uint4*)fresh, fstride, (const uint4*)kept, kstride, rows, total,
              (unsigned long long*)bits, counts);
  return hipGetLastError();
}

hipError_t launch_scrub_compare_many(const void* fresh, size_t fstride, const uint64_t* kept_addr, size_t rows, size_t n_items, uint64_t* bits,
                                     uint32_t* counts, hipStream_t st) {
  if (n_items == 0 || rows == 0) return hipSuccess;
  if (!fresh || !kept_addr || !bits || !counts || fstride < rows) return hipErrorInvalidValue;
  const size_t total = n_items * rows, groups = scrub_groups(total);
  if (groups > MAX_BLOCKS) return hipErrorInvalidValue;
  CP2K_LAUNCH(k_scrub_compare_many, dim3((unsigned)groups), dim3(TPB), 0, st, (const uint4*)fresh, fstride, kept_addr, rows, total,
              (unsigned long long*)bits, counts);
  return hipGetLastError();
}

hipError_t launch_scatter_rows_addr(const void* src, size_t sstride, const uint64_t* dst_addr, size_t rows, size_t n_items, hipStream_t st,
                                    size_t slice) {
  if (n_items == 0 || rows == 0) return hipSuccess;
  if (!src || !dst_addr || sstride < rows) return hipErrorInvalidValue;
  return for_slices(rows * n_items, [&](size_t g0, size_t m) {
    hipLaunchKernelGGL(k_scatter_rows_addr, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)src, sstride, dst_addr, rows, g0, m);
  }, slice && slice < MAX_ITEMS ? slice : MAX_ITEMS);
}

hipError_t launch_repair_compare(const void* fresh, const void* kept, size_t kept_rows, const uint64_t* rows, size_t n, uint32_t* verdict,
                                 hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!fresh || !kept || !rows || !verdict || !fits_one_grid(n)) return hipErrorInvalidValue;
  CP2K_LAUNCH(k_repair_compare, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, st, (const uint4*)fresh, (const uint4*)kept, kept_rows, rows, n,
              verdict);
  return hipGetLastError();
}

hipError_t launch_repair_compare_addr(const void* fresh, const uint64_t* kept_addr, size_t n, uint32_t* verdict, hipStream_t st, size_t slice) {
  if (n == 0) return hipSuccess;
  if (!fresh || !kept_addr || !verdict) return hipErrorInvalidValue;
  return for_slices(n, [&](size_t i0, size_t m) {
    hipLaunchKernelGGL(k_repair_compare_addr, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)fresh + 2 * i0, kept_addr + i0, m, verdict + i0);
  }, slice && slice < MAX_ITEMS ? slice : MAX_ITEMS);
}

hipError_t launch_block_path_roots(const void* fresh, const void* paths, const uint64_t* root_block, const void* slot_roots, uint64_t n_blocks,
                                   uint32_t depth, size_t n, uint32_t* verdict, void* roots_out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!fresh || !paths || !root_block || !slot_roots || !verdict || depth == 0 || n_blocks == 0) return hipErrorInvalidValue;
  return for_slices(n, [&](size_t i0, size_t m) {
    hipLaunchKernelGGL(k_block_path_roots, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)fresh + 2 * i0, (const uint4*)paths + 2 * i0 * depth,
                root_block + 2 * i0, (const uint4*)slot_roots, n_blocks, depth, m, verdict + i0, roots_out ? (uint4*)roots_out + 2 * i0 : nullptr);
  });
}

hipError_t launch_repair_judge_many(const void* fresh, const void* paths, const RepairManyReq* reqs, size_t n, uint32_t* verdict, hipStream_t st,
                                    size_t slice) {
  if (n == 0) return hipSuccess;
  if (!fresh || !reqs || !verdict) return hipErrorInvalidValue;
  return for_slices(n, [&](size_t i0, size_t m) {     // path_at is relative to `paths`, which stays where it is
    hipLaunchKernelGGL(k_repair_judge_many, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)fresh + 2 * i0, (const uint4*)paths, reqs + i0, m,
                       verdict + i0);
  }, slice && slice < MAX_ITEMS ? slice : MAX_ITEMS);
}

hipError_t launch_block_path_commit(const void* fresh, const void* paths, const uint64_t* slot_block, const void* slot_roots, const uint64_t* dest,
                                    uint64_t n_blocks, uint32_t depth, size_t n, uint32_t* verdict, void* layer0, uint64_t n_rows, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!fresh || !paths || !slot_block || !slot_roots || !dest || !verdict || !layer0 || depth == 0 || n_blocks == 0) return hipErrorInvalidValue;
  return for_slices(n, [&](size_t i0, size_t m) {
    hipLaunchKernelGGL(k_block_path_commit, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)fresh + 2 * i0, (const uint4*)paths + 2 * i0 * depth,
                slot_block + 2 * i0, (const uint4*)slot_roots, dest + i0, n_blocks, depth, m, verdict + i0, (uint4*)layer0, n_rows);
  });
}

hipError_t launch_block_path_commit_nodes(const void* fresh, const void* paths, const uint64_t* slot_block, const void* slot_roots,
                                          const uint64_t* dest, const uint64_t* layer_off, const uint64_t* layer_size, uint64_t n_blocks,
                                          uint32_t depth, size_t n, uint32_t* verdict, void* tree, uint64_t n_rows, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!fresh || !paths || !slot_block || !slot_roots || !dest || !layer_off || !layer_size || !verdict || !tree || !scratch || depth == 0 ||
      n_blocks == 0)
    return hipErrorInvalidValue;
  return for_slices(n, [&](size_t i0, size_t m) {
    hipLaunchKernelGGL(k_block_path_commit_nodes, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)fresh + 2 * i0, (const uint4*)paths + 2 * i0 * depth,
                slot_block + 2 * i0, (const uint4*)slot_roots, dest + i0, layer_off, layer_size, n_blocks, depth, m, verdict + i0, (uint4*)tree,
                n_rows, (uint4*)scratch + 4 * i0 * depth);
  });
}

hipError_t launch_block_path_commit_anchored(const void* fresh, const void* paths, const uint32_t* levels, const uint64_t* path_off,
                                             uint64_t path_base, const uint64_t* slot_block, const void* slot_roots, const uint64_t* dest,
                                             const uint64_t* anchor_row, const uint64_t* layer_off, const uint64_t* layer_size,
                                             uint64_t n_blocks, uint32_t depth, size_t n, uint32_t* verdict, void* tree, uint64_t n_rows,
                                             void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!fresh || !paths || !levels || !path_off || !slot_block || !slot_roots || !dest || !anchor_row || !layer_off || !layer_size || !verdict ||
      !tree || !scratch || depth == 0 || n_blocks == 0)
    return hipErrorInvalidValue;
  return for_slices(n, [&](size_t i0, size_t m) {     // path_off is absolute: `paths` and `scratch` stay where they are
    hipLaunchKernelGGL(k_block_path_commit_anchored, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)fresh + 2 * i0, (const uint4*)paths, levels + i0,
                path_off + i0, path_base, slot_block + 2 * i0, (const uint4*)slot_roots, dest + i0, anchor_row + i0, layer_off, layer_size, n_blocks,
                depth, m, verdict + i0, (uint4*)tree, n_rows, (uint4*)scratch);
  });
}

hipError_t launch_block_path_commit_many(const void* fresh, const void* paths, const FillManySession* sessions, uint64_t n_sessions,
                                         const uint64_t* session_of, const uint32_t* levels, const uint64_t* path_off, uint64_t path_base,
                                         const uint64_t* slot_block, const uint64_t* dest, const uint64_t* anchor_row, bool keep_top, size_t n,
                                         uint32_t* verdict, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!fresh || !paths || !sessions || !session_of || !levels || !path_off || !slot_block || !dest || !anchor_row || !verdict || !scratch ||
      n_sessions == 0)
    return hipErrorInvalidValue;
  return for_slices(n, [&](size_t i0, size_t m) {     // path_off is absolute: `paths` and `scratch` stay where they are
    hipLaunchKernelGGL(k_block_path_commit_many, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)fresh + 2 * i0, (const uint4*)paths, sessions,
                n_sessions, session_of + i0, levels + i0, path_off + i0, path_base, slot_block + 2 * i0, dest + i0, anchor_row + i0,
                keep_top ? 1u : 0u, m, verdict + i0, (uint4*)scratch);
  });
}

hipError_t launch_block_root_recheck(const void* fresh, const uint64_t* dest, size_t n, uint32_t* verdict, void* layer0, uint64_t n_rows,
                                     hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!fresh || !dest || !verdict || !layer0) return hipErrorInvalidValue;
  return for_slices(n, [&](size_t i0, size_t m) {
    hipLaunchKernelGGL(k_block_root_recheck, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)fresh + 2 * i0, dest + i0, m, verdict + i0, (uint4*)layer0,
                n_rows);
  });
}

hipError_t launch_block_root_recheck_addr(const void* fresh, const uint64_t* addr, size_t n, uint32_t* verdict, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!fresh || !addr || !verdict) return hipErrorInvalidValue;
  return for_slices(n, [&](size_t i0, size_t m) {
    hipLaunchKernelGGL(k_block_root_recheck_addr, dim3(grid_for(m)), dim3(TPB), 0, st, (const uint4*)fresh + 2 * i0, addr + i0, m, verdict + i0);
  });
}

hipError_t launch_adopt_layers(const void* tree, void* cand, uint8_t* flags, const void* slot_roots, const uint64_t* layer_off_host,
                               const uint64_t* layer_size_host, uint32_t depth, uint64_t n_local, uint64_t first_sel, uint64_t n_sel, uint64_t n_rows,
                               hipStream_t st) {
  if (n_sel == 0) return hipSuccess;
  if (!tree || !cand || !flags || !slot_roots || !layer_off_host || !layer_size_host || depth == 0 || first_sel > n_local ||
      n_sel > n_local - first_sel)
    return hipErrorInvalidValue;
  if (!is_compact_layout(layer_off_host, layer_size_host, depth, n_local)) return hipErrorInvalidValue;
  for (uint32_t l = 1; l <= depth; ++l)
    if (!fits_one_grid(layer_size_host[l] * n_sel)) return hipErrorInvalidValue;
  for (uint32_t l = 0; l < depth; ++l) {
    const uint64_t m_out = layer_size_host[l + 1];
    CP2K_LAUNCH(k_adopt_layer, dim3(grid_for(m_out * n_sel)), dim3(TPB), 0, st, (const uint4*)tree, (uint4*)cand, flags, (const uint4*)slot_roots,
                layer_off_host[l], layer_size_host[l], layer_off_host[l + 1], m_out, first_sel, n_sel, l == 0 ? 1u : 0u, l + 1 == depth ? 1u : 0u,
                n_rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_adopt_resolve(void* tree, const void* cand, const uint8_t* flags, uint8_t* out, const uint64_t* layer_off,
                                const uint64_t* layer_size, uint32_t depth, uint64_t n_local, uint64_t first_sel, uint64_t n_sel, uint64_t n_below,
                                uint64_t n_rows, hipStream_t st) {
  if (n_sel == 0 || n_below == 0) return hipSuccess;
  if (!tree || !cand || !flags || !out || !layer_off || !layer_size || depth == 0 || first_sel > n_local || n_sel > n_local - first_sel ||
      !fits_one_grid(n_below))
    return hipErrorInvalidValue;
  CP2K_LAUNCH(k_adopt_resolve, dim3(grid_for(n_below)), dim3(TPB), 0, st, (uint4*)tree, (const uint4*)cand, flags, out, layer_off, layer_size, depth,
              n_local, first_sel, n_sel, n_below, n_rows);
  return hipGetLastError();
}

hipError_t launch_nodes_restore_layer(void* tree, const void* cand, uint8_t* flags, const void* slot_roots, uint64_t off_in, uint64_t m_in,
                                      uint64_t off_out, uint64_t n_local, bool bottom, bool top, uint64_t n_rows, hipStream_t st) {
  if (n_local == 0) return hipSuccess;
  if (!tree || !cand || !flags || !slot_roots || m_in == 0) return hipErrorInvalidValue;
  const uint64_t m_out = (m_in + 1) / 2;
  if (!fits_one_grid(m_out * n_local)) return hipErrorInvalidValue;
  CP2K_LAUNCH(k_nodes_restore_layer, dim3(grid_for(m_out * n_local)), dim3(TPB), 0, st, (uint4*)tree, (const uint4*)cand, flags,
              (const uint4*)slot_roots, off_in, m_in, off_out, m_out, n_local, bottom ? 1u : 0u, top ? 1u : 0u, n_rows);
  return hipGetLastError();
}

hipError_t launch_nodes_restore_layers(void* tree, const void* cand, uint8_t* flags, const void* slot_roots, const uint64_t* layer_off_host,
                                       const uint64_t* layer_size_host, uint32_t depth, uint64_t n_local, uint64_t n_rows, hipStream_t st) {
  if (n_local == 0) return hipSuccess;
  if (!tree || !cand || !flags || !slot_roots || !layer_off_host || !layer_size_host || depth == 0) return hipErrorInvalidValue;
  if (!is_compact_layout(layer_off_host, layer_size_host, depth, n_local)) return hipErrorInvalidValue;
  for (uint32_t l = 1; l <= depth; ++l)
    if (!fits_one_grid(layer_size_host[l] * n_local)) return hipErrorInvalidValue;
  for (uint32_t l = depth; l-- > 0;) {                 // top first: a restored node vouches for its children in the next launch
    hipError_t e = launch_nodes_restore_layer(tree, cand, flags, slot_roots, layer_off_host[l], layer_size_host[l], layer_off_host[l + 1], n_local,
                                              l == 0, l + 1 == depth, n_rows, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_verify_samples(const VerifyGeom& g, const uint64_t* prm, const void* heads, const void* cells, const void* paths,
                                 uint8_t* ok, hipStream_t st) {
  const size_t lanes = g.n * g.ns + g.n;
  if (lanes == 0) return hipSuccess;
  if (!fits_one_grid(lanes)) return hipErrorInvalidValue;
  CP2K_LAUNCH(k_verify_samples, dim3(grid_for(lanes)), dim3(TPB), 0, st, g, prm, (const uint4*)heads, (const uint4*)cells,
              (const uint4*)paths, ok);
  return hipGetLastError();
}

}  // namespace cp2k
