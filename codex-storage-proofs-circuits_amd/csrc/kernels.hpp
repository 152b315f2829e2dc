// Launch wrappers of the HIP kernels in kernels.hip (device pointers, asynchronous on `st`).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace cp2k {

// Kernel-argument copy of the layer-major node layout of a batch of slot trees (proof_input.cpp, trees_layout):
// block-tree layer k of block b of slot s starts at element boff[k] + (s * nblocks + b) * bsz[k]; big-tree layer k
// of slot s at toff[k] + s * tsz[k]; the last big-tree layer holds the slot roots.
struct TreeGeom {
  static constexpr int MAX_LAYERS = 40;
  uint32_t nb, nt;                      // layer counts (leaves included) of a block tree / a big tree
  uint64_t cpb, nblocks, n_cells;
  uint64_t boff[MAX_LAYERS], bsz[MAX_LAYERS], toff[MAX_LAYERS], tsz[MAX_LAYERS];
};

hipError_t launch_permute_batch(const void* in, void* out, size_t n, hipStream_t st);
// one Merkle layer of nseg trees; segment strides are in field elements
hipError_t launch_compress_layer(const void* in, void* out, size_t m_in, size_t nseg, bool bottom,
                                 size_t in_seg_stride, size_t out_seg_stride, hipStream_t st);
// Every layer of many trees of different leaf counts, tree-major in `rows` (16-byte aligned), one launch per level in order on st
// (k_compress_layer_ragged; the tables are set_roots_plan.hpp's).  Device: tree_tab (first row and leaf count of tree r at [2 r],
// [2 r + 1]), prefix and tree_of (per level k the entries [level_off[k], + level_cnt[k]): the trees that have a layer k + 1 and the
// running sum of those layers' sizes).  Host: level_off, level_cnt, level_work (the lanes of level k: its last prefix), n_levels entries
// each.  The leaves are read, every other row of every tree is written, nothing else.  hipErrorInvalidValue, nothing launched: a NULL
// or misaligned pointer with work to do, a level with work and no entries, more than 63 levels.  No work at any level: success, no launch.
hipError_t launch_compress_layers_ragged(void* rows, const uint64_t* tree_tab, const uint64_t* prefix, const uint32_t* tree_of,
                                         const uint64_t* level_off, const uint64_t* level_cnt, const uint64_t* level_work, size_t n_levels,
                                         hipStream_t st);
// n pairs (x, y) of canonical elements -> compress(x, y, key), key in {0,1,2,3}
hipError_t launch_compress_pairs(const void* xy, uint32_t key, void* out, size_t n, hipStream_t st);
hipError_t launch_sponge2_felts(const void* felts, size_t nf, size_t nitems, void* out, hipStream_t st);
// k_hash_cells runs 256-lane workgroups at every batch size.  The 64-lane instantiation was measured against it from 2 MiB to
// 8 GiB (tools/hash_block_sweep.cpp, profiles/r03_hash_block_sweep.txt): identical up to 256 MiB -- a launch lasts at least
// the lifetime of ONE wave, 34 serial permutations = 3.3 ms, whatever the workgroup shape -- and 5...25 % slower above.
hipError_t launch_hash_cells(const void* cells, size_t cell_size, size_t n_cells, void* out, hipStream_t st, bool leave_room = false);   // leave_room: two workgroups per CU instead of three (kernels.hip)
// Can k_hash_cells be launched with leave_room on the CURRENT device?  Asked once per context (cp2_init): the device's LDS per
// workgroup (never more than lds_cap when that is non-zero: test hook) must hold the kernel's own LDS plus the room, and the kernel's
// dynamic-LDS ceiling is raised to the room.  *why says what was found either way.  A launch itself is never retried.
bool hash_cells_can_leave_room(size_t lds_cap, std::string* why);
// the same with the workgroup size given (64 or 256): measurement tooling only
hipError_t launch_hash_cells_block(int block, const void* cells, size_t cell_size, size_t n_cells, void* out, hipStream_t st, bool leave_room = false);
// cells_per_slot == 0: one slot with seed `seed0`; otherwise global cell g belongs to slot g / cells_per_slot
// whose seed is seed0 + 1001 * slot.  list (device, may be NULL) selects explicit global cells.
// units_per_slot > 1: slots cut into units of `cells_per_slot` cells each (batch-local unit g / cells_per_slot is unit
// first_unit + that of the dataset, unit u lies in slot u / units_per_slot; seed0 = the seed of slot 0 of the dataset).
hipError_t launch_gen_fake_cells(uint64_t seed0, uint64_t cells_per_slot, uint64_t first, const uint64_t* list,
                                 size_t n_cells, size_t cell_size, void* out, hipStream_t st, uint64_t units_per_slot = 1,
                                 uint64_t first_unit = 0);
// Sampling + path lookup for proof inputs, all on the device (sample/bn254.nim:16-27, merkle.nim:21-42,86-100,
// types.nim:27-37): for item i < n_items (slot = slots ? slots[i] : slot0 + i, an index INSIDE the batch) and
// counter c = 1..ns:  cell = low bits of sponge2[entropy, slotRoot, c];  indices[i*ns+c-1] = cell;
// gcell[...] = slot * n_cells + cell;  rows[(i*ns+c-1)*md ..] = node-row index of each sibling on the merged path,
// ~0 where the reference pads with zero.  entropy: 32 bytes in device memory.
hipError_t launch_sample_paths(const TreeGeom& g, const void* nodes, const void* d_entropy, const uint64_t* slots, uint64_t slot0,
                               size_t n_items, uint32_t ns, uint32_t md, uint64_t* indices, uint64_t* gcell, uint64_t* rows,
                               hipStream_t st);
// out[r] = row index[r] of src (row_bytes bytes each), zeros where index[r] is ~0.  Whole 32-bit words: hipErrorInvalidValue, and
// nothing launched, when row_bytes is no multiple of 4 or src / out are not 4-byte aligned.
hipError_t launch_gather_rows(const void* src, const uint64_t* index, size_t nrows, size_t row_bytes, void* out,
                              hipStream_t st);

// Scrub (scrub.cpp): row g < n_items * rows (item g / rows, row g % rows) of the fresh layer (fresh + (item * fstride + row) * 32) against
// the kept one (kept + (item * kstride + row) * 32), 32-byte rows.  Workgroup w covers rows [w * SCRUB_TILE, + SCRUB_TILE): bits[g / 64]
// bit g % 64 is set where the rows differ (every word of the tile is written, zeros past the end) and counts[w] holds the tile's number
// of set bits.  bits: scrub_groups(n) * SCRUB_TILE / 64 words, counts: scrub_groups(n) words.
constexpr size_t SCRUB_TILE = 4096;
inline size_t scrub_groups(size_t n_rows) { return (n_rows + SCRUB_TILE - 1) / SCRUB_TILE; }
hipError_t launch_scrub_compare(const void* fresh, size_t fstride, const void* kept, size_t kstride, size_t rows, size_t n_items,
                                uint64_t* bits, uint32_t* counts, hipStream_t st);
// The same with the kept layer of item i anywhere: kept_addr (device, n_items entries) holds the device address of row 0 of item i's
// kept layer, so the kept row of global row g is at kept_addr[g / rows] + (g % rows) * 32.  Same bits, same counts, same zero words.
hipError_t launch_scrub_compare_many(const void* fresh, size_t fstride, const uint64_t* kept_addr, size_t rows, size_t n_items, uint64_t* bits,
                                     uint32_t* counts, hipStream_t st);

// Building many datasets in one pass (build_many.cpp): the write through an address table.  Row g < rows * n_items is row g % rows of item
// g / rows and is copied from src + (item * sstride + row) * 32 to dst_addr[item] + row * 32; dst_addr (device, n_items entries) holds
// absolute device addresses, 16-byte aligned; 0 = the item keeps nothing here (its rows are neither read nor written).  Nothing outside
// the rows is written.  Launched in slices of at most `slice` rows (0: what one grid holds; the tests pass small ones).
// hipErrorInvalidValue, nothing launched: src or dst_addr NULL with work to do, sstride < rows.  rows == 0 or n_items == 0: no work.
hipError_t launch_scatter_rows_addr(const void* src, size_t sstride, const uint64_t* dst_addr, size_t rows, size_t n_items, hipStream_t st,
                                    size_t slice = 0);

// Block repair (repair.cpp): verdict[i] = 0 when the 32-byte row i of `fresh` equals row rows[i] of `kept` (kept_rows rows), else 1.
hipError_t launch_repair_compare(const void* fresh, const void* kept, size_t kept_rows, const uint64_t* rows, size_t n, uint32_t* verdict,
                                 hipStream_t st);
// The same with the kept row of request i at the absolute device address kept_addr[i] (device table, n entries; 16-byte aligned; 0 is
// none: a mismatch, not read), so that one launch serves the requests of many datasets (read_blocks.cpp).  Launched in slices of at
// most `slice` requests (0: what one grid holds; the tests pass small ones).
hipError_t launch_repair_compare_addr(const void* fresh, const uint64_t* kept_addr, size_t n, uint32_t* verdict, hipStream_t st, size_t slice = 0);

// Block proofs (block_proofs.cpp, k_block_path_roots): request i < n = the 32-byte row i of `fresh` (a candidate's block root), the pair
// root_block[2 i], root_block[2 i + 1] (index into slot_roots, block of the slot; validated by the host) and `depth` canonical siblings
// at paths + i * depth * 32.  reconstructRoot (merkle.nim:51-74) over n_blocks leaves; verdict[i] = 0 when the result equals
// slot_roots[root] as a field element, else 1; roots_out (may be NULL) receives n x 32 bytes, the rows of `fresh`.
hipError_t launch_block_path_roots(const void* fresh, const void* paths, const uint64_t* root_block, const void* slot_roots, uint64_t n_blocks,
                                   uint32_t depth, size_t n, uint32_t* verdict, void* roots_out, hipStream_t st);

// Repair across many datasets (repair_many.cpp, k_repair_judge_many): launch_block_path_roots' walk and launch_repair_compare_addr's
// absolute addresses with everything per request.  One descriptor per request, a device table uploaded once per call.
struct RepairManyReq {
  uint64_t want;         // device address of the 32-byte row to compare with, 16-byte aligned; 0 is none: a mismatch, not read
  uint64_t blk;          // block of the slot: the walk's first index
  uint64_t n_blocks;     // the walk's first layer size
  uint64_t path_at;      // first row of the request's siblings in `paths` (canonical or not, bottom first)
  uint32_t len;          // levels walked: 0 compares the row of `fresh` itself
  uint32_t reserved;     // 0
};
// verdict[i] = 0 when the 32-byte row i of `fresh`, walked up len levels of reconstructRoot over rows path_at ... of `paths`, equals the row
// at `want` as a field element, else 1.  `paths` may be NULL when every len is 0.  Nothing but verdict[0, n) is written.  Launched in
// slices of at most `slice` requests (0: what one grid holds; the tests pass small ones): a chunk of a call is a slice of one table.
hipError_t launch_repair_judge_many(const void* fresh, const void* paths, const RepairManyReq* reqs, size_t n, uint32_t* verdict, hipStream_t st,
                                    size_t slice = 0);

// Slot filling (fill.cpp, k_block_path_commit): launch_block_path_roots' walk over (local slot, block) pairs, slot_roots indexed by the
// local slot.  Where request i is a match (verdict[i] = 0) the 32-byte row i of `fresh` is also stored to row dest[i] of `layer0` (n_rows
// rows; the host computed dest[i] inside layer 0 of the compact layout); a mismatch stores nothing.
hipError_t launch_block_path_commit(const void* fresh, const void* paths, const uint64_t* slot_block, const void* slot_roots, const uint64_t* dest,
                                    uint64_t n_blocks, uint32_t depth, size_t n, uint32_t* verdict, void* layer0, uint64_t n_rows, hipStream_t st);

// Slot filling with the nodes kept (fill.cpp, k_block_path_commit_nodes): launch_block_path_commit's walk and verdicts.  Where request i is
// a match, the block root goes to row dest[i] as there, and every node its path proves goes where the compact layout has it: sibling l to
// row layer_off[l] + local_slot * layer_size[l] + ((block >> l) ^ 1) unless that index is at or past layer_size[l], ancestor l to row
// layer_off[l + 1] + local_slot * layer_size[l + 1] + (block >> (l + 1)); layer_off / layer_size are device tables of depth + 1 entries,
// `tree` has n_rows rows.  `scratch` (device, n x depth x 64 bytes, 16-byte aligned) receives every request's canonical siblings and
// ancestors during the walk; a mismatch writes nothing else.
hipError_t launch_block_path_commit_nodes(const void* fresh, const void* paths, const uint64_t* slot_block, const void* slot_roots,
                                          const uint64_t* dest, const uint64_t* layer_off, const uint64_t* layer_size, uint64_t n_blocks,
                                          uint32_t depth, size_t n, uint32_t* verdict, void* tree, uint64_t n_rows, void* scratch, hipStream_t st);

// Slot filling with paths that stop at a kept node (fill.cpp, k_block_path_commit_anchored): launch_block_path_commit_nodes' walk, request i
// over its lowest levels[i] <= depth levels only.  `paths` is PACKED: request i's levels[i] canonical siblings, bottom first, start at row
// path_off[i] - path_base (path_off: the prefix sum of levels, one entry per request; path_base: the entry of the first request whose
// siblings `paths` holds, 0 for a whole call).  verdict[i] = 0 when the node reached equals row anchor_row[i] of `tree` as a field element
// (anchor_row[i] == UINT64_MAX: slot_roots[local slot]; any other row >= n_rows: a mismatch).  A match stores the block root to row dest[i],
// the in-range siblings of levels 0 ... levels[i] - 1 and the ancestors of levels 1 ... levels[i] - 1 where the compact layout has them;
// the anchor row and every row above it are never written, levels[i] == 0 stores nothing.  `scratch` (device, sum(levels) x 64 bytes,
// 16-byte aligned) receives request i's siblings and ancestors at row 2 (path_off[i] - path_base); a mismatch writes nothing else.
hipError_t launch_block_path_commit_anchored(const void* fresh, const void* paths, const uint32_t* levels, const uint64_t* path_off,
                                             uint64_t path_base, const uint64_t* slot_block, const void* slot_roots, const uint64_t* dest,
                                             const uint64_t* anchor_row, const uint64_t* layer_off, const uint64_t* layer_size,
                                             uint64_t n_blocks, uint32_t depth, size_t n, uint32_t* verdict, void* tree, uint64_t n_rows,
                                             void* scratch, hipStream_t st);

// Slot filling across many sessions (fill_many.cpp, k_block_path_commit_many): launch_block_path_commit_anchored with the session per
// request.  One descriptor per session, a device table of n_sessions entries uploaded once per call: what the launchers above take as
// launch arguments.
struct FillManySession {
  uint64_t tree;         // device address of the session's compact buffer ...
  uint64_t n_rows;       // ... and its rows
  uint64_t slot_roots;   // device address of the stated roots, canonical, n_local x 32 bytes ...
  uint64_t n_local;      // ... and how many
  uint64_t layer_tab;    // device address of layer_off, depth + 1 entries, layer_size behind it; 0: the session keeps no nodes
  uint64_t n_blocks;
  uint32_t depth;
  uint32_t reserved;     // 0
};
// Request i belongs to session session_of[i]; levels, path_off / path_base, slot_block (local slot, block), dest and anchor_row as for
// launch_block_path_commit_anchored, the rows being rows of that session's buffer, and `paths` / `scratch` packed over the whole launch.
// verdict[i] = 0 and the stores of a match as there, into the session's buffer; a session that keeps no nodes receives the block root
// alone.  keep_top: a path of its session's full depth also leaves its last ancestor (the slot root's row) in a session that keeps nodes,
// as launch_block_path_commit_nodes does.  A session index >= n_sessions, a level above the session's depth, a level below it in a
// session that keeps no nodes, a slot >= n_local and a dest or anchor row >= n_rows are mismatches that store nothing.
hipError_t launch_block_path_commit_many(const void* fresh, const void* paths, const FillManySession* sessions, uint64_t n_sessions,
                                         const uint64_t* session_of, const uint32_t* levels, const uint64_t* path_off, uint64_t path_base,
                                         const uint64_t* slot_block, const uint64_t* dest, const uint64_t* anchor_row, bool keep_top, size_t n,
                                         uint32_t* verdict, void* scratch, hipStream_t st);

// Finishing many fill sessions (fill_finish_many.cpp, k_finish_layer_many): every layer above layer 0 of every local slot tree of
// n_sessions sessions, each in its own compact (layer-major) buffer, one launch per level in order on st, and on each session's last level
// the comparison of the computed slot roots with its stated ones.  Device: `sessions` (of a descriptor tree, n_rows, slot_roots, n_local,
// n_blocks and depth are read, layer_tab is not), voff (verdict offset of session k: the prefix sum of n_local, n_sessions entries),
// prefix and sess_of (per level l the entries [level_off[l], + level_cnt[l]): the sessions with depth > l in order and the running sum of
// their n_local * csizes[l + 1]), verdict (sum of n_local words; entry voff[k] + s = 0 when local slot s of session k ends in its stated
// root, else 1; every entry is written exactly once, nothing needs clearing).  Host: level_off, level_cnt, level_work (the lanes of level
// l: its last prefix), n_levels entries each.  Layer 0 is read, every other row of every session is written, nothing else; the computed
// root is stored whatever the verdict.  A destination row >= n_rows is not stored and ends in verdict 1.  hipErrorInvalidValue, nothing
// launched: a NULL or misaligned table with work to do, a level with work and no entries or more than 2^32, work that does not fit one
// grid, more than 63 levels.  No work at any level: success, no launch.
hipError_t launch_finish_layers_many(const FillManySession* sessions, uint64_t n_sessions, const uint64_t* voff, const uint64_t* prefix,
                                     const uint32_t* sess_of, const uint64_t* level_off, const uint64_t* level_cnt, const uint64_t* level_work,
                                     size_t n_levels, uint32_t* verdict, hipStream_t st);

// Block multiproofs (multiproofs.cpp, k_multiproof_layer): the induced subtrees of many groups of blocks, level by level, over one work
// table of 32-byte rows (`work`, n_work rows, 16-byte aligned): leaf rows, sent rows, then the computed rows (multiproof_plan.hpp).  One
// job per computed row, 16 bytes, the layout of cp2i::MultiproofJob.
struct MultiproofJob {
  uint32_t left;       // a row of the work table
  uint32_t right;      // a row of the work table, or MULTIPROOF_ZERO: the zero beside an odd layer's last node
  uint32_t key_last;   // the compression's key 0..3 | last << 8
  uint32_t group;
};
constexpr uint32_t MULTIPROOF_ZERO = 0xFFFFFFFFu;
// One launch per level in order on st, no host wait between them.  Device: jobs (16-byte aligned; level k's are [level_off[k],
// level_off[k + 1])), want_addr (per group the absolute device address of its stated root, 32 bytes, 16-byte aligned; 0 or misaligned: a
// mismatch, not read), verdict (one word per group).  Host: level_off (n_levels + 1 entries), level_base (n_levels).  Job t of level k
// stores compress(left, right, key) at row level_base[k] + t; a job with `last` set also writes verdict[group] = 0 when its row equals the
// stated root as a field element, else 1, the row stored as computed either way.  Every group has one such job, so each verdict word
// has one writer and nothing is cleared beforehand.  A job that names a row at or past its level's base reads and stores nothing (with
// `last`: verdict 1).  Nothing but the computed rows and the verdicts is written.  hipErrorInvalidValue, nothing launched: a NULL or
// misaligned table with work to do, a level whose output starts below the end of an earlier level's or ends past n_work or reaches row 2^32 - 1,
// level_off that descends, more than 63 levels.  No jobs at any level: success, no launch.
hipError_t launch_multiproof_layers(void* work, uint64_t n_work, const MultiproofJob* jobs, const uint64_t* level_off, const uint64_t* level_base,
                                    size_t n_levels, const uint64_t* want_addr, uint32_t* verdict, hipStream_t st);

// What a fill session keeps of them (fill.cpp, k_multiproof_commit): lane i < n copies the 32-byte row src_row[i] of `work` to the absolute
// device address dst_addr[i] (16-byte aligned) when verdict[group_of[i]] == 0, and does nothing otherwise.  Two lanes may name one
// destination: they carry identical bytes (every row of a proved group is the authentic node of its place).  A source row at or past
// n_work, a group at or past n_groups and a destination that is 0 or misaligned copy nothing.  hipErrorInvalidValue, nothing launched: a
// NULL or misaligned table with n > 0.  n == 0: success, no launch.
hipError_t launch_multiproof_commit(const void* work, uint64_t n_work, const uint32_t* src_row, const uint64_t* dst_addr, const uint32_t* group_of,
                                    const uint32_t* verdict, uint32_t n_groups, size_t n, hipStream_t st);

// Multiproofs that stop at nodes a fill session holds (fill.cpp, cp2_fill_add_multi_anchored; k_multiproof_tops, k_multiproof_fold): a
// group has one or more tops, rows of the work table that must each equal an authentic kept row.  Device: tops (n_tops, group-major),
// want_addr (per top the absolute address of the kept row, 32 bytes, 16-byte aligned), d_top_off (n_groups + 1: group g's tops are
// [d_top_off[g], d_top_off[g + 1])), top_verdict (n_tops words), verdict (n_groups words).  Host: top_off, the same n_groups + 1 values.
// Two launches in order on st: lane t writes top_verdict[t] = 0 when row tops[t].row equals the row at want_addr[t] as a field element,
// else 1 (a row at or past n_work, an address that is 0 or misaligned: 1, nothing read); then lane g writes verdict[g] = the OR of its
// range, 1 for an empty range.  Every word has one writer, nothing is cleared beforehand, nothing else is written.
// hipErrorInvalidValue, nothing launched: a NULL or misaligned table with work to do, a top_off that descends or ends past n_tops, work
// that does not fit one grid.  n_groups == 0: success, no launch.
struct MultiproofTop {
  uint32_t row;        // a row of the work table
  uint32_t group;
};
hipError_t launch_multiproof_tops(const void* work, uint64_t n_work, const MultiproofTop* tops, const uint64_t* want_addr, size_t n_tops,
                                  const uint64_t* top_off, const uint64_t* d_top_off, size_t n_groups, uint32_t* top_verdict, uint32_t* verdict,
                                  hipStream_t st);

// Resuming a fill session (fill.cpp, k_block_root_recheck): verdict[i] = 0 when the 32-byte row i of `fresh` (the root a re-read block
// hashed to) equals row dest[i] of `layer0` (n_rows rows), else 1 -- and then that row of layer0 is overwritten with zeros.  dest[i] >=
// n_rows: verdict 1, nothing read or written.  The rows of one call are distinct.
hipError_t launch_block_root_recheck(const void* fresh, const uint64_t* dest, size_t n, uint32_t* verdict, void* layer0, uint64_t n_rows,
                                     hipStream_t st);
// Resuming many fill sessions (fills_resume_many.cpp, k_block_root_recheck_addr): the same with the kept row of block i at the absolute
// device address addr[i] (layer 0 of its own session), so that one call judges blocks of many sessions.  addr[i] == 0 or not 16-byte
// aligned: verdict 1, nothing read or written.  The addresses of one call are distinct.  n == 0: success, no launch.
hipError_t launch_block_root_recheck_addr(const void* fresh, const uint64_t* addr, size_t n, uint32_t* verdict, hipStream_t st);

// Adopting blocks from disk (fill.cpp, cp2_fill_adopt).  `tree` is the session's compact buffer (n_rows rows of 32 bytes), `cand` a buffer of
// the same shape whose layer 0 holds the block roots of the candidates, `flags` one byte per row: bit 0 (ADOPT_KNOWN) the session knows
// the row -- set by the host, and for every top row -- bit 1 (ADOPT_CAND) the row of `cand` holds a computed value, bit 2 (ADOPT_MATCH)
// that value equals the kept one.  Both calls work on local slots [first_sel, first_sel + n_sel) of n_local and leave the rows, bytes and
// flags of every other slot alone; rows at or past n_rows are neither read nor written.
constexpr uint8_t ADOPT_KNOWN = 1, ADOPT_CAND = 2, ADOPT_MATCH = 4, ADOPT_PROVED = 8, ADOPT_ADOPTED = 16;
// k_adopt_layer once per layer, bottom first: layer l + 1 of `cand` and `flags` from layer l, a node's value taken from `tree` where it is
// known and from `cand` otherwise, bit 2 against the kept row or, in the top layer, against slot_roots[local slot].  The layer tables are
// HOST arrays of depth + 1 entries (FillPlan::coff / csizes); tables that are not a compact layout of n_local slots are refused.
hipError_t launch_adopt_layers(const void* tree, void* cand, uint8_t* flags, const void* slot_roots, const uint64_t* layer_off_host,
                               const uint64_t* layer_size_host, uint32_t depth, uint64_t n_local, uint64_t first_sel, uint64_t n_sel, uint64_t n_rows,
                               hipStream_t st);
// k_adopt_resolve over the n_below rows under the top layer (n_below = layer_off[depth]); layer_off / layer_size are DEVICE tables of
// depth + 1 entries.  out[r] (one byte per row, written for the selected slots only) = bits 0-2 of flags[r], bit 2 of a known layer-0 row
// set here from a bytewise comparison, bit 3 (ADOPT_PROVED) where an unknown row with a computed value reaches a matching known ancestor
// through computed rows only -- that row of `cand` is then copied into `tree` -- and bit 4 (ADOPT_ADOPTED) on a layer-0 row that is
// proved, or known and equal.  No known row of `tree` is written.
hipError_t launch_adopt_resolve(void* tree, const void* cand, const uint8_t* flags, uint8_t* out, const uint64_t* layer_off,
                                const uint64_t* layer_size, uint32_t depth, uint64_t n_local, uint64_t first_sel, uint64_t n_sel, uint64_t n_below,
                                uint64_t n_rows, hipStream_t st);

// Restoring kept nodes from a checkpoint (fill.cpp, cp2_fill_resume_nodes).  `tree` is the session's compact buffer (n_rows rows of 32
// bytes), `cand` a buffer of the same shape that holds what the checkpoint states in its candidate rows, `flags` one byte per row, a row
// being in one state: NODE_KNOWN the session knows the row -- set by the host, and for every top row -- NODE_CAND the row of `cand` is a
// candidate, NODE_RESTORED / NODE_REJECTED what the kernel made of a candidate, 0 undefined.
constexpr uint8_t NODE_KNOWN = 1, NODE_CAND = 2, NODE_RESTORED = 4, NODE_REJECTED = 8;
// k_nodes_restore_layer once per layer, TOP FIRST, over every local slot: a parent that is known or restored, with every child known or a
// candidate and at least one a candidate, is recomputed from its children (a known child from `tree`, a candidate from `cand`) and compared
// with its row of `tree` or, in the top layer, with slot_roots[local slot].  Equal: the candidate children are stored into `tree` and
// flagged NODE_RESTORED; unequal: flagged NODE_REJECTED.  Nothing else is written; rows at or past n_rows are neither read nor written.
// One layer: the children are rows off_in + slot x m_in + k (k < m_in) of the n_local slots, the parents rows off_out + slot x ceil(m_in / 2)
// + j; bottom: the children are layer 0 (key 1); top: a parent's value is slot_roots[slot] and its row of `tree` is not read.
hipError_t launch_nodes_restore_layer(void* tree, const void* cand, uint8_t* flags, const void* slot_roots, uint64_t off_in, uint64_t m_in,
                                      uint64_t off_out, uint64_t n_local, bool bottom, bool top, uint64_t n_rows, hipStream_t st);
// Every layer of a compact layout, top first.  The layer tables are HOST arrays of depth + 1 entries (FillPlan::coff / csizes); tables
// that are not a compact layout of n_local slots are refused.
hipError_t launch_nodes_restore_layers(void* tree, const void* cand, uint8_t* flags, const void* slot_roots, const uint64_t* layer_off_host,
                                       const uint64_t* layer_size_host, uint32_t depth, uint64_t n_local, uint64_t n_rows, hipStream_t st);

// Proof-input verification (k_verify_samples, circuit/codex/sample_cells.circom:58-148) over n inputs that share the circuit
// parameters.  Device arrays: prm n x 4 (nCellsPerSlot, nSlotsPerDataSet, slotIndex, shape ok), heads n x (3 + m) felts
// (dataSetRoot, entropy, slotRoot, slotProof), cells n x ns x nf felts, paths n x ns x md felts; ok receives n x ns sample
// bytes, then n dataset-root bytes.
struct VerifyGeom {
  size_t n;
  uint32_t ns, nf, md, m, bd;   // nSamples, felts per cell, maxDepth, maxLog2NSlots, blockTreeDepth
};
hipError_t launch_verify_samples(const VerifyGeom& g, const uint64_t* prm, const void* heads, const void* cells, const void* paths,
                                 uint8_t* ok, hipStream_t st);

// Proof inputs across datasets (proof_many.cpp).  One request = (dataset, slot, entropy); all requests share nSamples and maxDepth.
struct alignas(16) ManyReq {
  uint8_t entropy[32];     // canonical
  uint8_t slot_root[32];   // the slot's root (layer 0 of its dataset tree)
  uint64_t n_cells;        // cells of the slot (a power of two)
  uint64_t cpb;            // cells per network block
  uint64_t nodes;          // every node resident: device address of the node buffer of the dataset's trees; 0: compact
  uint64_t slot;           // index of the slot inside that node buffer (resident only)
  uint32_t geom, pad;      // resident only: index into the TreeGeom table
};
// k_sample_many: lane t = (request t / ns, counter t % ns + 1) of n_req * ns lanes.  indices[t] = cellIndex (sample/bn254.nim:16-27).
// Resident requests: addr[t * md + d] = device address of path sibling d (merkle.nim:21-42,86-100), 0 where padMerkleProof pads with
// zero (types.nim:27-37), and addr[n_req * ns * md + t] = the address of the sampled cell's own hash.  Compact requests: blocks[t] = the
// touched network block; their addresses are left as they are.
hipError_t launch_sample_many(const ManyReq* reqs, const TreeGeom* geoms, size_t n_req, uint32_t ns, uint32_t md, uint64_t* indices,
                              uint64_t* blocks, uint64_t* addr, hipStream_t st);
// out[r] = the row_bytes bytes at device address addr[r]; address 0 gives a row of zeros
hipError_t launch_gather_addr(const uint64_t* addr, size_t nrows, size_t row_bytes, void* out, hipStream_t st);
// genFakeCell (slot.nim:22-32), list form with a seed per group of `per` rows: row i is cell firsts[i / per] + i % per of the slot whose
// seed (cp2_slot_seed) is seeds[i / per]
hipError_t launch_gen_fake_cells_many(const uint64_t* seeds, const uint64_t* firsts, uint64_t per, size_t n_rows, size_t cell_size,
                                      void* out, hipStream_t st);

}  // namespace cp2k
