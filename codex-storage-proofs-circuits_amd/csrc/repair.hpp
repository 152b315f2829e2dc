// Block repair shared by repair.cpp (cp2_dataset_repair_blocks) and multi_gpu.cpp (cp2_multi_dataset_repair_blocks).  Not installed.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "repair_plan.hpp"
#include "trees.hpp"

namespace cp2i {

// the device node buffer that holds the kept block roots (32-byte rows)
struct RepairKept {
  const uint8_t* nodes = nullptr;
  size_t rows = 0;
};
// what a dataset keeps of its block roots: every node (its trees) or the compact layers; tree mode 1, 2, or 0 (roots only: none)
int repair_dataset_mode(const cp2_dataset* ds);
RepairKept repair_dataset_kept(const cp2_dataset* ds);
// the kept row of block `block` of dataset slot `slot` (inside the local range) of a dataset of mode 1 or 2
uint64_t repair_dataset_row(const cp2_dataset* ds, uint64_t slot, uint64_t block);
// the checks of cp2_dataset_repair_blocks before any device or file work (validation, roots-only, fake source without CHECK_ONLY):
// CP2_OK, or CP2_ERR_INVALID with *err naming the rule and, for a request, its index.  tree_mode 0: roots only.
int repair_refuse(const cp2_config& cfg, bool from_file, int tree_mode, const uint64_t* slot_block, const uint8_t* data, size_t n, int flags,
                  const uint32_t* status, uint64_t first_slot, uint64_t n_local, std::string* err);
// n candidate blocks (host, n x block_size) hashed and reduced to their block roots on the context's device, chunk by chunk (half the
// context's staging each), and compared with row rows[i] of `k` by k_repair_compare: status[i] = CP2_REPAIR_MATCH or _MISMATCH
int repair_check(cp2_ctx* ctx, const RepairKept& k, size_t cell_size, size_t block_size, const uint8_t* data, const uint64_t* rows, size_t n,
                 uint32_t* status);
// The same data path with the last step given by the caller (block_proofs.cpp walks each root up its Merkle path instead of comparing
// it with a kept row).  begin (may be empty): once, before any chunk, with the number of requests a chunk holds at most, for what the call needs on the
// device (queued on the context's stream).  stage (may be empty): per chunk of requests [c0, c0 + m), queued on `st` behind the chunk's hashing and before its
// block trees: what the verdicts of that chunk read beside the roots.  verdicts: queued on `st` behind the chunk's block trees; `fresh`
// holds the chunk's m block roots (32-byte rows, request c0 + i at row i), verdict[i] receives 0 for a match, anything else for a
// mismatch.  cells (may be empty): a device-side source of the candidates, in place of `data`, which may then be NULL: per chunk it queues
// on `st` whatever fills d_cells with the m x block_size bytes of requests [c0, c0 + m); the chunk is hashed behind it on the context's
// stream, as a small pageable chunk is behind its upload.  host (may be empty): a host-side source that produces the candidates chunk by
// chunk, in place of `data`, which is then not looked at: called once per chunk, in order, before anything of the chunk is queued, it
// sets *src to the m x block_size bytes of requests [c0, c0 + m), which stay valid and unchanged until the chunk after the next is asked
// for; host_pinned says whether the copy engines read every such *src in place (read_blocks.cpp reads slot files one chunk ahead).
// Everything the callbacks allocate must outlive the call (it ends with the stream drained).
struct RepairJudge {
  std::function<int(size_t chunk)> begin;
  std::function<int(size_t c0, size_t m, const uint8_t** src)> host;
  bool host_pinned = false;
  std::function<int(size_t c0, size_t m, uint8_t* d_cells, hipStream_t st)> cells;
  std::function<int(size_t c0, size_t m, hipStream_t st)> stage;
  std::function<int(const uint8_t* fresh, size_t c0, size_t m, uint32_t* verdict, hipStream_t st)> verdicts;
};
int repair_check_with(cp2_ctx* ctx, size_t cell_size, size_t block_size, const uint8_t* data, size_t n, uint32_t* status, const RepairJudge& judge);
// Block proofs out of a device node buffer (block_proofs.cpp; cp2_dataset_block_proofs and cp2_fill_block_proofs): `rows` (host) names
// depth + 1 rows of `nodes` per request, its block root and then its siblings bottom first, BLOCK_PROOF_NO_ROW for zeros.  A row at or past
// n_rows: CP2_ERR_INVALID with the error text `outside`, before any device work.  Otherwise one gather and one download, split into
// block_roots (n x 32 bytes, may be NULL) and paths (n x depth x 32 bytes, may be NULL).
int gather_block_proofs(cp2_ctx* ctx, const void* nodes, size_t n_rows, const std::vector<uint64_t>& rows, size_t depth, const char* outside,
                        uint8_t* block_roots, uint8_t* paths);
// The gather under it, by absolute device address (read_blocks.cpp: the rows of many datasets in one launch): out (host, addr.size() x 32
// bytes) row r = the 32 bytes at addr[r], zeros for 0.  One upload of the table, one k_gather_addr, one download; the stream is drained.
int gather_rows_by_addr(cp2_ctx* ctx, const std::vector<uint64_t>& addr, uint8_t* out);
// Groups of candidates with their multiproofs judged against stated roots (multiproofs.cpp; cp2_blocks_verify_multi and
// cp2_fill_add_multi): `plan` is the work table and job tables of the call's validated groups (multiproof_plan.hpp), want[g] the absolute
// device address of group g's stated root (32 bytes, 16-byte aligned), data the plan.n candidates in request order, nodes the plan.n_rows
// sent rows.  repair_check_with's data path, then k_multiproof_layer level by level, then `commit` (may be empty) with the work table and
// the group verdicts in device memory, queued on the same stream; then group_verdict (host, n_groups: 0 proved, anything else not) and
// block_roots (host, plan.n x 32 bytes, may be NULL: what each candidate hashed to) are downloaded and the stream is drained.
//   With `anchors` (cp2_fill_add_multi_anchored; multiproof_anchor_plan.hpp) the groups stop at nodes a fill session holds: the work
// table has n_kept rows between the sent rows and the computed ones, gathered once, before the layers, from the absolute device
// addresses kept_addr (k_gather_addr); no job of the plan compares, `want` is not looked at, and the group verdicts come from the
// n_tops tops ((work row, group), group-major; top_off: n_groups + 1) compared with the kept rows at top_want (k_multiproof_tops,
// k_multiproof_fold) before `commit` runs.
struct MultiproofPlan;
struct MultiproofAnchors {
  size_t n_kept = 0, n_tops = 0;
  const uint64_t* kept_addr = nullptr;   // n_kept
  const uint32_t* top_row_group = nullptr;   // n_tops x 2: the layout of cp2k::MultiproofTop
  const uint64_t* top_want = nullptr;    // n_tops
  const uint64_t* top_off = nullptr;     // n_groups + 1
};
using MultiproofCommit = std::function<int(const void* d_work, const uint32_t* d_verdict, hipStream_t st)>;
int multiproof_check(cp2_ctx* ctx, size_t cell_size, size_t block_size, const MultiproofPlan& plan, const uint64_t* want, size_t n_groups,
                     const uint8_t* data, const uint8_t* nodes, const MultiproofCommit& commit, uint32_t* group_verdict, uint8_t* block_roots,
                     const MultiproofAnchors* anchors = nullptr);
// the requests whose status is CP2_REPAIR_MATCH written into "<base><slot>.dat", grouped by file in ascending offset order, each file synced
// once.  The first file that cannot be opened, written or synced: CP2_ERR_IO, *err "cannot write <file>: <reason>", its matched requests and
// those of every later file CP2_REPAIR_UNWRITTEN.  *n_written counts the blocks of the files written and synced, `written` their stamps.
int repair_write(const std::string& base, size_t block_size, const uint64_t* slot_block, const uint8_t* data, size_t n, uint32_t* status,
                 size_t* n_written, std::vector<FileStamp>* written, std::string* err);
// the same writer with request i's bytes at row row[i] of `data` (cp2_fills_add_many: one session's requests out of the call's blocks, with
// no copy of them); row == NULL: row i
int repair_write_rows(const std::string& base, size_t block_size, const uint64_t* slot_block, const uint8_t* data, const size_t* row, size_t n,
                      uint32_t* status, size_t* n_written, std::vector<FileStamp>* written, std::string* err);
// cache_restamp (cache_file.hpp) over each of `paths`; *restamped accumulates
int repair_restamp_caches(const std::vector<std::string>& paths, const cp2_config& cfg, uint64_t n_items, size_t n_cells, uint64_t first_item,
                          uint64_t units_per_slot, const std::string& base, const std::vector<FileStamp>& written, size_t* restamped,
                          std::string* err);
// the CP2_TRACE line of one call
void repair_trace(const char* what, size_t n, const uint32_t* status, size_t n_written, size_t block_size, double seconds, size_t restamped,
                  bool cache);

}  // namespace cp2i
