// The session behind the header's opaque cp2_fill, shared by fill.cpp (one session's calls), fill_many.cpp (cp2_fills_add_many),
// fill_finish_many.cpp (cp2_fills_finish_many) and fills_resume_many.cpp (cp2_fills_resume_many): many sessions in one pass.  Not installed.
#pragma once
#include <cstdint>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "dataset_obj.hpp"
#include "fill_plan.hpp"

struct cp2_fill_session {
  cp2_ctx* ctx = nullptr;
  cp2_config cfg{};                     // file_base cleared: the name lives in `file_base`
  std::string file_base;
  bool from_file = false;
  cp2i::FillPlan plan;
  cp2i::DevBuf compact;                 // the compact layout of the local slots; becomes the dataset's buffer in finish
  cp2i::DevBuf slot_roots;              // the stated roots, canonical: n_local x 32 bytes
  std::vector<uint8_t> roots;           // ... and on the host, for a checkpoint
  cp2i::DevBuf layer_tab;               // a session that keeps nodes: coff then csizes as uint64, depth + 1 entries each, uploaded once
  cp2i::DevBuf adopt_roots;             // cp2_fill_adopt: the fresh block roots of the candidates, n_local x n_blocks rows, from the first adopt on
  std::vector<uint64_t> adopt_have;     // ... and which of its rows hold one
};

namespace cp2i {

// a buffer handed over without a copy
inline void hand_over(DevBuf& from, DevBuf& to) {
  to.release();
  to.p = from.p; to.bytes = from.bytes; to.owner = from.owner; to.home = from.home; to.borrowed = from.borrowed;
  from.p = nullptr; from.bytes = 0; from.owner = nullptr; from.home = nullptr; from.borrowed = false;
}

// The compact dataset a complete session becomes (dataset_alloc_kept's layout, source as begun), all but its buffer: the finish calls
// hand the session's buffer over into `compact` and mark the session finished.  nullptr: no memory.
inline std::unique_ptr<cp2_dataset> fill_dataset_shell(const cp2_fill_session* f) {
  std::unique_ptr<cp2_dataset> ds(new (std::nothrow) cp2_dataset());
  if (!ds) return ds;
  ds->ctx = f->ctx;
  ds->cfg = f->cfg;
  ds->from_file = f->from_file;
  ds->file_base = f->file_base;
  ds->first_slot = f->plan.first_slot;
  ds->n_local = f->plan.n_local;
  ds->tree_mode = 2;
  ds->csizes = f->plan.csizes;
  ds->coff = f->plan.coff;
  return ds;
}

// What cp2_fill_begin and cp2_fill_resume do before and for a session (fill.cpp), for cp2_fills_resume_many to do per entry:
// the checks of (cfg, first_slot, n_local, slot_roots) before anything is allocated (CP2_ERR_INVALID, the reason in ctx->err) ...
int fill_session_check(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, const uint8_t* slot_roots);
// ... the session of checked arguments, its two buffers as cp2_fill_begin allocates them and nothing uploaded or queued ...
int fill_session_alloc(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, const uint8_t* slot_roots,
                       std::unique_ptr<cp2_fill_session>* out);
// ... and a CP2FILL1 checkpoint file read and parsed: CP2_ERR_IO with cp2_fill_resume's words in *err (any thread may call it)
struct FillCheckpoint;
int fill_read_checkpoint(std::string* err, const char* path, FillCheckpoint* ck);

}  // namespace cp2i
