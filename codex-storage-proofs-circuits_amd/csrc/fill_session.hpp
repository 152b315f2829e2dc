// The session behind the header's opaque cp2_fill, shared by fill.cpp (one session's calls) and fill_many.cpp (cp2_fills_add_many, many
// sessions in one pass).  Not installed.
#pragma once
#include <cstdint>
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
