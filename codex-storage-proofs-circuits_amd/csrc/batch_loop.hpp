// THE loop of the builds that rebuild slot trees batch by batch in two node buffers used alternately, nothing synchronised per batch:
// the compact / roots-only build and the batched streamed build (proof_input.cpp), the scrub (scrub.cpp), build many (build_many.cpp).
// Plain logic, no HIP: the product's device is BatchDevice (trees.hpp); the CPU suite drives this header with a stand-in device that
// models the two buffers, over every shape and every failing step (tests/host_check/batch_loop_check.cpp).  The ordering in here is the
// part of the host code where a mistake is a GPU memory fault, not a wrong answer: a buffer handed on one batch early is overwritten
// while a copy-out or a compare still reads it.
//
// n_items are cut into batches of `batch` (the last one shorter); batch k uses buffer b = k & 1.  Per batch, in this order:
//   dev.wait(b)         k >= 2 only: the event recorded after batch k - 2, whatever read buffer b then has completed
//   reuse(step)         the caller's work that needs buffer b (and what it keeps beside it: tables, counts) free
//   build(step, &tail)  one builder call; reports the stream the batch's layer passes ended on.  The batch object stays with the device
//   after(step, tail)   what the caller enqueues behind the batch on that stream (the builds: their copy-out)
//   dev.record(b, tail) then dev.release(): the batch object goes once per build call, whatever the status
//   progress(step)      every 32nd batch and the last
// The first status that is not CP2_OK ends the loop: nothing but that release runs after it.  After the last batch, when every batch went
// well, dev.drain().  A failed wait or drain is CP2_ERR_HIP, "<what>: a batch failed on the device" (a failed launch or copy shows up
// there).  *n_batches (may be null): the batches that ran, the failing one included.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/codex_p2.h"

namespace cp2i {

// Items per batch: half a staging chunk of nodes (1 GiB by default: 4 slots of 8 GiB), at least one item, no more than there are.  The
// pipeline holds two such node buffers, together one staging chunk's worth.  item_bytes: every node of one item (trees_node_bytes).
inline size_t batch_items(size_t stage_bytes, uint64_t item_bytes, uint64_t n_items) {
  return (size_t)std::max<uint64_t>(1, std::min<uint64_t>(n_items, (stage_bytes / 2) / std::max<uint64_t>(1, item_bytes)));
}

struct BatchStep { size_t k, s0, n; int b; bool last; };   // batch k holds items [s0, s0 + n) in buffer b

template <typename Device, typename Reuse, typename Build, typename After, typename Progress>
int batch_loop(Device& dev, const char* what, std::string& err, size_t n_items, size_t batch, Reuse reuse, Build build, After after,
               Progress progress, size_t* n_batches = nullptr) {
  size_t none = 0;
  size_t& k = n_batches ? *n_batches : none;
  k = 0;
  if (batch == 0) return CP2_ERR_INVALID;
  const auto failed = [&] { err = std::string(what) + ": a batch failed on the device"; return CP2_ERR_HIP; };
  for (size_t s0 = 0; s0 < n_items; s0 += batch) {
    const size_t n = std::min(batch, n_items - s0);
    const BatchStep step{k, s0, n, (int)(k & 1), s0 + n == n_items};
    ++k;
    if (step.k >= 2 && dev.wait(step.b) != CP2_OK) return failed();
    if (const int st = reuse(step); st != CP2_OK) return st;
    typename Device::Tail tail{};
    int st = build(step, &tail);
    if (st == CP2_OK) st = after(step, tail);
    if (st == CP2_OK) st = dev.record(step.b, tail);
    dev.release();
    if (st != CP2_OK) return st;
    if ((step.k % 32) == 31 || step.last) progress(step);
  }
  return dev.drain() == CP2_OK ? CP2_OK : failed();
}

}  // namespace cp2i
