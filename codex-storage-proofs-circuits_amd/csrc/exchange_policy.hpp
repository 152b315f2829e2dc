// The multi-device exchange of slot (or unit) roots (csrc/multi_gpu.cpp): THE loop around it -- exchange, install, verify, and when it
// may be tried once more through host memory.  Plain logic, no HIP: the CPU suite compiles this header and walks the loop over every
// outcome (tests/host_check/exchange_loop_check.cpp; the predicate alone: tests/test_boundary_version.py).
//
// A retry only in the automatic mode, only once, only with more than one shard -- and NEVER after a time-out.  A launch error or a failed
// verification leaves the participating streams drained: host memory then carries the same 1 MiB just as well.  A time-out leaves a
// collective (or a peer copy) queued on those very streams; the host path enqueues its downloads behind it and then waits without a
// bound, so the "bounded" exchange would never return after all.  A time-out is final: the error goes to the caller, the
// contexts are marked as taking no further work, their pooled buffers are dropped from the books rather than waited for.
#pragma once
#include <cstddef>
#include <string>

#include "../../include/codex_p2.h"

namespace cp2i {

inline bool exchange_may_retry_on_host(int status, bool timed_out, int gather_mode, size_t world, int attempt) {
  if (status == CP2_OK || timed_out) return false;
  return attempt == 0 && gather_mode == CP2_GATHER_AUTO && world > 1 && status == CP2_ERR_HIP;
}

// one exchange: its status; given up with work still queued?  the roots in device memory (else host memory)?  did anything move at all?
struct ExchangeOutcome { int status = CP2_OK; bool timed_out = false, on_device = false, moved = true; };

// At most two exchanges.  exchange(force_host) -> ExchangeOutcome, its error text in `err` and what carried the roots in `note`;
// install(outcome) -> status puts the gathered roots to use; verify(outcome, bad) -> status, `bad` left empty when all is where it belongs.
//   a failed exchange   retried at once through host memory where the rule above allows it, `note` then gains " [first attempt: <error>]";
//                       when the retry fails as well: the FIRST error with the second status
//   nothing moved       installed, not verified
//   a bad verification  a first device path in the automatic mode goes once more through host memory (said through `trace`); any other:
//                       CP2_ERR_HIP, "exchange verification failed (<note>): <bad>"
template <typename Exchange, typename Install, typename Verify, typename Trace>
int exchange_until_verified(int gather_mode, size_t world, std::string& note, std::string& err, Exchange exchange, Install install, Verify verify, Trace trace) {
  for (int attempt = 0; attempt < 2; ++attempt) {
    ExchangeOutcome r = exchange(attempt == 1);
    if (r.status != CP2_OK) {
      if (!exchange_may_retry_on_host(r.status, r.timed_out, gather_mode, world, attempt)) return r.status;
      const std::string first = err;   // the device path broke (NOT: timed out)
      err.clear();
      attempt = 1;
      r = exchange(true);
      if (r.status != CP2_OK) { err = first; return r.status; }
      note += " [first attempt: " + first + "]";
    }
    if (const int st = install(r); st != CP2_OK) return st;
    if (!r.moved) return CP2_OK;
    std::string bad;
    if (const int st = verify(r, bad); st != CP2_OK) return st;
    if (bad.empty()) return CP2_OK;
    if (attempt == 1 || gather_mode != CP2_GATHER_AUTO || !r.on_device) {
      err = "exchange verification failed (" + note + "): " + bad;
      return CP2_ERR_HIP;
    }
    trace("exchange verification FAILED (" + note + ": " + bad + "): once more through host memory");
  }
  return CP2_ERR_HIP;   // not reached
}

}  // namespace cp2i
