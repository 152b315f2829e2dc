// csrc/exchange_policy.hpp on the CPU, under AddressSanitizer + UBSan (tests/test_boundary_version.py compiles and runs this): no HIP, no
// device.  exchange_until_verified -- the one loop csrc/multi_gpu.cpp runs around the exchange of slot roots and of unit roots -- driven
// with stand-in callables over the full product of
//   gather mode (4) x shards (1, 2, 8) x what the first exchange does (7) x what a second one does (2) x install (2) x verify (3)
// and every run compared with the table written out in expected() below, which does not call exchange_may_retry_on_host.
#include <cstdio>
#include <string>
#include <vector>

#include "exchange_policy.hpp"

using namespace cp2i;

namespace {

enum First { OkDevice, OkHost, NothingMoved, ErrHip, ErrHipTimedOut, ErrInvalid, ErrAlloc, N_FIRST };
enum Verify { Good, BadOnce, BadAlways, N_VERIFY };   // BadOnce: the first call of verify finds a fault, a later one does not
const char* const FIRST_NAME[] = {"ok on device", "ok on host", "nothing moved", "ERR_HIP", "ERR_HIP timed out", "ERR_INVALID", "ERR_ALLOC"};

const int RETRY_STATUS = CP2_ERR_IO;        // what a failing second exchange returns: no first exchange of the product returns it
const int INSTALL_STATUS = CP2_ERR_NO_DEVICE;   // what a failing install returns: nothing else does
const std::string FIRST_ERR = "first exchange broke", RETRY_ERR = "second exchange broke", BAD = "rows misplaced";

struct Case { int mode; size_t world; int first; bool retry_ok, install_ok; int verify; };

struct Seen {
  std::vector<bool> force_host;     // one entry per exchange
  int installs = 0, verifies = 0, traces = 0;
  bool after_failed_exchange = false, after_time_out = false;   // install or verify ran although ..., anything ran although ...
  int status = CP2_OK;
  std::string note, err, trace;
};

struct Want {
  std::vector<bool> force_host;
  int installs, verifies, traces, status;
  std::string err_is;        // the whole error text, or ...
  bool err_is_verification;  // ... "exchange verification failed (<note>): <bad>"
  bool suffix;               // the note ends in " [first attempt: <first error>]"
};

// THE TABLE.  Written out case by case from the rules of csrc/exchange_policy.hpp's file comment.
Want expected(const Case& c) {
  const bool automatic = c.mode == CP2_GATHER_AUTO;
  // ---- the first exchange fails
  if (c.first == ErrHipTimedOut) return {{false}, 0, 0, 0, CP2_ERR_HIP, FIRST_ERR, false, false};            // a time-out is final, whatever the mode
  if (c.first == ErrInvalid) return {{false}, 0, 0, 0, CP2_ERR_INVALID, FIRST_ERR, false, false};            // (RCCL by name and unavailable)
  if (c.first == ErrAlloc) return {{false}, 0, 0, 0, CP2_ERR_ALLOC, FIRST_ERR, false, false};
  if (c.first == ErrHip) {
    if (!automatic || c.world == 1) return {{false}, 0, 0, 0, CP2_ERR_HIP, FIRST_ERR, false, false};         // a way asked for by name is never replaced
    if (!c.retry_ok) return {{false, true}, 0, 0, 0, RETRY_STATUS, FIRST_ERR, false, false};                 // the FIRST error, the second status
    if (!c.install_ok) return {{false, true}, 1, 0, 0, INSTALL_STATUS, "", false, true};
    if (c.verify == Good) return {{false, true}, 1, 1, 0, CP2_OK, "", false, true};
    return {{false, true}, 1, 1, 0, CP2_ERR_HIP, "", true, true};                                             // the second exchange's check is final
  }
  // ---- the first exchange succeeds
  if (!c.install_ok) return {{false}, 1, 0, 0, INSTALL_STATUS, "", false, false};
  if (c.first == NothingMoved) return {{false}, 1, 0, 0, CP2_OK, "", false, false};                          // the only skipped verification
  if (c.verify == Good) return {{false}, 1, 1, 0, CP2_OK, "", false, false};
  if (!automatic || c.first == OkHost) return {{false}, 1, 1, 0, CP2_ERR_HIP, "", true, false};              // by name, or host memory already: final
  // automatic mode, a device path failed its check: once more through host memory, said in the trace
  if (!c.retry_ok) return {{false, true}, 1, 1, 1, RETRY_STATUS, RETRY_ERR, false, false};
  if (c.verify == BadOnce) return {{false, true}, 2, 2, 1, CP2_OK, "", false, false};
  return {{false, true}, 2, 2, 1, CP2_ERR_HIP, "", true, false};
}

Seen run(const Case& c) {
  Seen s;
  bool last_failed = false;
  auto exchange = [&](bool force_host) {
    s.force_host.push_back(force_host);
    ExchangeOutcome r;
    if (s.force_host.size() == 1) {
      switch (c.first) {
        case OkDevice: s.note = "copy (device to device)"; r.on_device = true; break;
        case OkHost: s.note = "host (requested)"; break;
        case NothingMoved: s.note = "none (one shard: nothing to exchange)"; r.on_device = true; r.moved = false; break;
        case ErrHip: r.status = CP2_ERR_HIP; break;
        case ErrHipTimedOut: r.status = CP2_ERR_HIP; r.timed_out = true; break;
        case ErrInvalid: r.status = CP2_ERR_INVALID; break;
        default: r.status = CP2_ERR_ALLOC; break;
      }
      if (r.status != CP2_OK) { s.note = "copy (device to device)"; s.err = FIRST_ERR; }
    } else {
      s.note = "host (the device-to-device exchange failed its verification)";
      if (!c.retry_ok) { r.status = RETRY_STATUS; s.err = RETRY_ERR; }
    }
    last_failed = r.status != CP2_OK;
    if (r.timed_out) s.after_time_out = true;
    return r;
  };
  auto install = [&](const ExchangeOutcome& r) -> int {
    ++s.installs;
    if (last_failed || r.status != CP2_OK) s.after_failed_exchange = true;
    return c.install_ok ? CP2_OK : INSTALL_STATUS;
  };
  auto verify = [&](const ExchangeOutcome& r, std::string& bad) -> int {
    ++s.verifies;
    if (last_failed || r.status != CP2_OK) s.after_failed_exchange = true;
    if (c.verify == BadAlways || (c.verify == BadOnce && s.verifies == 1)) bad = BAD;
    return CP2_OK;
  };
  auto trace = [&](const std::string& line) { ++s.traces; s.trace = line; };
  s.status = exchange_until_verified(c.mode, c.world, s.note, s.err, exchange, install, verify, trace);
  return s;
}

}  // namespace

int main() {
  size_t runs = 0, wrong = 0, retried = 0, verified_failures = 0;
  for (int mode : {CP2_GATHER_AUTO, CP2_GATHER_RCCL, CP2_GATHER_HOST, CP2_GATHER_COPY})
    for (size_t world : {(size_t)1, (size_t)2, (size_t)8})
      for (int first = 0; first < N_FIRST; ++first)
        for (int retry_ok = 0; retry_ok < 2; ++retry_ok)
          for (int install_ok = 0; install_ok < 2; ++install_ok)
            for (int verify = 0; verify < N_VERIFY; ++verify) {
              const Case c{mode, world, first, retry_ok != 0, install_ok != 0, verify};
              const Want w = expected(c);
              const Seen s = run(c);
              ++runs;
              const std::string suffix = " [first attempt: " + FIRST_ERR + "]";
              const bool has_suffix = s.note.size() >= suffix.size() && s.note.compare(s.note.size() - suffix.size(), suffix.size(), suffix) == 0;
              const bool any_suffix = s.note.find(" [first attempt: ") != std::string::npos;
              std::string why;
              if (s.force_host.size() > 2) why = "more than two exchanges";
              else if (s.force_host != w.force_host) why = "the exchanges or their force_host";
              else if (s.installs != w.installs) why = "how often install ran";
              else if (s.verifies != w.verifies) why = "how often verify ran";
              else if (s.traces != w.traces) why = "how often the trace line was written";
              else if (s.after_failed_exchange) why = "install or verify ran on a failed exchange";
              else if (first == ErrHipTimedOut && (s.force_host.size() != 1 || s.installs || s.verifies || s.traces)) why = "something ran after a time-out";
              else if (s.status != w.status) why = "the status";
              else if (w.err_is_verification && s.err != "exchange verification failed (" + s.note + "): " + BAD) why = "the verification's error text";
              else if (!w.err_is_verification && s.err != w.err_is) why = "the error text";
              else if (has_suffix != w.suffix || any_suffix != w.suffix) why = "the note's [first attempt: ...] suffix";
              else if (w.traces && s.trace != "exchange verification FAILED (copy (device to device): " + BAD + "): once more through host memory") why = "the trace line";
              if (!why.empty()) {
                ++wrong;
                std::printf("WRONG (%s): mode %d, %zu shard(s), first %s, retry %s, install %s, verify %d -> status %d, %zu exchange(s), %d install(s), %d verif.,"
                            " note \"%s\", error \"%s\"\n", why.c_str(), mode, world, FIRST_NAME[first], retry_ok ? "ok" : "fails", install_ok ? "ok" : "fails", verify,
                            s.status, s.force_host.size(), s.installs, s.verifies, s.note.c_str(), s.err.c_str());
              }
              retried += s.force_host.size() == 2;
              verified_failures += w.err_is_verification;
            }
  std::printf("exchange loop %s: %zu runs, %zu with a second exchange, %zu ending in a failed verification\n", wrong ? "WRONG" : "ok", runs, retried,
              verified_failures);
  return wrong != 0;
}
