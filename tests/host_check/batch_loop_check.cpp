// csrc/batch_loop.hpp on the CPU, under AddressSanitizer + UBSan (tests/test_host_check.py compiles and runs this): no HIP, no device.
// batch_loop -- the one loop the compact / roots-only build, the batched streamed build, the scrub and build many run their batches
// through -- driven with a stand-in device that MODELS the two node buffers: buffer b is busy from the build of a batch in it until the
// event recorded after that build has been waited for, or the device drained.  Walked over
//   n_items 0..9 x batch 1..4                        no batch, exactly one, exactly two, an odd tail, n_items < batch
//   x no failure, or a failure of one step kind (wait, reuse, build, after, record, drain) at one batch, with one of four statuses
// and every run's log of calls compared, call by call, with what the contract in the header's comment says; then one long run for the
// progress callback.  Every build makes a heap object that only release() frees: a batch object the loop drops is a leak the sanitizer
// reports, one it releases twice a double free.
#include <cstdio>
#include <string>
#include <vector>

#include "batch_loop.hpp"

using namespace cp2i;

namespace {

enum Kind { Wait, Reuse, Build, After, Record, Drain, Release, Progress, None };
const char* const KIND_NAME[] = {"wait", "reuse", "build", "after", "record", "drain", "release", "progress", "none"};
const char* const WHAT = "check";
const std::string UNTOUCHED = "no error yet";

struct Call { Kind kind; size_t k, s0, n; int b; long tail; };   // what a call was given (device calls know only b and the tail)

struct Run {
  size_t n_items = 0, batch = 1;
  Kind fail = None;
  size_t fail_k = 0;
  int fail_status = CP2_OK;
  // what happened
  std::vector<Call> log;
  std::string err = UNTOUCHED;
  std::string wrong;           // the first thing the model saw go wrong
  int status = CP2_OK;
  size_t n_batches = ~(size_t)0;
  size_t step_k = 0;           // the batch the callers' callables were last called for (the device's calls belong to it)
  void note(const std::string& w) { if (wrong.empty()) wrong = w; }
  int outcome(Kind kind, size_t k) {
    if (kind != fail || (kind != Drain && k != fail_k)) return CP2_OK;
    if (kind != Wait && kind != Drain) err = std::string("injected ") + KIND_NAME[kind];   // (a failed wait or drain: the loop's own text)
    return fail_status;
  }
};

struct Device {
  using Tail = long;
  Run& r;
  int* batch = nullptr;                           // the batch object of the current step
  bool busy[2] = {false, false};
  size_t built[2] = {0, 0}, recorded[2] = {0, 0};   // generation of the last build in buffer b, and the one its event covers (0: none)
  size_t generation = 0, live = 0, releases = 0;
  explicit Device(Run& run) : r(run) {}
  ~Device() { delete batch; }
  int wait(int b) {
    r.log.push_back({Wait, r.step_k + 1, 0, 0, b, 0});   // (called before reuse: for the batch after the last one the callables saw)
    if (recorded[b] == 0) r.note("wait for an event that was never recorded");
    if (recorded[b] == built[b]) busy[b] = false;
    return r.outcome(Wait, r.log.back().k);
  }
  int record(int b, long tail) {
    r.log.push_back({Record, r.step_k, 0, 0, b, tail});
    recorded[b] = built[b];
    return r.outcome(Record, r.step_k);
  }
  int drain() {
    r.log.push_back({Drain, 0, 0, 0, 0, 0});
    busy[0] = busy[1] = false;
    return r.outcome(Drain, 0);
  }
  void release() {
    r.log.push_back({Release, r.step_k, 0, 0, 0, 0});
    if (!batch) r.note("release without a batch object");
    delete batch;
    batch = nullptr;
    ++releases;
  }
  void use(const BatchStep& s, const char* who) {
    if (busy[s.b]) r.note(std::string(who) + " saw a busy buffer");
  }
};

void run(Run& r) {
  Device dev(r);
  bool first = true;
  r.status = batch_loop(dev, WHAT, r.err, r.n_items, r.batch,
      [&](const BatchStep& s) {
        r.step_k = s.k;
        if (first && s.k != 0) r.note("the first batch is not batch 0");
        first = false;
        r.log.push_back({Reuse, s.k, s.s0, s.n, s.b, 0});
        dev.use(s, "reuse");
        return r.outcome(Reuse, s.k);
      },
      [&](const BatchStep& s, long* tail) {
        r.log.push_back({Build, s.k, s.s0, s.n, s.b, 0});
        dev.use(s, "build");
        if (dev.batch) r.note("build with the batch object of an earlier step still there");
        dev.batch = new int((int)s.k);
        dev.busy[s.b] = true;
        dev.built[s.b] = ++dev.generation;
        *tail = 100 + (long)s.k;
        return r.outcome(Build, s.k);
      },
      [&](const BatchStep& s, long tail) {
        r.log.push_back({After, s.k, s.s0, s.n, s.b, tail});
        if (!dev.batch || *dev.batch != (int)s.k) r.note("after without its batch object");
        return r.outcome(After, s.k);
      },
      [&](const BatchStep& s) { r.log.push_back({Progress, s.k, s.s0, s.n, s.b, 0}); }, &r.n_batches);
  if (r.status == CP2_OK && (dev.busy[0] || dev.busy[1])) r.note("a buffer still busy after a run that went well");
  if (dev.batch) r.note("a batch object left with the device");
}

// the log against the contract, call by call; "" when all is as it says
std::string judge(const Run& r) {
  if (!r.wrong.empty()) return r.wrong;
  const size_t nb = (r.n_items + r.batch - 1) / r.batch;
  size_t at = 0;
  bool failed = false;
  size_t ran = 0, covered = 0;
  const auto next = [&](Kind kind) -> const Call* { return at < r.log.size() && r.log[at].kind == kind ? &r.log[at++] : nullptr; };
  const auto fails = [&](Kind kind, size_t k) { return r.fail == kind && (kind == Drain || r.fail_k == k); };
  for (size_t k = 0; k < nb && !failed; ++k) {
    const size_t s0 = k * r.batch, n = std::min(r.batch, r.n_items - s0);
    const int b = (int)(k & 1);
    const long tail = 100 + (long)k;
    const auto same = [&](const Call* c) { return c && c->k == k && c->s0 == s0 && c->n == n && c->b == b; };
    ++ran;
    if (k >= 2) {
      const Call* c = next(Wait);
      if (!c || c->b != b) return "no wait(b) before batch " + std::to_string(k);
      if (fails(Wait, k)) { failed = true; break; }
    }
    if (!same(next(Reuse))) return "reuse of batch " + std::to_string(k) + " missing, out of order or with another (s0, n, b)";
    if (fails(Reuse, k)) { failed = true; break; }
    if (!same(next(Build))) return "build of batch " + std::to_string(k) + " missing, out of order or with another (s0, n, b)";
    covered += n;
    bool ok = !fails(Build, k);
    if (ok) {
      const Call* c = next(After);
      if (!same(c) || c->tail != tail) return "after of batch " + std::to_string(k) + " missing, out of order, or not on the tail its build reported";
      ok = !fails(After, k);
    }
    if (ok) {
      const Call* c = next(Record);
      if (!c || c->b != b || c->tail != tail) return "record of batch " + std::to_string(k) + " missing, out of order, or not on the batch's tail";
      ok = !fails(Record, k);
    }
    if (!next(Release)) return "the batch object of batch " + std::to_string(k) + " was not released after its steps";
    if (!ok) { failed = true; break; }
    const bool due = (k % 32) == 31 || k + 1 == nb;
    const Call* p = next(Progress);
    if (due != (p != nullptr) || (p && !same(p))) return "progress after batch " + std::to_string(k);
  }
  if (!failed) {
    if (covered != r.n_items) return "the batches do not tile [0, n_items)";
    if (!next(Drain)) return "no drain after the last batch";
    if (fails(Drain, 0)) failed = true;
  }
  if (at != r.log.size()) return std::string("a call after the run should have ended: ") + KIND_NAME[r.log[at].kind];
  if (r.n_batches != ran) return "the reported batch count";
  const bool device_step = r.fail == Wait || r.fail == Drain;
  const int want_status = !failed ? CP2_OK : (device_step ? CP2_ERR_HIP : r.fail_status);
  const std::string want_err = !failed ? UNTOUCHED : (device_step ? std::string(WHAT) + ": a batch failed on the device" : std::string("injected ") + KIND_NAME[r.fail]);
  if (failed != (r.fail != None)) return "the injected failure was not reached";
  if (r.status != want_status) return "the status";
  if (r.err != want_err) return "the error text";
  return "";
}

}  // namespace

int main() {
  size_t runs = 0, failing = 0, wrong = 0, batches = 0;
  const auto check = [&](Run& r) {
    run(r);
    ++runs;
    failing += r.fail != None;
    batches += r.n_batches;
    const std::string why = judge(r);
    if (why.empty()) return;
    ++wrong;
    std::printf("WRONG (%s): %zu items in batches of %zu, %s failing at batch %zu with status %d -> status %d, %zu batch(es), error \"%s\", %zu call(s)\n",
                why.c_str(), r.n_items, r.batch, KIND_NAME[r.fail], r.fail_k, r.fail_status, r.status, r.n_batches, r.err.c_str(), r.log.size());
  };
  for (size_t n_items = 0; n_items <= 9; ++n_items)
    for (size_t batch = 1; batch <= 4; ++batch) {
      const size_t nb = (n_items + batch - 1) / batch;
      Run plain;
      plain.n_items = n_items;
      plain.batch = batch;
      check(plain);
      for (int kind = Wait; kind <= Drain; ++kind)
        for (size_t k = kind == Wait ? 2 : 0; k < (kind == Drain ? 1 : nb); ++k)
          for (int status : {CP2_ERR_HIP, CP2_ERR_ALLOC, CP2_ERR_IO, CP2_ERR_INVALID}) {
            Run r;
            r.n_items = n_items;
            r.batch = batch;
            r.fail = (Kind)kind;
            r.fail_k = k;
            r.fail_status = status;
            check(r);
          }
    }
  // one long run: the progress callback on batches 31, 63 and the last
  Run longrun;
  longrun.n_items = 70;
  check(longrun);
  std::vector<size_t> progress;
  for (const Call& c : longrun.log)
    if (c.kind == Progress) progress.push_back(c.k);
  if (progress != std::vector<size_t>{31, 63, 69}) {
    ++wrong;
    std::printf("WRONG: the long run's progress lines came after %zu batch(es), not after batches 31, 63 and 69\n", progress.size());
  }
  std::printf("batch loop %s: %zu runs, %zu of them with a failing step, %zu batches, %zu progress lines in the run of 70\n", wrong ? "WRONG" : "ok", runs,
              failing, batches, progress.size());
  return wrong != 0;
}
