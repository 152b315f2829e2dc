"""GPU suite: the gfx950 build of the field arithmetic one primitive at a time, at the bounds its comments claim.

The device build is not the host build: fr_tie.inc feeds register ties into the optimiser, the column accumulator is a plain
64-bit register with no shadow, CP2_BOUND compiles to nothing, FR_TWO29 and the tables come from __constant__ memory.  So the cases
of tests/test_fr_unit_cpu.py (tests/fr_model.py builds them: limbs at 2.02 U / 2.47 U, columns near 2^64, quotient digits all
ones and all zero, reduce_wide at every table row and where its estimate is one short, every multiple of N through
to_canonical_words, the rounds at the worst case of their comments) run here through tests/device_check/libfr_unit.so, one case
per lane, and are judged by the same big-int model.  Then the device must equal the host twin word for word on those cases and
on a far larger seeded random set per op (2^18 records; round pairs 2^17, permutations 2^16), which needs no big-int work; and
every op runs at n = 1, 63, 64, 65, 257 and the full set with guard words around the output.

No case here is meant to break the kernel: every input is inside the documented bounds of its op, index words are clamped by
the op table, and fru_run refuses an unknown op or an absurd n before anything touches the GPU.

Counts and times: 52 111 model-judged cases (about 12 000 structured, 2000 random per op) and 4 967 311 records compared word
for word (those cases plus the bulk random sets).  On an MI355X the module ran in 5.6 s: 3.4 s for the word-for-word test (numpy
generation and the host twin; the twenty kernels together take milliseconds), 1.3 s generating and judging the model cases.
Its summary line there: "52111 cases judged by the model, 4967311 records compared word for word with the host twin, 0 skipped"."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fr_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libfr_unit.so")
SIZES = (1, 63, 64, 65, 257)
GUARD_ROWS = 4
GUARD_WORD = 0x5EC0DE5E
TALLY = {"judged": 0, "compared": 0, "skipped": 0}


@pytest.fixture(scope="module")
def fru():
    if not os.path.exists(LIB):      # a missing kernel library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/libfr_unit.so"],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(LIB)
    lib.fru_run.restype = ctypes.c_int
    lib.fru_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert lib.fru_n_ops() == len(M.OPS) and lib.fru_record_words() == M.REC
    return lib


def run_device(lib, op, arr):
    """arr: (n, 32) uint32.  The result lands in the middle of a guarded buffer; the guards must come back untouched."""
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    n = arr.shape[0]
    buf = np.full((n + 2 * GUARD_ROWS, M.REC), GUARD_WORD, dtype=np.uint32)
    out = buf[GUARD_ROWS:GUARD_ROWS + n]
    status = lib.fru_run(M.OP_ID[op], arr.ctypes.data_as(ctypes.c_void_p), n, out.ctypes.data_as(ctypes.c_void_p))
    assert status == 0, "%s: fru_run(n=%d) returned %d" % (op, n, status)
    assert (buf[:GUARD_ROWS] == GUARD_WORD).all() and (buf[GUARD_ROWS + n:] == GUARD_WORD).all(), "%s: guard words disturbed at n=%d" % (op, n)
    return out.copy()


def first_difference(op, fams, got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    w = int(np.nonzero(got[i] != want[i])[0][0])
    return "%s/%s: %d of %d records differ from %s; first: case %d word %d: device %#x, %s %#x" % (
        op, fams[i] if fams else "random", bad.size, got.shape[0], what, i, w, int(got[i, w]), what, int(want[i, w]))


@pytest.fixture(scope="module")
def sections():
    M.check_device_constants()
    return M.to_sections(M.build_cases(M.N_RANDOM).items)


@pytest.fixture(scope="module")
def device_results(fru, sections):
    return [run_device(fru, op, arr) for op, _, arr in sections]


@pytest.fixture(scope="module")
def plain_twin(tmp_path_factory):
    return M.build_host_twin(str(tmp_path_factory.mktemp("fr_unit") / "fr_unit_host_plain"), M.PLAIN)


def test_launcher_refuses_what_it_cannot_run(fru):
    """Nothing reaches the GPU for an unknown op, an absurd n or a missing buffer; n = 0 is a no-op."""
    word = np.zeros((1, M.REC), dtype=np.uint32)
    p = word.ctypes.data_as(ctypes.c_void_p)
    assert fru.fru_run(-1, p, 1, p) != 0 and fru.fru_run(len(M.OPS), p, 1, p) != 0
    assert fru.fru_run(0, p, (1 << 24) + 1, p) != 0
    assert fru.fru_run(0, None, 1, p) != 0 and fru.fru_run(0, p, 1, None) != 0
    assert fru.fru_run(0, None, 0, None) == 0


def test_every_case_on_the_device_against_the_model(sections, device_results, oracle):
    judged, failures = M.judge_sections(sections, device_results, M.oracle_permute_both)
    TALLY["judged"] += judged
    assert judged == sum(arr.shape[0] for _, _, arr in sections)
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), judged, "\n".join(failures[:40]))


def test_device_equals_host_twin_word_for_word(fru, sections, device_results, plain_twin, tmp_path):
    host, aborts = M.run_host_twin(plain_twin, sections, tmp_path)
    assert not aborts, "\n".join(aborts)
    failures = []
    for (op, fams, arr), got, want in zip(sections, device_results, host):
        TALLY["compared"] += arr.shape[0]
        failures.append(first_difference(op, fams, got, want, "host twin"))
    for op in M.OPS:
        arr = M.random_records(op, M.BULK_RANDOM[op], 0xB01C)
        for rec in arr[:64].tolist():          # the bulk generator stays inside the op's bounds (spot check; the twin asserts the rest)
            M.PRE[op](rec)
        want, aborts = M.run_host_twin(plain_twin, [(op, None, arr)], tmp_path, tag="bulk")
        assert not aborts, "\n".join(aborts)
        TALLY["compared"] += arr.shape[0]
        failures.append(first_difference(op, None, run_device(fru, op, arr), want[0], "host twin"))
    failures = [f for f in failures if f]
    assert not failures, "\n".join(failures)


def test_every_op_at_partial_waves_and_workgroups(fru, sections, device_results):
    """n = 1, 63, 64, 65, 257: a lone lane, a wave short of one lane, a full wave, a wave and a lane, a workgroup and a lane; the
    i < n guard must hold (guard words around the output, on the host and in the launcher's device buffer)."""
    failures = []
    for (op, fams, arr), full in zip(sections, device_results):
        assert arr.shape[0] >= max(SIZES), op
        for n in SIZES:
            failures.append(first_difference(op, fams, run_device(fru, op, arr[:n]), full[:n], "the full-set run"))
        tail = arr.shape[0] - 65             # the same records in other lanes
        failures.append(first_difference(op, fams[tail:], run_device(fru, op, arr[tail:]), full[tail:], "the full-set run"))
    failures = [f for f in failures if f]
    assert not failures, "\n".join(failures)


def test_summary(sections):
    """Runs last in this module: every case of the plan was judged, none skipped."""
    planned = sum(arr.shape[0] for _, _, arr in sections)
    print("fr_unit on the device: %d cases judged by the model, %d records compared word for word with the host twin, %d skipped"
          % (TALLY["judged"], TALLY["compared"], TALLY["skipped"]))
    assert TALLY["judged"] == planned and TALLY["skipped"] == 0
    assert TALLY["compared"] == planned + sum(M.BULK_RANDOM.values())
