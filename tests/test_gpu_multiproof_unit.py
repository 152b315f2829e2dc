"""GPU suite: launch_multiproof_layers and launch_multiproof_commit on their own (csrc/kernels.hpp), through the forwarders of
tests/device_check/multiproof_unit.hip.

cp2_blocks_verify_multi reaches k_multiproof_layer only behind a host that hashes candidates first; here the launcher gets its tables
directly (tests/multiproof_models.py makes them), and the work table of a case is ONE torch allocation with guard rows in front and behind;
the stated roots and the verdict words have guards too, the verdicts pre-filled with 0xA5A5A5A5.  The WHOLE buffer is compared: every
computed row must be the C oracle's tree node at its (level, index), leaf rows, sent rows and guards must be unchanged, and every verdict
must be exact.  In every case of more than one group between 15 % and 40 % of the stated roots are wrong -- in the lowest byte only, in
the top limb only, or swapped with the next group's, every kind in every such case --: their verdicts must be 1, their rows still stored as
computed, all other verdicts 0.

Shapes (tests/multiproof_models.py: cases): block counts from {1, 2, 3, 4, 5, 7, 8, 9, 16, 33, 64, 257}; per group one block, the last
block (of an odd layer where the count is odd), all blocks, every second block or a seeded random half; level 0 has 1, 63, 64, 65, 255, 256,
257 and 4097 jobs; groups of many depths share a case, so they end at different levels and their comparison falls in different launches;
at least three cases have a wave whose jobs belong to four or more groups of at least three depths and mix odd-tail, inner and comparing
jobs.  launch_multiproof_commit: 1, 64, 65 and 4097 lanes into a guarded destination buffer; the rows of proved groups land exactly, those
of failed groups leave their destinations untouched, and two lanes name one destination."""
import ctypes
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import multiproof_models as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libmultiproof_unit.so")
HIP_INVALID = 1                               # hipErrorInvalidValue
GUARD = 3                                     # rows in front of and behind the work table and the roots, words around the verdicts
UNWRITTEN = 0xA5A5A5A5                        # what every verdict word holds before the launch


@pytest.fixture(autouse=True)
def time_limit():
    """every test under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


class Layout:
    """The buffers of one case.  image: GUARD rows, the work table, GUARD rows -- a pattern everywhere, the groups' leaves and sent rows
    from oracle trees over random leaves --; want: what it must hold afterwards.  roots: GUARD rows, one stated root per group, GUARD
    rows; verdict: GUARD words, one per group, GUARD words.  oracle None: the plan only (which roots are wrong, and how)."""

    def __init__(self, c, oracle, all_true=False):
        rng = np.random.default_rng([0x3B3B, c.no])
        self.case, self.plan = c, M.Plan(c.groups)
        p, ng = self.plan, len(c.groups)
        self.image = rng.integers(0, 256, size=(p.n_work + 2 * GUARD, 32), dtype=np.uint8)
        self.roots = rng.integers(0, 256, size=(ng + 2 * GUARD, 32), dtype=np.uint8)
        self.verdict0 = np.full(ng + 2 * GUARD, UNWRITTEN, dtype=np.uint32)
        self.wrong = M.wrong_roots(ng, rng) if ng > 1 and not all_true else {}
        if oracle is None:
            return
        trees = []
        for n, _ in p.groups:
            leaves = np.zeros((n, 32), dtype=np.uint8)
            leaves[:, :31] = rng.integers(0, 256, size=(n, 31), dtype=np.uint8)
            trees.append(oracle.merkle_tree(leaves))
            assert [len(x) for x in trees[-1]] == M.layer_sizes(n)
        self.want = self.image.copy()
        for r in range(p.n_work):                          # leaves and sent rows are given, every row above them is expected
            g, level, index = p.node[r]
            self.want[GUARD + r] = trees[g][level][index]
            if r < p.n + p.n_rows:
                self.image[GUARD + r] = trees[g][level][index]
        stated = np.stack([t[-1][0] for t in trees])
        g = 0
        while g < ng:
            kind = self.wrong.get(g)
            if kind == "low byte":
                stated[g, 0] ^= 1
            elif kind == "top limb":
                stated[g, 28] ^= 1
            elif kind == "swapped":                        # a swapped pair is two neighbours, both marked: each pair once
                assert self.wrong.get(g + 1) == "swapped" and not np.array_equal(stated[g], stated[g + 1])
                stated[[g, g + 1]] = stated[[g + 1, g]]
                g += 1
            g += 1
        self.roots[GUARD:GUARD + ng] = stated
        self.want_verdict = self.verdict0.copy()
        for g in range(ng):
            self.want_verdict[GUARD + g] = int(g in self.wrong)


def test_the_plan_holds_the_shapes_it_claims():
    cs = M.cases()
    plans = [M.Plan(c.groups) for c in cs]
    assert set(M.TOTALS) <= {len(p.jobs[0]) for p in plans}
    assert {n for c in cs for n, _ in c.groups} == set(M.BLOCKS)
    for n in M.BLOCKS:                                                              # every kind of B for every block count
        sets = {tuple(B) for c in cs for m, B in c.groups if m == n}
        assert (n - 1,) in sets and tuple(range(n)) in sets and tuple(range(0, n, 2)) in sets
        assert any(len(B) == max(1, n // 2) for B in sets) and any(len(B) == 1 for B in sets)
    assert any(n % 2 == 1 and B == [n - 1] for c in cs for n, B in c.groups if n > 1)   # the last block of an odd layer
    mixed = sum(any(M.mixed_wave(p, level, w) for level in range(len(p.jobs)) for w in range((len(p.jobs[level]) + M.WAVE - 1) // M.WAVE)) for p in plans)
    assert mixed >= 3
    assert any(len(p.jobs[0]) > 4096 for p in plans)                                # many workgroups
    for c, p in zip(cs, plans):
        assert sorted(p.top) == list(range(len(c.groups)))                          # every group has its one comparing job
        assert all(sum(1 for jobs in p.jobs for j in jobs if j[3] == g and j[2] >> 8) == 1 for g in range(len(c.groups)))
        for l, jobs in enumerate(p.jobs):                                           # reads below the level's base, writes from it
            assert all(j[0] < p.level_base[l] and (j[1] == M.ZERO or j[1] < p.level_base[l]) for j in jobs)
        if len(c.groups) > 1:
            lay = Layout(c, None)
            assert len(c.groups) >= 10 and len({M.depth(n) for n, _ in c.groups}) >= 3
            assert set(lay.wrong.values()) == {"low byte", "top limb", "swapped"}
            assert 0.15 * len(c.groups) <= len(lay.wrong) <= 0.40 * len(c.groups)
            swapped = sorted(g for g, k in lay.wrong.items() if k == "swapped")
            assert len(swapped) % 2 == 0 and all(b == a + 1 for a, b in zip(swapped[::2], swapped[1::2]))


@pytest.fixture(scope="module")
def mpu(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/libmultiproof_unit.so"],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(LIB)
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    lib.mpu_multiproof_layers.restype, lib.mpu_multiproof_layers.argtypes = ctypes.c_int, [vp, u64, vp, vp, vp, sz, vp, vp]
    return lib


@pytest.fixture(scope="module")
def torch_(mpu):
    import torch
    yield torch
    torch.cuda.synchronize()


def up(torch, arr):
    a = np.array(arr, copy=True, order="C")
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


def hp(a):
    return a.ctypes.data if a.size else None


def launch(torch, lib, lay, shift=None, null=None, jobs=None, want=None, level_base=None, n_work=None):
    """the launch of a case; shift / null: the name of one device table passed misaligned / as NULL; jobs, want, level_base, n_work: tables
    in place of the plan's.  Returns (status, rows, roots, verdicts)"""
    p = lay.plan
    d_rows, d_roots, d_verdict = up(torch, lay.image), up(torch, lay.roots), up(torch, lay.verdict0)
    tab, off, base = p.tables()
    tab = tab if jobs is None else jobs
    base = base if level_base is None else level_base
    addr = np.array([d_roots.data_ptr() + 32 * (GUARD + g) for g in range(len(p.groups))], dtype=np.uint64) if want is None else want(d_roots.data_ptr())
    dev = {"jobs": up(torch, tab), "want": up(torch, addr)}
    ptr = {k: v.data_ptr() for k, v in dev.items()}
    ptr["work"] = d_rows.data_ptr() + 32 * GUARD
    ptr["verdict"] = d_verdict.data_ptr() + 4 * GUARD
    if shift:
        ptr[shift] += {"work": 8, "jobs": 8, "want": 4, "verdict": 2}[shift]
    if null:
        ptr[null] = None
    st = lib.mpu_multiproof_layers(ptr["work"], p.n_work if n_work is None else n_work, ptr["jobs"], hp(off), hp(base), len(base), ptr["want"],
                                   ptr["verdict"])
    torch.cuda.synchronize()
    return st, d_rows.cpu().numpy().reshape(-1, 32), d_roots.cpu().numpy().reshape(-1, 32), d_verdict.cpu().numpy().view(np.uint32)


def test_groups_against_the_oracle_with_guard_rows(mpu, torch_, oracle, capsys):
    c_oracle, _ = oracle
    bad, cs = [], M.cases()
    for c in cs:
        lay = Layout(c, c_oracle)
        st, got, roots, verdict = launch(torch_, mpu, lay)
        p = lay.plan
        what = "case %d (%d groups, %d leaves, %d sent rows, %d jobs, %d stated roots wrong)" % (c.no, len(c.groups), p.n, p.n_rows, p.computed(),
                                                                                                 len(lay.wrong))
        if st != 0:
            bad.append("%s: status %d" % (what, st))
            continue
        if not np.array_equal(got, lay.want):
            rows = np.nonzero((got != lay.want).any(axis=1))[0]
            bad.append("%s: %d rows differ, first row %d" % (what, rows.size, int(rows[0])))
        if not np.array_equal(roots, lay.roots):
            bad.append("%s: the stated roots were written" % what)
        if not np.array_equal(verdict, lay.want_verdict):
            at = np.nonzero(verdict != lay.want_verdict)[0]
            bad.append("%s: %d verdict words differ, first word %d: %#x for %#x" % (what, at.size, int(at[0]), int(verdict[at[0]]),
                                                                                  int(lay.want_verdict[at[0]])))
    with capsys.disabled():
        print("\n[multiproof unit] %d cases checked, 0 skipped, %d failed" % (len(cs), len(bad)))
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad))


SMALL = M.Case(97, [(1, [0]), (5, [0, 4]), (9, [8]), (4, [0, 1, 2, 3]), (3, [1])])


def test_a_stated_root_plus_r_matches_and_a_missing_one_does_not(mpu, torch_, oracle):
    """the comparison is of field elements; a want_addr that is 0 or misaligned is a mismatch, the row still stored as computed"""
    c_oracle, _ = oracle
    lay = Layout(SMALL, c_oracle, all_true=True)
    g = next(g for g in range(5) if int.from_bytes(lay.roots[GUARD + g].tobytes(), "little") + M.R_MOD < 1 << 256)
    v = int.from_bytes(lay.roots[GUARD + g].tobytes(), "little") + M.R_MOD
    lay.roots[GUARD + g] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)
    st, got, roots, verdict = launch(torch_, mpu, lay)
    assert st == 0 and np.array_equal(got, lay.want) and np.array_equal(verdict, lay.want_verdict) and np.array_equal(roots, lay.roots)

    def holes(base):
        a = np.array([base + 32 * (GUARD + k) for k in range(5)], dtype=np.uint64)
        a[1], a[3] = 0, a[3] + 8
        return a
    want_verdict = lay.want_verdict.copy()
    want_verdict[GUARD + 1] = want_verdict[GUARD + 3] = 1
    st, got, roots, verdict = launch(torch_, mpu, lay, want=holes)
    assert st == 0 and np.array_equal(got, lay.want) and np.array_equal(verdict, want_verdict)


def test_a_job_that_names_a_row_at_or_past_its_base_stores_nothing(mpu, torch_, oracle):
    """the kernel's guard: such a job reads and stores nothing, and with `last` set its group's verdict is 1"""
    c_oracle, _ = oracle
    lay = Layout(SMALL, c_oracle, all_true=True)
    p = lay.plan
    tab, _, base = p.tables()
    k = p.level_off[1] - 1                             # the last job of level 0: group 4 (three blocks: not yet its top)
    last0 = next(i for i in range(p.level_off[1]) if tab[i, 2] >> 8)   # a comparing job of level 0 (a one-block or two-block group)
    tab[k, 0], tab[last0, 1] = base[0], base[0] + 5
    st, got, roots, verdict = launch(torch_, mpu, lay, jobs=tab)
    assert st == 0
    for j in (k, last0):                               # neither row is written
        assert np.array_equal(got[GUARD + int(base[0]) + j], lay.image[GUARD + int(base[0]) + j])
    assert verdict[GUARD + tab[last0, 3]] == 1 and verdict[GUARD + tab[k, 3]] == 1      # the latter: its top hashed an unwritten row
    assert np.array_equal(got[:GUARD + p.n + p.n_rows], lay.image[:GUARD + p.n + p.n_rows]) and np.array_equal(got[-GUARD:], lay.image[-GUARD:])
    assert (verdict[:GUARD] == UNWRITTEN).all() and (verdict[-GUARD:] == UNWRITTEN).all()


def test_refusals_and_no_work(mpu, torch_, oracle):
    c_oracle, _ = oracle
    lay = Layout(SMALL, c_oracle, all_true=True)
    p = lay.plan

    def untouched(st, got, roots, verdict):
        return st == HIP_INVALID and np.array_equal(got, lay.image) and np.array_equal(roots, lay.roots) and np.array_equal(verdict, lay.verdict0)

    for name in ("work", "jobs", "want", "verdict"):
        assert untouched(*launch(torch_, mpu, lay, null=name)), "NULL " + name          # a NULL table with work to do
        assert untouched(*launch(torch_, mpu, lay, shift=name)), "misaligned " + name   # each table misaligned
    _, off, base = p.tables()
    low = base.copy()
    low[1] = base[0]                                                                   # a level that writes what the one before wrote
    assert untouched(*launch(torch_, mpu, lay, level_base=low))
    assert untouched(*launch(torch_, mpu, lay, n_work=p.n_work - 1))                   # output past the end of the table
    high = base.copy()
    high[-1] = M.ROW_LIMIT - 1                                                         # rows that reach 2^32 - 1
    assert untouched(*launch(torch_, mpu, lay, level_base=high, n_work=1 << 33))
    f = mpu.mpu_multiproof_layers
    zero = np.zeros(4, dtype=np.uint64)
    assert f(None, 0, None, None, None, 0, None, None) == 0                            # no levels: no work
    assert f(None, 0, None, hp(zero), hp(zero), 3, None, None) == 0                    # levels without jobs: no work
    assert f(None, 0, None, None, None, 2, None, None) == HIP_INVALID                  # levels without their host tables
    down = off.copy()
    down[1] = off[2] + 1
    assert f(None, 0, None, hp(down), hp(base), len(base), None, None) == HIP_INVALID  # level_off that descends
    st, got, roots, verdict = launch(torch_, mpu, lay)                                 # and the same arguments, valid
    assert st == 0 and np.array_equal(got, lay.want) and np.array_equal(verdict, lay.want_verdict)


# ---- launch_multiproof_commit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65, 4097])
def test_commit_copies_the_rows_of_proved_groups_only(mpu, torch_, n):
    """n lanes over a work table of n + 7 rows and a guarded destination buffer: rows of proved groups land exactly, rows of failed groups
    leave their destinations untouched, two lanes may name one destination (they carry the same row), and a lane whose source row, group
    or destination is out of range copies nothing"""
    mpu.mpu_multiproof_commit.restype = ctypes.c_int
    mpu.mpu_multiproof_commit.argtypes = [ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 4 + [ctypes.c_uint32, ctypes.c_size_t]
    rng = np.random.default_rng([0xC0, n])
    n_work, n_groups, n_dst = n + 7, max(2, n // 9), n + 5
    work = rng.integers(0, 256, size=(n_work, 32), dtype=np.uint8)
    image = rng.integers(0, 256, size=(n_dst + 2 * GUARD, 32), dtype=np.uint8)
    verdict = rng.integers(0, 3, size=n_groups + 2 * GUARD).astype(np.uint32)       # 0 proved, 1 and 2 not
    verdict[GUARD] = 0
    src = rng.permutation(n_work)[:n].astype(np.uint32)
    group = rng.integers(0, n_groups, size=n).astype(np.uint32)
    place = rng.permutation(n_dst)[:n]
    if n > 2:                                                                       # two lanes, one destination, one source row
        group[1] = group[0] = 0
        src[1], place[1] = src[0], place[0]
    d_work, d_image, d_verdict = up(torch_, work), up(torch_, image), up(torch_, verdict)
    dst = (d_image.data_ptr() + 32 * (GUARD + place)).astype(np.uint64)
    want = image.copy()
    odd = {}
    if n > 8:                                                                       # lanes that must copy nothing, whatever their group says
        src[3], dst[4], dst[5], group[6] = n_work, 0, dst[5] + 8, n_groups
        odd = {3, 4, 5, 6}
    for i in range(n):
        if i not in odd and verdict[GUARD + group[i]] == 0:
            want[GUARD + place[i]] = work[src[i]]
    tabs = [up(torch_, a) for a in (src, dst, group)]
    st = mpu.mpu_multiproof_commit(d_work.data_ptr(), n_work, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), d_verdict.data_ptr() + 4 * GUARD,
                                   n_groups, n)
    torch_.cuda.synchronize()
    assert st == 0
    assert np.array_equal(d_image.cpu().numpy().reshape(-1, 32), want) and not np.array_equal(want, image)
    assert np.array_equal(d_work.cpu().numpy().reshape(-1, 32), work) and np.array_equal(d_verdict.cpu().numpy().view(np.uint32), verdict)
    f = mpu.mpu_multiproof_commit
    assert f(None, 0, None, None, None, None, 0, 0) == 0                               # no lanes: no work
    assert f(None, n_work, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), d_verdict.data_ptr(), n_groups, n) == HIP_INVALID
    assert f(d_work.data_ptr() + 8, n_work, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), d_verdict.data_ptr(), n_groups, n) == HIP_INVALID
    torch_.cuda.synchronize()
    assert np.array_equal(d_image.cpu().numpy().reshape(-1, 32), want)
