"""GPU suite: launch_multiproof_tops on its own, and behind launch_multiproof_layers (csrc/kernels.hpp), through the forwarders of
tests/device_check/multiproof_anchor_unit.hip.

cp2_fill_add_multi_anchored reaches k_multiproof_tops and k_multiproof_fold only behind a host that hashes candidates first; here the
launcher gets its tables directly (tests/multiproof_anchor_models.py makes them).  The work table and the kept rows of a case are torch
allocations with guard rows in front and behind; both verdict arrays have guard words and are pre-filled with 0xA5A5A5A5.  WHOLE buffers are
compared: the work table and the kept rows must be unchanged, every top_verdict word and every group verdict must be exact -- a group's
verdict is 1 exactly when one of its tops is wrong.

Shapes (tops_cases): 1, 63, 64, 65, 257 and 4097 tops; groups of one top, groups whose tops are all at level 0, groups with tops at three or
more levels, ranges that straddle wave and workgroup boundaries.  Wrong kept rows: in the lowest byte only, in the top limb only, or
swapped with the next top's; in every case of more than one group between 15 % and 40 % of the groups hold a wrong top, at least one group
is all right and one failing group has exactly one wrong top among several (tests/test_multiproof_anchor_cpu.py asserts that of the cases).
Layers and tops together: plans against seeded known sets over oracle trees of 1, 2, 3, 5, 8, 9, 33 and 257 blocks, the kept inputs placed
in the table, no job with `last`: every computed row must be the oracle's node at its place.  And the launcher's refusals."""
import ctypes
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import multiproof_anchor_models as A
import multiproof_models as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libmultiproof_anchor_unit.so")
HIP_INVALID = 1                               # hipErrorInvalidValue
GUARD = 3                                     # rows in front of and behind the tables, words around the verdicts
UNWRITTEN = 0xA5A5A5A5                        # what every verdict word holds before the launch


@pytest.fixture(autouse=True)
def time_limit():
    """every test under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def mau(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/libmultiproof_anchor_unit.so"],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(LIB)
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    lib.mau_multiproof_tops.restype, lib.mau_multiproof_tops.argtypes = ctypes.c_int, [vp, u64, vp, vp, sz, vp, vp, sz, vp, vp]
    lib.mau_multiproof_layers.restype, lib.mau_multiproof_layers.argtypes = ctypes.c_int, [vp, u64, vp, vp, vp, sz, vp, vp]
    return lib


@pytest.fixture(scope="module")
def torch_(mau):
    import torch
    yield torch
    torch.cuda.synchronize()


def up(torch, arr):
    a = np.array(arr, copy=True, order="C")
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


def hp(a):
    return a.ctypes.data if a.size else None


def felts(rng, n):
    rows = np.zeros((n, 32), dtype=np.uint8)
    rows[:, :31] = rng.integers(0, 256, size=(n, 31), dtype=np.uint8)
    return rows


def spoil(kept, wrong):
    """kept: the right row of every top, in top order; wrong = {top: kind}"""
    t = 0
    n = kept.shape[0]
    while t < n:
        kind = wrong.get(t)
        if kind == "low byte":
            kept[t, 0] ^= 1
        elif kind == "top limb":
            kept[t, 28] ^= 1
        elif kind == "swapped":                            # a swapped pair is two neighbours, both marked: each pair once
            assert wrong.get(t + 1) == "swapped" and not np.array_equal(kept[t], kept[t + 1])
            kept[[t, t + 1]] = kept[[t + 1, t]]
            t += 1
        t += 1


class Buffers:
    """work: GUARD rows, the table, GUARD rows; kept: GUARD rows, one row per top, GUARD rows; top_verdict and verdict with GUARD words
    around them, all UNWRITTEN.  tops: uint32[n_tops, 2] (row, group); top t is compared with kept row t."""

    def __init__(self, work, top_rows, top_groups, top_off, wrong, rng):
        self.n_work, self.n_tops, self.n_groups = work.shape[0], len(top_rows), len(top_off) - 1
        self.work = rng.integers(0, 256, size=(self.n_work + 2 * GUARD, 32), dtype=np.uint8)
        self.work[GUARD:GUARD + self.n_work] = work
        self.kept = rng.integers(0, 256, size=(self.n_tops + 2 * GUARD, 32), dtype=np.uint8)
        right = work[np.array(top_rows, dtype=np.int64)].copy() if self.n_tops else np.zeros((0, 32), dtype=np.uint8)
        spoil(right, wrong)
        self.kept[GUARD:GUARD + self.n_tops] = right
        self.tops = np.array(list(zip(top_rows, top_groups)), dtype=np.uint32).reshape(-1, 2)
        self.top_off = np.array(top_off, dtype=np.uint64)
        self.top_verdict0 = np.full(self.n_tops + 2 * GUARD, UNWRITTEN, dtype=np.uint32)
        self.verdict0 = np.full(self.n_groups + 2 * GUARD, UNWRITTEN, dtype=np.uint32)
        self.want_top, self.want_verdict = self.top_verdict0.copy(), self.verdict0.copy()
        for t in range(self.n_tops):
            self.want_top[GUARD + t] = int(t in wrong)
        for g in range(self.n_groups):
            self.want_verdict[GUARD + g] = int(any(t in wrong for t in range(top_off[g], top_off[g + 1])))


def launch_tops(torch, lib, b, d_work=None, shift=None, null=None, top_off=None, want=None, n_work=None, n_groups=None):
    """the launch over a case's buffers; shift / null: the name of one device table passed misaligned / as NULL; top_off, want, n_work,
    n_groups in place of the case's.  Returns (status, work, kept, top_verdict, verdict)"""
    d_work = up(torch, b.work) if d_work is None else d_work
    d_kept, d_tv, d_v = up(torch, b.kept), up(torch, b.top_verdict0), up(torch, b.verdict0)
    off = b.top_off if top_off is None else np.array(top_off, dtype=np.uint64)
    addr = np.array([d_kept.data_ptr() + 32 * (GUARD + t) for t in range(b.n_tops)], dtype=np.uint64) if want is None else want(d_kept.data_ptr())
    dev = {"tops": up(torch, b.tops) if b.n_tops else up(torch, np.zeros(2, dtype=np.uint32)), "want": up(torch, addr if addr.size else np.zeros(1, dtype=np.uint64)),
           "d_top_off": up(torch, off)}
    ptr = {k: v.data_ptr() for k, v in dev.items()}
    ptr["work"] = d_work.data_ptr() + 32 * GUARD
    ptr["top_verdict"] = d_tv.data_ptr() + 4 * GUARD
    ptr["verdict"] = d_v.data_ptr() + 4 * GUARD
    ptr["top_off"] = hp(off)
    if shift:
        ptr[shift] += {"work": 8, "tops": 4, "want": 4, "d_top_off": 4, "top_verdict": 2, "verdict": 2}[shift]
    if null:
        ptr[null] = None
    st = lib.mau_multiproof_tops(ptr["work"], b.n_work if n_work is None else n_work, ptr["tops"], ptr["want"], b.n_tops, ptr["top_off"], ptr["d_top_off"],
                                 b.n_groups if n_groups is None else n_groups, ptr["top_verdict"], ptr["verdict"])
    torch.cuda.synchronize()
    return (st, d_work.cpu().numpy().reshape(-1, 32), d_kept.cpu().numpy().reshape(-1, 32), d_tv.cpu().numpy().view(np.uint32),
            d_v.cpu().numpy().view(np.uint32))


def tops_buffers(c):
    """the buffers of one TopsCase: a table of distinct random field elements, twice as many as tops; top t names a seeded row of its own"""
    rng = np.random.default_rng([0x7A7A, c.no])
    work = felts(rng, 2 * c.n_tops + 5)
    rows = [int(r) for r in rng.permutation(work.shape[0])[:c.n_tops]]
    return Buffers(work, rows, [c.group_of(t) for t in range(c.n_tops)], c.top_off, c.wrong, rng)


def differences(what, b, got):
    st, work, kept, tv, v = got
    bad = []
    if st != 0:
        return ["%s: status %d" % (what, st)]
    if not np.array_equal(work, b.work):
        bad.append("%s: the work table was written" % what)
    if not np.array_equal(kept, b.kept):
        bad.append("%s: the kept rows were written" % what)
    if not np.array_equal(tv, b.want_top):
        at = np.nonzero(tv != b.want_top)[0]
        bad.append("%s: %d top_verdict words differ, first word %d: %#x for %#x" % (what, at.size, int(at[0]), int(tv[at[0]]), int(b.want_top[at[0]])))
    if not np.array_equal(v, b.want_verdict):
        at = np.nonzero(v != b.want_verdict)[0]
        bad.append("%s: %d verdict words differ, first word %d: %#x for %#x" % (what, at.size, int(at[0]), int(v[at[0]]), int(b.want_verdict[at[0]])))
    return bad


def test_tops_and_group_verdicts_over_guarded_buffers(mau, torch_, capsys):
    bad, cs = [], A.tops_cases()
    for c in cs:
        b = tops_buffers(c)
        bad += differences("case %d (%d tops, %d groups, %d wrong)" % (c.no, c.n_tops, c.n_groups, len(c.wrong)), b, launch_tops(torch_, mau, b))
    with capsys.disabled():
        print("\n[multiproof anchor unit] %d cases checked, 0 skipped, %d failed" % (len(cs), len(bad)))
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad))


def test_a_kept_row_plus_r_matches_and_defensive_tops_do_not(mau, torch_):
    """the comparison is of field elements; a row at or past n_work and an address that is 0 or misaligned are mismatches and are not read;
    an empty range gives 1"""
    rng = np.random.default_rng(0x7A7B)
    work = felts(rng, 16)
    work[:, 0] |= 1
    b = Buffers(work, [3, 9, 12, 5, 7], [0, 0, 1, 3, 3], [0, 2, 3, 3, 5], {}, rng)
    for t in (0, 3):
        v = int.from_bytes(b.kept[GUARD + t].tobytes(), "little") + M.R_MOD
        assert v < 1 << 256
        b.kept[GUARD + t] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)
    b.want_verdict[GUARD + 2] = 1                          # group 2 has no top
    assert differences("plus r", b, launch_tops(torch_, mau, b)) == []

    def addresses(base):
        a = np.array([base + 32 * (GUARD + t) for t in range(5)], dtype=np.uint64)
        a[1], a[4] = 0, a[4] + 8
        return a
    b2 = Buffers(work, [3, 9, 12, 5, 7], [0, 0, 1, 3, 3], [0, 2, 3, 3, 5], {1: "low byte", 4: "low byte"}, rng)
    b2.kept[GUARD + 1], b2.kept[GUARD + 4] = work[9], work[7]           # the rows are right; their addresses are not
    b2.want_verdict[GUARD + 2] = 1
    assert differences("bad addresses", b2, launch_tops(torch_, mau, b2, want=addresses)) == []
    b3 = Buffers(work, [3, 9, 12, 5, 7], [0, 0, 1, 3, 3], [0, 2, 3, 3, 5], {2: "low byte"}, rng)
    b3.kept[GUARD + 2] = work[12]                          # row 12 is past a table of 12 rows
    b3.want_verdict[GUARD + 2] = 1
    assert differences("a row past n_work", b3, launch_tops(torch_, mau, b3, n_work=12)) == []


def test_the_launcher_refuses_bad_tables_and_launches_nothing(mau, torch_):
    c = A.tops_cases()[2]
    b = tops_buffers(c)

    def untouched(got, what):
        st, work, kept, tv, v = got
        assert st == HIP_INVALID, (what, st)
        assert np.array_equal(work, b.work) and np.array_equal(kept, b.kept) and (tv == UNWRITTEN).all() and (v == UNWRITTEN).all(), what

    for name in ("work", "tops", "want", "d_top_off", "top_verdict", "verdict"):
        untouched(launch_tops(torch_, mau, b, shift=name), "misaligned " + name)
        untouched(launch_tops(torch_, mau, b, null=name), "NULL " + name)
    untouched(launch_tops(torch_, mau, b, null="top_off"), "NULL top_off")
    off = [int(x) for x in b.top_off]
    down = list(off)
    down[2], down[3] = off[3], off[2]
    if down[2] == down[3]:
        down[3] -= 1
    untouched(launch_tops(torch_, mau, b, top_off=down), "top_off descends")
    untouched(launch_tops(torch_, mau, b, top_off=off[:-1] + [off[-1] + 1]), "top_off ends past n_tops")
    st, work, kept, tv, v = launch_tops(torch_, mau, b, n_groups=0)
    assert st == 0 and (tv == UNWRITTEN).all() and (v == UNWRITTEN).all()           # n_groups == 0: success, no launch
    assert differences("the case itself", b, launch_tops(torch_, mau, b)) == []


# ---- layers, then tops ------------------------------------------------------------------------------------------------------------------------
LAYER_BLOCKS = (1, 2, 3, 5, 8, 9, 33, 257)


def layer_groups(rng):
    """per block count three groups: against what presence gives a half-filled slot, against a seeded sparse known set, and against the
    root alone"""
    out = []
    for n in LAYER_BLOCKS:
        half = sorted(int(x) for x in rng.choice(n, size=max(1, n // 2), replace=False))
        for known in (A.derive(n, half), A.random_known(rng, n, 0.2), set()):
            k = int(rng.integers(1, min(n, 40) + 1))
            out.append((n, sorted(int(x) for x in rng.choice(n, size=k, replace=False)), known))
    return out


def test_layers_then_tops_reproduce_the_oracles_nodes(mau, torch_, oracle):
    c_oracle, _ = oracle
    rng = np.random.default_rng(0x7A7C)
    groups = layer_groups(rng)
    p = A.Plan(groups)
    assert p.n_kept > 20 and p.computed() > 100 and len({l for _, _, l, _ in p.tops}) >= 4
    assert not any(j[2] >> 8 for jobs in p.jobs for j in jobs)                      # no job compares
    trees = {}
    for n in LAYER_BLOCKS:
        trees[n] = c_oracle.merkle_tree(felts(rng, n))
    node = lambda r: trees[groups[p.node[r][0]][0]][p.node[r][1]][p.node[r][2]]
    work = rng.integers(0, 256, size=(p.n_work, 32), dtype=np.uint8)
    want = work.copy()
    for r in range(p.n_work):                              # leaves, sent rows and kept inputs are given, every row above them is expected
        want[r] = node(r)
        if r < p.kept_base + p.n_kept:
            work[r] = node(r)
    failing = {g for g in range(len(groups)) if g % 4 == 1}
    wrong = {p.top_off[g + 1] - 1: "low byte" for g in failing}
    b = Buffers(want, [t[0] for t in p.tops], [t[1] for t in p.tops], p.top_off, wrong, rng)
    image = b.work.copy()
    image[GUARD:GUARD + p.n_work] = work
    d_work = up(torch_, image)
    tab, off, base = p.tables()
    d_jobs, d_none = up(torch_, tab), up(torch_, np.full(4, UNWRITTEN, dtype=np.uint32))
    st = mau.mau_multiproof_layers(d_work.data_ptr() + 32 * GUARD, p.n_work, d_jobs.data_ptr(), hp(off), hp(base), len(base), d_none.data_ptr(),
                                   d_none.data_ptr() + 8)
    torch_.cuda.synchronize()
    assert st == 0
    assert (d_none.cpu().numpy().view(np.uint32) == UNWRITTEN).all()                # nothing compared, nothing written beside the rows
    assert differences("layers, then tops", b, launch_tops(torch_, mau, b, d_work=d_work)) == []
