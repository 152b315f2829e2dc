"""GPU suite: launch_finish_layers_many on its own (csrc/kernels.hpp), through the forwarder of tests/device_check/fill_finish_many_unit.hip.

cp2_fills_finish_many reaches k_finish_layer_many only behind a host whose sessions each own an allocation; here the launcher gets its
tables directly (tests/fill_finish_many_models.py makes them), and the sessions of a case lie in ONE torch allocation with guard rows in
front, between and behind; the stated roots and the verdicts have guards too.  The WHOLE buffer is compared: every row above layer 0 must
be the C oracle's Merkle tree of that (session, slot)'s leaves at its layer-major place, layer 0 and all guards must be unchanged, and
every verdict must be exact.  About a quarter of the stated roots are wrong -- in the lowest byte only, in the top limb only, or swapped
with a neighbouring slot's --: their verdicts must be 1, their rows still stored as computed, all other verdicts 0.

Shapes (tests/fill_finish_many_models.py: cases): block counts from {1, 2, 3, 4, 5, 7, 8, 9, 16, 33, 64, 128, 257}, slot counts from {1, 2,
3, 5, 64, 65}; level 0 has 1, 63, 64, 65, 255, 256, 257 and 4097 lanes; the first and the last session are one-block, one-slot; sessions
of at least three depths share a case, so they leave at different levels and their comparison falls in different launches; at least three
cases have a wave whose lanes belong to four or more sessions and mix paired nodes, odd tails, inner lanes and comparing lanes."""
import ctypes
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import fill_finish_many_models as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libfill_finish_many_unit.so")
HIP_INVALID = 1                               # hipErrorInvalidValue
GUARD = 3                                     # rows in front of the first and behind the last session, words around the verdicts
UNWRITTEN = 0xA5A5A5A5                        # what every verdict word holds before the launch


@pytest.fixture(autouse=True)
def time_limit():
    """every test under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def test_the_plan_holds_the_shapes_it_claims():
    cs = M.cases()
    assert set(M.TOTALS) <= {M.plan(c.sessions).level_work[0] for c in cs}
    assert {n for c in cs for n, _ in c.sessions} == set(M.BLOCKS) and {nl for c in cs for _, nl in c.sessions} == set(M.LOCALS)
    for c in cs:
        assert c.sessions[0] == (1, 1) and c.sessions[-1] == (1, 1)
    many = [c for c in cs if len(c.sessions) > 3]
    assert len(many) >= 8 and all(len({M.depth(n) for n, _ in c.sessions}) >= 3 for c in many)   # sessions leave at different levels
    mixed = 0
    for c in cs:                                # a wave with lanes of four sessions: paired and odd-tail, inner and comparing
        p = M.plan(c.sessions)
        mixed += any(M.mixed_wave(p, level, w) for level in range(len(p.level_off)) for w in range((p.level_work[level] + M.WAVE - 1) // M.WAVE))
    assert mixed >= 3
    assert any(M.plan(c.sessions).level_work[0] > 4096 for c in cs)                               # many workgroups
    wrong = [Layout(c, None).wrong for c in cs]
    kinds = {k for w in wrong for k in w.values()}
    assert kinds == {"low byte", "top limb", "swapped"}
    total, bad = sum(sum(nl for _, nl in c.sessions) for c in cs), sum(len(w) for w in wrong)
    assert 0.15 * total <= bad <= 0.40 * total


@pytest.fixture(scope="module")
def ffm(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/libfill_finish_many_unit.so"],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(LIB)
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    lib.ffm_finish_layers_many.restype, lib.ffm_finish_layers_many.argtypes = ctypes.c_int, [vp, u64, vp, vp, vp, vp, vp, vp, sz, vp]
    return lib


@pytest.fixture(scope="module")
def torch_(ffm):
    import torch
    yield torch
    torch.cuda.synchronize()


def up(torch, arr):
    a = np.array(arr, copy=True, order="C")
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


def hp(a):
    return a.ctypes.data if a.size else None


class Layout:
    """The buffers of one case.  rows: GUARD rows, then every session's layer-major buffer with 1 or 2 guard rows after it, GUARD more at
    the end; `image` is what the device starts from (a pattern everywhere, random field elements in layer 0), `want` what it must hold
    afterwards.  roots: the stated roots of all sessions with guard rows likewise; verdict: GUARD words, one per (session, slot), GUARD
    words.  oracle None: the plan only (which roots are wrong, and how)."""

    def __init__(self, c, oracle):
        rng = np.random.default_rng([0xF1F1, c.no])
        ss = c.sessions
        self.sessions, self.plan = ss, M.plan(ss)
        self.first, self.root_first, at, rat = [], [], GUARD, GUARD
        for k, (n, nl) in enumerate(ss):
            self.first.append(at)
            self.root_first.append(rat)
            at += M.rows(n, nl) + 1 + k % 2
            rat += nl + 1 + (k + 1) % 2
        self.rows, self.root_rows = at + GUARD, rat + GUARD
        self.image = rng.integers(0, 256, size=(self.rows, 32), dtype=np.uint8)
        self.want = self.image.copy()
        self.roots = rng.integers(0, 256, size=(self.root_rows, 32), dtype=np.uint8)
        self.verdict0 = np.full(self.plan.voff[-1] + 2 * GUARD, UNWRITTEN, dtype=np.uint32)
        self.want_verdict = self.verdict0.copy()
        self.wrong = {}                                    # (session, slot) -> how its stated root is wrong
        for k, (n, nl) in enumerate(ss):
            true_roots = np.zeros((nl, 32), dtype=np.uint8)
            for s in range(nl):
                leaves = np.zeros((n, 32), dtype=np.uint8)
                leaves[:, :31] = rng.integers(0, 256, size=(n, 31), dtype=np.uint8)
                if oracle is None:
                    continue
                layers = oracle.merkle_tree(leaves)
                assert [len(x) for x in layers] == M.layer_sizes(n)
                for level, layer in enumerate(layers):
                    r = self.first[k] + M.row_of(n, nl, level, s, 0)
                    (self.image if level == 0 else self.want)[r:r + len(layer)] = layer
                    if level == 0:
                        self.want[r:r + len(layer)] = layer
                true_roots[s] = layers[-1][0]
            stated = true_roots.copy()
            s = 0
            while s < nl:
                kind = rng.integers(0, 12)                 # 0, 1, 2: wrong; a swap makes two wrong at once
                if kind == 0:
                    stated[s, 0] ^= 1
                    self.wrong[(k, s)] = "low byte"
                elif kind == 1:
                    stated[s, 28] ^= 1
                    self.wrong[(k, s)] = "top limb"
                elif kind == 2 and s + 1 < nl:
                    stated[[s, s + 1]] = stated[[s + 1, s]]
                    self.wrong[(k, s)] = self.wrong[(k, s + 1)] = "swapped"
                    s += 1
                s += 1
            self.roots[self.root_first[k]:self.root_first[k] + nl] = stated
            for s in range(nl):
                self.want_verdict[GUARD + self.plan.voff[k] + s] = int((k, s) in self.wrong)


def launch(torch, lib, lay, shift=None, null=None, cnt_zero=False, n_rows_less=None):
    """the launch of a case; shift / null: the name of one table passed misaligned / as NULL.  Returns (status, rows, roots, verdicts)"""
    d_rows, d_roots, d_verdict = up(torch, lay.image), up(torch, lay.roots), up(torch, lay.verdict0)
    addrs = [d_rows.data_ptr() + 32 * f for f in lay.first]
    roots = [d_roots.data_ptr() + 32 * f for f in lay.root_first]
    tab, voff, prefix, sess_of, off, cnt, work = M.tables(lay.plan, addrs, roots)
    if n_rows_less is not None:
        tab = tab.copy()
        tab[7 * n_rows_less + 1] -= 1
    if cnt_zero:
        cnt = cnt.copy()
        cnt[0] = 0
    dev = {"sessions": up(torch, tab), "voff": up(torch, voff), "prefix": up(torch, prefix), "sess_of": up(torch, sess_of)}
    ptr = {k: v.data_ptr() for k, v in dev.items()}
    ptr["verdict"] = d_verdict.data_ptr() + 4 * GUARD
    if shift:
        ptr[shift] += 2 if shift in ("sess_of", "verdict") else 4
    if null:
        ptr[null] = None
    st = lib.ffm_finish_layers_many(ptr["sessions"], len(lay.sessions), ptr["voff"], ptr["prefix"], ptr["sess_of"], hp(off), hp(cnt), hp(work), len(off),
                                    ptr["verdict"])
    torch.cuda.synchronize()
    return st, d_rows.cpu().numpy().reshape(-1, 32), d_roots.cpu().numpy().reshape(-1, 32), d_verdict.cpu().numpy().view(np.uint32)


def test_sessions_against_the_oracle_with_guard_rows(ffm, torch_, oracle, capsys):
    c_oracle, _ = oracle
    bad, cs = [], M.cases()
    for c in cs:
        lay = Layout(c, c_oracle)
        st, got, roots, verdict = launch(torch_, ffm, lay)
        what = "case %d (%d sessions, %d rows, %d slots, %d stated roots wrong)" % (c.no, len(c.sessions), lay.rows, lay.plan.voff[-1], len(lay.wrong))
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
        print("\n[fill finish many unit] %d cases checked, 0 skipped, %d failed" % (len(cs), len(bad)))
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad))


def test_a_row_beyond_n_rows_is_not_stored_and_ends_in_verdict_one(ffm, torch_, oracle):
    """the kernel's guard: a descriptor whose n_rows is one short leaves the last slot's root row alone and reports a mismatch"""
    c_oracle, _ = oracle
    lay = Layout(M.Case(97, [(1, 1), (5, 2), (3, 1)]), c_oracle)
    st, got, roots, verdict = launch(torch_, ffm, lay, n_rows_less=1)
    last = lay.first[1] + M.rows(5, 2) - 1
    want, want_verdict = lay.want.copy(), lay.want_verdict.copy()
    want[last] = lay.image[last]
    want_verdict[GUARD + lay.plan.voff[1] + 1] = 1
    assert st == 0 and np.array_equal(got, want) and np.array_equal(verdict, want_verdict) and np.array_equal(roots, lay.roots)


def test_refusals_and_no_work(ffm, torch_, oracle):
    c_oracle, _ = oracle
    lay = Layout(M.Case(99, [(1, 1), (5, 2), (2, 3), (1, 1)]), c_oracle)

    def untouched(st, got, roots, verdict):
        return st == HIP_INVALID and np.array_equal(got, lay.image) and np.array_equal(roots, lay.roots) and np.array_equal(verdict, lay.verdict0)

    for name in ("sessions", "voff", "prefix", "sess_of", "verdict"):
        assert untouched(*launch(torch_, ffm, lay, null=name)), "NULL " + name          # a NULL table with work to do
        assert untouched(*launch(torch_, ffm, lay, shift=name)), "misaligned " + name   # each table misaligned
    assert untouched(*launch(torch_, ffm, lay, cnt_zero=True))                         # a level with work and no entries
    f = ffm.ffm_finish_layers_many
    zero = np.zeros(3, dtype=np.uint64)
    assert f(None, 0, None, None, None, None, None, None, 0, None) == 0                 # no levels: no work
    assert f(None, 0, None, None, None, hp(zero), hp(zero), hp(zero), 3, None) == 0     # levels without lanes: no work
    assert f(None, 0, None, None, None, None, None, None, 2, None) == HIP_INVALID       # levels without their host tables
    st, got, roots, verdict = launch(torch_, ffm, lay)                                  # and the same arguments, valid
    assert st == 0 and np.array_equal(got, lay.want) and np.array_equal(verdict, lay.want_verdict)
