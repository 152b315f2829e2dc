"""GPU suite: k_nodes_restore_layer through its launchers alone (tests/device_check/libfill_node_ckpt_unit.so, forwarders linked against the
product).  The session's buffer, the candidate buffer and the flag bytes are torch tensors between guard bytes, pre-filled with a non-zero
pattern; the oracle's authentic nodes stand in exactly the rows a case calls known or restored.

Single layers through launch_nodes_restore_layer, children of m_in = 1 (the single child, as the bottom layer and above it), 2, 3 (an odd
layer: only the launcher reaches it, the sessions' trees are powers of two), 8 and 514 (257 parents: past one workgroup) per slot, over 1
and 3 slots.  The parents cycle through every combination of

  parent   known, restored, or neither (undefined, a candidate, rejected)
  left     KNOWN, CAND, undefined
  right    KNOWN, CAND, undefined -- or absent, for the last node of an odd layer and the single child
  values   matching, or one child's value damaged

so that each of the 54 stands under some parent of every shape (small layers are launched again with the cycle shifted).  The model
(tests/fill_node_ckpt_models.py) runs on the same rows with the oracle's compression.  Every comparison is bit exact and covers the guards:
no row and no flag byte outside the CAND children of a matching parent may change, and the candidate buffer never."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

import fill_node_ckpt_models as N2
import fill_nodes_models as M
import kernel_models as K
from test_gpu_kernel_units import FRONT, PATTERN, Out, as_int, canonical_rows, flip, up

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libfill_node_ckpt_unit.so")
PARENTS = ("known", "restored", "undef", "cand", "rejected")
CHILD = ("known", "cand", "undef")
COMBOS = [(p, l, r, ok) for p in range(3) for l in range(3) for r in range(3) for ok in (True, False)]      # 54
FLAG = {"known": N2.KNOWN, "cand": N2.CAND, "undef": 0, "restored": N2.RESTORED, "rejected": N2.REJECTED}


@pytest.fixture(scope="module")
def fnc(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/" + os.path.basename(LIB)],
                              stdout=subprocess.DEVNULL)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib = ctypes.CDLL(LIB)
    lib.fnc_restore_layer.restype, lib.fnc_restore_layer.argtypes = i32, [vp, vp, vp, vp, u64, u64, u64, u64, i32, i32, u64]
    lib.fnc_restore_layers.restype, lib.fnc_restore_layers.argtypes = i32, [vp, vp, vp, vp, vp, vp, u32, u64, u64]
    return lib


def body(n):
    return np.resize(PATTERN, FRONT + n)[FRONT:].copy()          # what Out pre-fills its body with


def plus_r(row):
    return np.frombuffer((as_int(row) + K.R_MOD).to_bytes(32, "little"), dtype=np.uint8)          # below 2^256: the value is below r


def device(torch, t0, c0, f0):
    tree, cand, flags = Out(torch, t0.size), Out(torch, c0.size), Out(torch, f0.size)
    for o, a in ((tree, t0), (cand, c0), (flags, f0)):
        o.t[o.lo:o.lo + o.n] = torch.from_numpy(a.reshape(-1).copy()).cuda()
    return tree, cand, flags


class Layer:
    """children of m_in rows per slot, their parents, and the states one shift of the cycle gives every row"""

    def __init__(self, C, m_in, n_local, bottom, top):
        rng = np.random.default_rng([0x2C47, m_in, n_local, bottom, top])
        self.C, self.m_in, self.n_local, self.bottom, self.top = C, m_in, n_local, bottom, top
        self.m_out = (m_in + 1) // 2
        self.off_out = n_local * m_in
        self.n_rows = self.off_out + n_local * self.m_out
        self.truth = np.zeros((self.n_rows, 32), np.uint8)
        self.truth[:self.off_out] = canonical_rows(rng, self.off_out)
        zero = np.zeros(32, np.uint8)
        for s in range(n_local):
            for j in range(self.m_out):
                rl = s * m_in + 2 * j
                pair = 2 * j + 1 < m_in
                self.truth[self.off_out + s * self.m_out + j] = C.compress(self.truth[rl], self.truth[rl + 1] if pair else zero,
                                                                           (1 if bottom else 0) + (0 if pair else 2))
        self.roots = np.stack([self.truth[self.off_out + s * self.m_out] for s in range(n_local)])    # what a top launch judges against

    def start(self, shift):
        t0, c0 = body(self.n_rows * 32).reshape(-1, 32), body(self.n_rows * 32).reshape(-1, 32)
        f0 = np.zeros(self.n_rows, np.uint8)
        seen = set()
        for s in range(self.n_local):
            for j in range(self.m_out):
                i = s * self.m_out + j
                p, l, r, ok = COMBOS[(i + shift) % len(COMBOS)]
                parent = PARENTS[p] if p < 2 else PARENTS[2 + (i // len(COMBOS) + shift) % 3]
                rp, rl = self.off_out + i, s * self.m_in + 2 * j
                pair = 2 * j + 1 < self.m_in
                f0[rp] = N2.KNOWN if self.top and parent == "known" else FLAG[parent]
                if parent in ("known", "restored") and not self.top:
                    t0[rp] = self.truth[rp]                                   # (a top launch reads slot_roots: the row keeps the pattern)
                kids = [(rl, CHILD[l])] + ([(rl + 1, CHILD[r])] if pair else [])
                for row, st in kids:
                    f0[row] = FLAG[st]
                    if st == "known":
                        t0[row] = self.truth[row]
                    elif st == "cand":
                        c0[row] = self.truth[row]
                if not ok:                                                    # one child's value damaged: a candidate where there is one
                    cands = [row for row, st in kids if st == "cand"]
                    row = cands[i % len(cands)] if cands else kids[i % len(kids)][0]
                    flip(c0 if cands else t0, row, (i * 13 + 5) % 250)
                seen.add((min(p, 2), CHILD[l], CHILD[r] if pair else "absent", ok))
        return t0, c0, f0, seen

    def model(self, t0, c0, f0, n_rows=None):
        tree, flags = list(t0), [int(x) for x in f0]
        N2.restore_layer(tree, list(c0), flags, list(self.roots), 0, self.m_in, self.off_out, self.n_local, self.bottom, self.top,
                         self.n_rows if n_rows is None else n_rows, lambda x, y, key: self.C.compress(x, y, key), np.zeros(32, np.uint8))
        return np.stack(tree), np.array(flags, np.uint8)

    def launch(self, fnc, torch, tree, cand, flags, n_rows=None):
        d_roots = up(torch, self.roots)
        st = fnc.fnc_restore_layer(tree.ptr, cand.ptr, flags.ptr, d_roots.data_ptr(), 0, self.m_in, self.off_out, self.n_local, int(self.bottom),
                                   int(self.top), self.n_rows if n_rows is None else n_rows)
        torch.cuda.synchronize()
        return st


# (m_in, bottom, top): the single child at the bottom (the one-block slot, judged against the stated root) and above it; a top layer of two
LAYERS = [(1, True, True), (1, False, False), (1, True, False), (2, True, True), (2, False, True), (2, False, False), (3, True, False), (3, False, False),
          (8, True, False), (8, False, False), (514, True, False), (514, False, False)]


def test_single_layers_agree_with_the_model_in_every_combination(fnc, oracle, capsys):
    import torch
    C, _ = oracle
    t_start, bad, lanes, launches = time.time(), [], 0, 0
    tally = dict(restored=0, rejected=0, left_alone=0)
    for m_in, bottom, top in LAYERS:
        for n_local in (1, 3):
            lay = Layer(C, m_in, n_local, bottom, top)
            parents = lay.m_out * n_local
            seen = set()
            for shift in range(len(COMBOS) if parents < 2 * len(COMBOS) else 1):      # a small layer again and again, the cycle one further
                what = "m_in=%d n_local=%d bottom=%d top=%d shift=%d" % (m_in, n_local, bottom, top, shift)
                t0, c0, f0, s = lay.start(shift)
                seen |= s
                tree, cand, flags = device(torch, t0, c0, f0)
                if lay.launch(fnc, torch, tree, cand, flags) != 0:
                    bad.append(what + ": the launcher refused")
                    continue
                m_tree, m_flags = lay.model(t0, c0, f0)
                tree.check(m_tree, what + " tree", bad, 32)
                flags.check(m_flags, what + " flags", bad, 1)
                cand.check(c0, what + " candidates", bad, 32)
                lanes += parents
                launches += 1
                tally["restored"] += int((m_flags == N2.RESTORED).sum() - (f0 == N2.RESTORED).sum())
                tally["rejected"] += int((m_flags == N2.REJECTED).sum() - (f0 == N2.REJECTED).sum())
                tally["left_alone"] += int(((m_flags == N2.CAND) & (f0 == N2.CAND)).sum())
                # canaries, stated directly: only CAND children changed, and their rows only where they were restored
                changed = np.nonzero((m_tree != t0).any(axis=1))[0]
                assert all(f0[r] == N2.CAND and m_flags[r] == N2.RESTORED and r < lay.off_out for r in changed), what
                assert all(f0[r] == N2.CAND for r in np.nonzero(m_flags != f0)[0]), what
            want = {(p, l, r, ok) for p in range(3) for l in CHILD for r in CHILD for ok in (True, False)}
            if m_in == 1:
                want = {(p, l, "absent", ok) for p in range(3) for l in CHILD for ok in (True, False)}
            elif m_in % 2:
                want |= {(p, l, "absent", ok) for p in range(3) for l in CHILD for ok in (True, False)}
            assert want <= seen, ("combinations never met", m_in, n_local, sorted(want - seen))
    with capsys.disabled():
        print("\n[fill node ckpt unit] %d lanes in %d launches over %d layer shapes: %s, %d failed, %.1f s" % (lanes, launches, 2 * len(LAYERS), tally, len(bad),
                                                                                                         time.time() - t_start))
    assert all(tally[k] > 0 for k in tally), tally
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:100]))


def test_rows_at_or_past_n_rows_are_not_touched(fnc, oracle):
    import torch
    C, _ = oracle
    lay = Layer(C, 8, 3, True, False)
    t0, c0, f0, _ = lay.start(0)
    for n_rows in (lay.off_out + 5, lay.off_out, 11):                            # some parents, every parent, and some children past the end
        tree, cand, flags = device(torch, t0, c0, f0)
        assert lay.launch(fnc, torch, tree, cand, flags, n_rows=n_rows) == 0
        m_tree, m_flags = lay.model(t0, c0, f0, n_rows=n_rows)
        bad = []
        tree.check(m_tree, "tree", bad, 32)
        flags.check(m_flags, "flags", bad, 1)
        cand.check(c0, "cand", bad, 32)
        assert not bad, (n_rows, bad)
        assert np.array_equal(m_flags[n_rows:], f0[n_rows:]) and np.array_equal(m_tree[n_rows:], t0[n_rows:])
        if n_rows <= lay.off_out:
            assert np.array_equal(m_flags, f0) and np.array_equal(m_tree, t0)       # no parent below n_rows: nothing at all


class Chain:
    """whole trees of n_blocks over n_local slots: nothing known but the top rows, every row below a candidate"""

    def __init__(self, C, n_blocks, n_local):
        rng = np.random.default_rng([0x2C48, n_blocks, n_local])
        self.C, self.n_blocks, self.n_local = C, n_blocks, n_local
        self.sizes, self.offs, self.n_rows = M.layout(n_blocks, n_local)
        self.depth = len(self.sizes) - 1
        trees = [C.merkle_tree(canonical_rows(rng, n_blocks)) for _ in range(n_local)]
        self.truth = np.zeros((self.n_rows, 32), np.uint8)
        for s in range(n_local):
            for lvl in range(self.depth + 1):
                for k in range(self.sizes[lvl]):
                    self.truth[self.row(lvl, s, k)] = trees[s][lvl][k]
        self.roots = np.stack([t[-1][0] for t in trees])

    def row(self, lvl, s, k):
        return self.offs[lvl] + s * self.sizes[lvl] + k

    def run(self, fnc, torch, c0, f0, roots=None):
        t0 = body(self.n_rows * 32).reshape(-1, 32)
        tree, cand, flags = device(torch, t0, c0, f0)
        offs, sizes = np.array(self.offs, dtype=np.uint64), np.array(self.sizes, dtype=np.uint64)
        d_roots = up(torch, self.roots if roots is None else roots)
        st = fnc.fnc_restore_layers(tree.ptr, cand.ptr, flags.ptr, d_roots.data_ptr(), offs.ctypes.data, sizes.ctypes.data, self.depth, self.n_local,
                                    self.n_rows)
        torch.cuda.synchronize()
        assert st == 0
        return t0, tree, cand, flags


@pytest.mark.parametrize("n_blocks", [8, 64])
def test_a_whole_chain_is_restored_from_the_stated_roots_and_a_forged_node_stops_it(fnc, oracle, n_blocks):
    import torch
    C, _ = oracle
    ch = Chain(C, n_blocks, 3)
    assert ch.depth == {8: 3, 64: 6}[n_blocks]
    top = ch.offs[ch.depth]
    c0 = body(ch.n_rows * 32).reshape(-1, 32)
    c0[:top] = ch.truth[:top]
    f0 = np.full(ch.n_rows, N2.CAND, np.uint8)
    f0[top:] = N2.KNOWN
    # slot 1: a forged node two layers under the top; slot 2: a leaf stated as value + r, and the root stated as root + r
    forged = ch.row(ch.depth - 2, 1, 1)
    flip(c0, forged, 77)
    c0[ch.row(0, 2, 3)] = plus_r(ch.truth[ch.row(0, 2, 3)])
    roots = ch.roots.copy()
    roots[2] = plus_r(roots[2])
    t0, tree, cand, flags = ch.run(fnc, torch, c0, f0, roots)
    compress = lambda x, y, key: C.compress(x, y, key)     # noqa: E731
    canon = c0.copy()
    canon[ch.row(0, 2, 3)] = ch.truth[ch.row(0, 2, 3)]      # the model compares and copies canonical values
    m_tree, m_flags = N2.restore(n_blocks, 3, list(t0), list(canon), [int(x) for x in f0], list(ch.roots), compress, np.zeros(32, np.uint8))
    bad = []
    tree.check(np.stack(m_tree), "tree", bad, 32)
    flags.check(np.array(m_flags, np.uint8), "flags", bad, 1)
    cand.check(c0, "cand", bad, 32)
    assert not bad, bad
    got_f, got_t = flags.fetch(), tree.fetch().reshape(-1, 32)
    for s in (0, 2):                                        # chains of every length from 1 to depth
        for lvl in range(ch.depth):
            for k in range(ch.sizes[lvl]):
                r = ch.row(lvl, s, k)
                assert got_f[r] == N2.RESTORED and np.array_equal(got_t[r], ch.truth[r]), (s, lvl, k)
    # the forged node and its sibling candidate are rejected, nothing below either is reached, everything else of the slot is restored
    under = {ch.row(lvl, 1, k) for lvl in range(ch.depth - 2) for k in range(ch.sizes[lvl]) if (k >> (ch.depth - 2 - lvl)) in (0, 1)}
    for lvl in range(ch.depth):
        for k in range(ch.sizes[lvl]):
            r = ch.row(lvl, 1, k)
            want = N2.REJECTED if r in (forged, forged - 1) else N2.CAND if r in under else N2.RESTORED
            assert got_f[r] == want, (lvl, k, got_f[r], want)
            assert np.array_equal(got_t[r], ch.truth[r] if want == N2.RESTORED else t0[r])
    assert np.array_equal(got_t[top:], t0[top:])            # the top rows are judged against slot_roots and never written


def test_no_work_and_refusals(fnc, oracle):
    import torch
    C, _ = oracle
    ch = Chain(C, 2, 1)
    c0 = body(ch.n_rows * 32).reshape(-1, 32)
    f0 = np.array([N2.CAND, N2.CAND, N2.KNOWN], np.uint8)
    t0 = body(ch.n_rows * 32).reshape(-1, 32)
    tree, cand, flags = device(torch, t0, c0, f0)
    offs, sizes = np.array(ch.offs, dtype=np.uint64), np.array(ch.sizes, dtype=np.uint64)
    d_roots = up(torch, ch.roots)
    one = lambda **kw: fnc.fnc_restore_layer(*[kw.get(k, v) for k, v in (("tree", tree.ptr), ("cand", cand.ptr), ("flags", flags.ptr), ("roots", d_roots.data_ptr()),   # noqa: E731
                                                                         ("off_in", 0), ("m_in", 2), ("off_out", 2), ("n_local", 1), ("bottom", 1), ("top", 1),
                                                                         ("n_rows", ch.n_rows))])
    all_ = lambda **kw: fnc.fnc_restore_layers(*[kw.get(k, v) for k, v in (("tree", tree.ptr), ("cand", cand.ptr), ("flags", flags.ptr), ("roots", d_roots.data_ptr()),   # noqa: E731
                                                                           ("offs", offs.ctypes.data), ("sizes", sizes.ctypes.data), ("depth", ch.depth),
                                                                           ("n_local", 1), ("n_rows", ch.n_rows))])
    assert one(n_local=0) == 0 and all_(n_local=0) == 0                                     # n == 0 launches no work
    for hole in ("tree", "cand", "flags", "roots"):
        assert one(**{hole: None}) == 1 and all_(**{hole: None}) == 1, hole                 # hipErrorInvalidValue
    assert all_(offs=None) == 1 and all_(sizes=None) == 1 and all_(depth=0) == 1 and one(m_in=0) == 1
    wrong = sizes.copy()
    wrong[1] = 2
    assert all_(sizes=wrong.ctypes.data) == 1                                              # tables that are not a compact layout
    wrong = offs.copy()
    wrong[1] = 3
    assert all_(offs=wrong.ctypes.data) == 1
    torch.cuda.synchronize()
    for o, a in ((tree, t0), (cand, c0), (flags, f0)):
        assert np.array_equal(o.fetch(), a.reshape(-1)) and o.guards_ok()
