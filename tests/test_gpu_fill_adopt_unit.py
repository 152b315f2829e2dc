"""GPU suite: k_adopt_layer and k_adopt_resolve through their launchers alone (tests/device_check/libfill_adopt_unit.so, forwarders linked
against the product).  The session's buffer, the candidate buffer, the flag bytes and the verdict bytes are torch tensors between guard
bytes, pre-filled with a non-zero pattern; the oracle's authentic nodes stand in exactly the rows a case calls known.  Trees of 1, 2, 5
(odd layers), 8 and 64 blocks over 1 and 3 local slots.  With three slots:

  slot 0   a seeded mix of states, NOT selected in the first pass: every byte of it must stay as it was;
  slot 1   nothing known, every block a true candidate, the root stated as root + r: the whole slot is proved from the stated root, chains
           of every length from 1 to depth;
  slot 2   a seeded mix: rows below the top known with probability 0.35, the leaves cycling through undefined / true candidate / damaged
           candidate / known / known with a true candidate / known with a damaged candidate, so that every pair of child states (known,
           candidate, undefined on each side) stands under some parent, known parents match and mismatch, chains break at undefined rows and
           end at known nodes that do not match.

The models (tests/fill_adopt_models.py) run on the same rows with the oracle's compression.  Every comparison is bit exact and covers the
guards; the known rows of the session's buffer, its top rows and everything of an unselected slot must be bit-identical afterwards."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

import fill_adopt_models as D
import fill_nodes_models as M
import kernel_models as K
from test_gpu_kernel_units import FRONT, PATTERN, Out, as_int, canonical_rows, flip, up

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libfill_adopt_unit.so")
UNDEF, TRUE, BAD, KNOWN, KNOWN_TRUE, KNOWN_BAD = range(6)


@pytest.fixture(scope="module")
def fad(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/" + os.path.basename(LIB)],
                              stdout=subprocess.DEVNULL)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib = ctypes.CDLL(LIB)
    lib.fad_adopt_layers.restype, lib.fad_adopt_layers.argtypes = i32, [vp, vp, vp, vp, vp, vp, u32, u64, u64, u64, u64]
    lib.fad_adopt_resolve.restype, lib.fad_adopt_resolve.argtypes = i32, [vp, vp, vp, vp, vp, vp, u32, u64, u64, u64, u64, u64]
    return lib


def plus_r(row):
    return np.frombuffer((as_int(row) + K.R_MOD).to_bytes(32, "little"), dtype=np.uint8)          # below 2^256: the value is below r


class Plan:
    """The trees, the states of every row and the candidates of one (n_blocks, n_local)."""

    def __init__(self, C, n_blocks, n_local):
        rng = np.random.default_rng([0xAD07, n_blocks, n_local])
        self.C, self.n_blocks, self.n_local = C, n_blocks, n_local
        self.sizes, self.offs, self.n_rows = M.layout(n_blocks, n_local)
        self.depth = len(self.sizes) - 1
        self.trees = [C.merkle_tree(canonical_rows(rng, n_blocks)) for _ in range(n_local)]
        assert [len(x) for x in self.trees[0]] == self.sizes
        self.roots = np.stack([t[-1][0] for t in self.trees])
        self.known, self.leaf = set(), {}
        for s in range(n_local):
            whole = n_local == 3 and s == 1
            if whole:
                self.roots[s] = plus_r(self.roots[s])
            for b in range(n_blocks):
                self.leaf[(s, b)] = TRUE if whole else (b + 3 * (b // 6) + s) % 6
                if self.leaf[(s, b)] >= KNOWN:
                    self.known.add(self.row(0, s, b))
            if not whole:
                for lvl in range(1, self.depth):
                    for k in range(self.sizes[lvl]):
                        if rng.random() < 0.35:
                            self.known.add(self.row(lvl, s, k))
        self.truth = [None] * self.n_rows
        for s in range(n_local):
            for lvl in range(self.depth + 1):
                for k in range(self.sizes[lvl]):
                    self.truth[self.row(lvl, s, k)] = self.trees[s][lvl][k]

    def row(self, lvl, s, k):
        return self.offs[lvl] + s * self.sizes[lvl] + k

    def host_start(self, slots):
        """the host images of the session's buffer, the candidate buffer and the flag bytes for the selected slots"""
        body = lambda n: np.resize(PATTERN, FRONT + n)[FRONT:].copy()    # noqa: E731  (what Out pre-fills its body with)
        t0, c0 = body(self.n_rows * 32).reshape(self.n_rows, 32), body(self.n_rows * 32).reshape(self.n_rows, 32)
        f0 = np.zeros(self.n_rows, np.uint8)
        for r in self.known:
            t0[r] = self.truth[r]
            f0[r] = D.KNOWN
        for s in range(self.n_local):
            f0[self.row(self.depth, s, 0)] |= D.KNOWN                              # the top rows: the stated roots; the rows keep the pattern
            for b in range(self.n_blocks):
                st, r = self.leaf[(s, b)], self.row(0, s, b)
                if st in (TRUE, BAD, KNOWN_TRUE, KNOWN_BAD):
                    c0[r] = self.truth[r]
                    if st in (BAD, KNOWN_BAD):
                        flip(c0, r, (b * 11 + s * 5 + 3) % 248)
                    if s in slots:
                        f0[r] |= D.CAND
        return t0, c0, f0

    def start(self, torch, slots):
        """(tree, cand, flags, out) on the device with their host images"""
        tree, cand, flags, out = Out(torch, self.n_rows * 32), Out(torch, self.n_rows * 32), Out(torch, self.n_rows), Out(torch, self.n_rows)
        t0, c0, f0 = self.host_start(slots)
        for o, a in ((tree, t0), (cand, c0), (flags, f0)):
            o.t[o.lo:o.lo + o.n] = torch.from_numpy(a.reshape(-1).copy()).cuda()
        return tree, cand, flags, out, t0, c0, f0

    def model(self, slots, t0, c0, f0):
        compress = lambda x, y, key: self.C.compress(x, y, key)    # noqa: E731
        cand, flags = D.layers(self.n_blocks, self.n_local, slots, list(t0), list(c0), [int(x) for x in f0], list(self.roots), compress, np.zeros(32, np.uint8))
        # the stated root + r compares as the root: the model compares canonical values
        for s in slots:
            top = self.row(self.depth, s, 0)
            if flags[top] & D.CAND and np.array_equal(cand[top], self.trees[s][-1][0]):
                flags[top] |= D.MATCH
        out, tree = D.resolve(self.n_blocks, self.n_local, slots, list(t0), cand, flags)
        return np.stack(cand), np.array(flags, np.uint8), np.array(out, np.uint8), np.stack(tree)


@pytest.fixture(scope="module")
def plans(oracle):
    C, _ = oracle
    return {(nb, nl): Plan(C, nb, nl) for nb in D.ADOPT_N_BLOCKS for nl in (1, 3)}


def run(fad, torch, p, slots, n_rows=None):
    first, n_sel = slots[0], len(slots)
    tree, cand, flags, out, t0, c0, f0 = p.start(torch, slots)
    offs, sizes = np.array(p.offs, dtype=np.uint64), np.array(p.sizes, dtype=np.uint64)
    d_offs, d_sizes, d_roots = up(torch, offs), up(torch, sizes), up(torch, p.roots)
    n_rows = p.n_rows if n_rows is None else n_rows
    st = fad.fad_adopt_layers(tree.ptr, cand.ptr, flags.ptr, d_roots.data_ptr(), offs.ctypes.data, sizes.ctypes.data, p.depth, p.n_local, first, n_sel, n_rows)
    torch.cuda.synchronize()
    mid = (tree.fetch().copy(), cand.fetch().copy(), flags.fetch().copy())
    st2 = fad.fad_adopt_resolve(tree.ptr, cand.ptr, flags.ptr, out.ptr, d_offs.data_ptr(), d_sizes.data_ptr(), p.depth, p.n_local, first, n_sel,
                                p.offs[p.depth], n_rows)
    torch.cuda.synchronize()
    return (st, st2), (tree, cand, flags, out), (t0, c0, f0), mid


def test_layers_and_resolve_agree_with_the_models(fad, plans, capsys):
    import torch
    t_start, bad, cases = time.time(), [], 0
    combos, steps_seen, tally = set(), set(), dict(match=0, mismatch=0, broken=0, unmatched_end=0, single=0, leaf_equal=0, leaf_differs=0, proved=0, adopted=0)
    for (nb, nl), p in plans.items():
        for slots in ([0],) if nl == 1 else ([1, 2], [0, 1, 2], [2]):
            what = "adopt n_blocks=%d n_local=%d slots=%s" % (nb, nl, slots)
            (st, st2), (tree, cand, flags, out), (t0, c0, f0), mid = run(fad, torch, p, slots)
            if st != 0 or st2 != 0:
                bad.append("%s: status %d, %d" % (what, st, st2))
                continue
            m_cand, m_flags, m_out, m_tree = p.model(slots, t0, c0, f0)
            cases += sum(p.sizes[1:]) * len(slots) + p.offs[p.depth]
            # after the layer launches: the tree untouched, the computed rows and their flag bytes as the model has them
            if not np.array_equal(mid[0], t0.reshape(-1)):
                bad.append("%s: k_adopt_layer wrote the session's buffer" % what)
            want_c = c0.copy()
            for r in range(p.offs[1], p.n_rows):
                if m_flags[r] & D.CAND:
                    want_c[r] = m_cand[r]
            if not np.array_equal(mid[1], want_c.reshape(-1)):
                r = int(np.nonzero(mid[1].reshape(-1, 32) != want_c)[0][0])
                bad.append("%s: candidate row %d differs after the layers" % (what, r))
            if not np.array_equal(mid[2], m_flags):
                r = int(np.nonzero(mid[2] != m_flags)[0][0])
                bad.append("%s: flag byte of row %d is %d after the layers, expected %d" % (what, r, mid[2][r], m_flags[r]))
            # after the resolve: the proved rows copied, every known row, every top row and every unselected slot bit-identical
            tree.check(m_tree, what + " tree", bad, 32)
            want_out = out.prefill().copy()
            for lvl in range(p.depth):
                for s in slots:
                    for k in range(p.sizes[lvl]):
                        want_out[p.row(lvl, s, k)] = m_out[p.row(lvl, s, k)]
            out.check(want_out, what + " verdict bytes", bad, 1)
            cand.check(want_c, what + " candidates after the resolve", bad, 32)
            flags.check(m_flags, what + " flags after the resolve", bad, 1)
            got_tree = tree.fetch().reshape(p.n_rows, 32)
            for r in range(p.n_rows):
                top_or_known = r >= p.offs[p.depth] or r in p.known
                if top_or_known and not np.array_equal(got_tree[r], t0[r]):
                    bad.append("%s: row %d (known or top) changed" % (what, r))
                if m_out[r] & D.PROVED and not np.array_equal(got_tree[r], p.truth[r]):
                    bad.append("%s: proved row %d is not the true node" % (what, r))
            # what the plan really held
            state = lambda f: "known" if f & D.KNOWN else "cand" if f & D.CAND else "undef"    # noqa: E731
            for lvl in range(p.depth):
                for s in slots:
                    for j in range(p.sizes[lvl + 1]):
                        rl, rp = p.row(lvl, s, 2 * j), p.row(lvl + 1, s, j)
                        if 2 * j + 1 < p.sizes[lvl]:
                            combos.add((state(m_flags[rl]), state(m_flags[rl + 1])))
                        else:
                            tally["single"] += 1
                        if m_flags[rp] & D.KNOWN and m_flags[rp] & D.CAND:
                            tally["match" if m_flags[rp] & D.MATCH else "mismatch"] += 1
                    for k in range(p.sizes[lvl]):
                        r = p.row(lvl, s, k)
                        f = int(m_out[r])
                        tally["proved"] += bool(f & D.PROVED)
                        tally["adopted"] += bool(f & D.ADOPTED)
                        if lvl == 0 and f & D.KNOWN and f & D.CAND:
                            tally["leaf_equal" if f & D.MATCH else "leaf_differs"] += 1
                        if f & D.CAND and not f & D.KNOWN:
                            idx, n = k, 0
                            for upl in range(lvl + 1, p.depth + 1):
                                idx >>= 1
                                n += 1
                                fa = int(m_flags[p.row(upl, s, idx)])
                                if not fa & D.CAND:
                                    tally["broken"] += 1
                                    break
                                if fa & D.KNOWN:
                                    if fa & D.MATCH:
                                        steps_seen.add((nb, n))
                                    else:
                                        tally["unmatched_end"] += 1
                                    break
    with capsys.disabled():
        print("\n[fill adopt unit] %d lanes over %d plans: %s, child pairs %d of 9, %d failed, %.1f s" % (cases, len(plans), tally, len(combos), len(bad),
                                                                                                        time.time() - t_start))
    assert len(combos) == 9, combos                                                        # known / candidate / undefined on each side
    assert all(tally[k] > 0 for k in tally), tally
    assert {n for nb, n in steps_seen if nb == 64} == set(range(1, 7))                     # chains of every length up to depth
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:100]))


def test_the_key_at_layer_0_differs_from_the_key_above(fad, plans, oracle):
    """the same two children under the bottom key and under the upper key give different parents: slot 1 of the 8-block plan against a
    one-layer-up restatement with the oracle"""
    C, _ = oracle
    p = plans[(8, 3)]
    a, b = p.trees[1][0][0], p.trees[1][0][1]
    assert not np.array_equal(C.compress(a, b, 1), C.compress(a, b, 0))
    assert np.array_equal(C.compress(a, b, 1), p.trees[1][1][0])
    a, b = p.trees[1][1][0], p.trees[1][1][1]
    assert np.array_equal(C.compress(a, b, 0), p.trees[1][2][0])
    one = plans[(1, 1)]
    assert np.array_equal(C.compress(one.trees[0][0][0], np.zeros(32, np.uint8), 3), one.trees[0][1][0])   # the singleton: key + 2, zero sibling


def test_rows_at_or_past_n_rows_are_not_touched(fad, plans):
    import torch
    p = plans[(8, 3)]
    short = p.offs[p.depth]                                                               # the top rows lie past n_rows
    (st, st2), (tree, cand, flags, out), (t0, c0, f0), mid = run(fad, torch, p, [0, 1, 2], n_rows=short)
    assert st == 0 and st2 == 0
    got_c, got_f, got_t, got_o = (x.fetch().copy() for x in (cand, flags, tree, out))
    assert all(x.guards_ok() for x in (cand, flags, tree, out))
    assert np.array_equal(got_c.reshape(-1, 32)[short:], c0[short:]) and np.array_equal(got_f[short:], f0[short:])
    assert np.array_equal(got_t.reshape(-1, 32)[short:], t0[short:]) and np.array_equal(got_o[short:], out.prefill()[short:])
    # without its top row slot 1 has nothing that vouches for it: no row of it is proved
    for lvl in range(p.depth):
        for k in range(p.sizes[lvl]):
            assert not got_o[p.row(lvl, 1, k)] & D.PROVED


def test_no_work_and_refusals(fad, plans):
    import torch
    p = plans[(2, 1)]
    tree, cand, flags, out, t0, c0, f0 = p.start(torch, [0])
    offs, sizes = np.array(p.offs, dtype=np.uint64), np.array(p.sizes, dtype=np.uint64)
    d_offs, d_sizes, d_roots = up(torch, offs), up(torch, sizes), up(torch, p.roots)
    lay = lambda **kw: fad.fad_adopt_layers(*[kw.get(k, v) for k, v in (("tree", tree.ptr), ("cand", cand.ptr), ("flags", flags.ptr), ("roots", d_roots.data_ptr()),   # noqa: E731
                                                                         ("offs", offs.ctypes.data), ("sizes", sizes.ctypes.data), ("depth", p.depth),
                                                                         ("n_local", 1), ("first", 0), ("n_sel", 1), ("n_rows", p.n_rows))])
    res = lambda **kw: fad.fad_adopt_resolve(*[kw.get(k, v) for k, v in (("tree", tree.ptr), ("cand", cand.ptr), ("flags", flags.ptr), ("out", out.ptr),   # noqa: E731
                                                                          ("offs", d_offs.data_ptr()), ("sizes", d_sizes.data_ptr()), ("depth", p.depth),
                                                                          ("n_local", 1), ("first", 0), ("n_sel", 1), ("n_below", p.offs[p.depth]), ("n_rows", p.n_rows))])
    assert lay(n_sel=0) == 0 and res(n_sel=0) == 0 and res(n_below=0) == 0                 # n == 0 launches no work
    for hole in ("tree", "cand", "flags", "roots", "offs", "sizes"):
        assert lay(**{hole: None}) == 1, hole                                             # hipErrorInvalidValue
    for hole in ("tree", "cand", "flags", "out", "offs", "sizes"):
        assert res(**{hole: None}) == 1, hole
    assert lay(depth=0) == 1 and res(depth=0) == 1
    assert lay(first=1) == 1 and lay(n_sel=2) == 1 and res(first=2) == 1 and res(n_sel=2) == 1
    wrong = sizes.copy()
    wrong[1] = 2
    assert lay(sizes=wrong.ctypes.data) == 1                                              # tables that are not a compact layout
    torch.cuda.synchronize()
    for o, a in ((tree, t0), (cand, c0), (flags, f0)):
        assert np.array_equal(o.fetch(), a.reshape(-1)) and o.guards_ok()
    assert np.array_equal(out.fetch(), out.prefill()) and out.guards_ok()
