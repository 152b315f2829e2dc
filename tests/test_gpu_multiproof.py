"""GPU suite: block multiproofs -- cp2_dataset_block_multiproofs serves the rows of groups of blocks from what a dataset keeps,
cp2_blocks_verify_multi checks groups of candidate blocks, each with its multiproof, against bare slot roots, and cp2_fill_add_multi adds
such groups to a fill session, which must then equal a twin filled by cp2_fill_add with the oracle's whole paths.  Expected values come from
the oracles (c_oracle for hashes and trees, tests/multiproof_models.py's layout for the places), never from another call of the library
except in the round trip.  Every comparison is bit-exact.  Geometries: (128, 4096, nCells) giving 1, 2, 5, 8 and 33 blocks (a dataset takes
the powers of two among them), and (2048, 65536, 4096) with 128 blocks."""
import ctypes
import faulthandler
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import multiproof_models as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CP2_OK, CP2_ERR_INVALID = 0, -1
N_SLOTS = 4
SMALL = {nb: (128, 4096, 32 * nb) for nb in (1, 2, 5, 8, 33)}
BIG = (2048, 65536, 4096)


@pytest.fixture(autouse=True)
def time_limit():
    """every case under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def sctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files_root(tmp_path_factory):
    return tmp_path_factory.mktemp("multiproofs")


# ---- the oracle's side ------------------------------------------------------------------------------------------------------------------
class Slot:
    """one slot's bytes as (nBlocks, blockSize), and the C oracle's tree over its block roots"""

    def __init__(self, C, cells, cs, bs):
        cpb = bs // cs
        leaves = C.hash_cells(cells, cs, threads=16)
        self.data = cells.reshape(-1, bs)
        self.block_roots = np.stack([C.merkle_tree(leaves[b * cpb:(b + 1) * cpb])[-1][0] for b in range(leaves.shape[0] // cpb)])
        self.layers = C.merkle_tree(self.block_roots)
        self.root = self.layers[-1][0]

    def rows(self, B):
        nodes = [self.layers[l][i] for l, i in M.layout(len(self.block_roots), B)]
        return np.stack(nodes) if nodes else np.zeros((0, 32), dtype=np.uint8)


_cache = {}


def slots_of(C, geom, source, tmp_root):
    """N_SLOTS slots of a geometry, computed once: fake source (seed 5) or slot files of random bytes; (file base or None, [Slot])"""
    key = (geom, source)
    if key not in _cache:
        cs, bs, nc = geom
        base = os.path.join(str(tmp_root), "g%d_slot" % nc) if source == "file" else None
        rng = np.random.default_rng(nc)
        out = []
        for s in range(N_SLOTS):
            if source == "file":
                cells = rng.integers(1, 256, nc * cs, dtype=np.uint8)
                cells.tofile("%s%d.dat" % (base, s))
            else:
                cells = C.gen_fake_cells(C.slot_seed(5, s), 0, nc, cs).reshape(-1)
            out.append(Slot(C, cells, cs, bs))
        _cache[key] = (base, out)
    return _cache[key]


def config(pkg, geom, base=None):
    cs, bs, nc = geom
    return pkg.make_config(maxDepth=16, maxLog2NSlots=2, cellSize=cs, blockSize=bs, nSlots=N_SLOTS, nCells=nc, nSamples=5, seed=5, file=base)


def build(ctx, cfg, mode):
    ctx.set_keep_trees(mode)
    try:
        ds = ctx.dataset(cfg)
    finally:
        ctx.set_keep_trees(-1)
    assert ds.tree_mode == mode
    return ds


def some_groups(nb, rng, n_groups):
    """(slot, B) groups over N_SLOTS slots: the kinds of the launcher test, slot 0 twice at least"""
    out = [(0, list(range(nb))), (0, [nb - 1])]
    while len(out) < n_groups:
        out.append((int(rng.integers(0, N_SLOTS)), M.pick(nb, str(rng.choice(M.KINDS)), rng)))
    return out


def flat(groups):
    return [(s, len(B)) for s, B in groups], [b for _, B in groups for b in B]


def call_of(slots, groups):
    """the arguments of a verify call from the oracle alone: (groups, blocks, data, nodes)"""
    g, b = flat(groups)
    data = np.concatenate([slots[s].data[B].reshape(-1) for s, B in groups])
    nodes = np.concatenate([slots[s].rows(B) for s, B in groups])
    return g, b, data, nodes


# ---- 1: serving ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("source", ["file", "fake"])
@pytest.mark.parametrize("nb", [1, 2, 8, 128])
def test_served_rows_equal_the_oracles_and_verify(pkg, oracle, sctx, files_root, nb, source, mode):
    C, _ = oracle
    geom = SMALL[nb] if nb in SMALL else BIG
    base, slots = slots_of(C, geom, source, files_root)
    ds = build(sctx, config(pkg, geom, base), mode)
    try:
        assert np.array_equal(ds.local_roots(), np.stack([s.root for s in slots]))
        groups = some_groups(nb, np.random.default_rng(nb), 9)              # slot 0 in two groups: two proofs
        g, b = flat(groups)
        roots, nodes = ds.block_multiproofs(g, b)
        assert roots.tobytes() == np.concatenate([slots[s].block_roots[B] for s, B in groups]).tobytes()
        assert nodes.tobytes() == np.concatenate([slots[s].rows(B) for s, B in groups]).tobytes()
        assert nodes.shape[0] == sum(pkg.block_multiproof_rows(*geom, B) for _, B in groups)
        _, again = ds.block_multiproofs(g, b, want_roots=False)            # serving is read-only: the same bytes again
        assert again.tobytes() == nodes.tobytes()
        # the round trip: what was served verifies against the slot roots, group by group
        data = np.concatenate([slots[s].data[B].reshape(-1) for s, B in groups])
        st, hashed = sctx.blocks_verify_multi(*geom, ds.local_roots(), g, b, data, nodes)
        assert st.tolist() == [pkg.BLOCK_MATCH] * len(groups) and hashed.tobytes() == roots.tobytes()
    finally:
        ds.free()


def test_serving_refuses_roots_only_and_a_small_cap(pkg, oracle, sctx, files_root):
    C, _ = oracle
    geom = SMALL[8]
    _, slots = slots_of(C, geom, "fake", files_root)
    L = sctx.L
    last_error = lambda: L.cp2_last_error(sctx.h).decode()          # noqa: E731
    ds0 = build(sctx, config(pkg, geom), 0)
    with pytest.raises(Exception, match="keeps only its slot roots"):
        ds0.block_multiproofs([(0, 1)], [3])
    ds0.free()
    ds = build(sctx, config(pkg, geom), 2)
    try:
        g, b = np.array([[1, 2], [3, 1]], dtype=np.uint64), np.array([0, 5, 6], dtype=np.uint64)
        need = len(M.layout(8, [0, 5])) + len(M.layout(8, [6]))
        nodes, roots = np.full((need, 32), 0x5E, dtype=np.uint8), np.full((3, 32), 0x5E, dtype=np.uint8)
        n_rows = ctypes.c_size_t(0)
        p = lambda a: a.ctypes.data                                  # noqa: E731
        assert L.cp2_dataset_block_multiproofs(ds.h, p(g), 2, p(b), p(roots), p(nodes), need - 1, ctypes.byref(n_rows)) == CP2_ERR_INVALID
        assert n_rows.value == need and str(need) in last_error() and (nodes == 0x5E).all() and (roots == 0x5E).all()
        assert L.cp2_dataset_block_multiproofs(ds.h, p(g), 2, p(b), p(roots), p(nodes), need, ctypes.byref(n_rows)) == CP2_OK
        assert nodes.tobytes() == np.concatenate([slots[1].rows([0, 5]), slots[3].rows([6])]).tobytes()
        assert roots.tobytes() == np.concatenate([slots[1].block_roots[[0, 5]], slots[3].block_roots[[6]]]).tobytes()
        # every rule of the requests, the outputs untouched
        nodes[:], roots[:] = 0x5E, 0x5E
        for groups, blocks, word in (([(1, 2), (3, 0)], [0, 5], "group 1 holds no block"), ([(1, 2), (4, 1)], [0, 5, 6], "group 1: slot 4"),
                                     ([(1, 2), (3, 1)], [0, 5, 8], "request 2: block 8"), ([(1, 2), (3, 1)], [5, 5, 6], "request 1: block 5 does not ascend")):
            gg, bb = np.array(groups, dtype=np.uint64), np.array(blocks, dtype=np.uint64)
            n_rows = ctypes.c_size_t(0x5E)
            assert L.cp2_dataset_block_multiproofs(ds.h, p(gg), len(groups), p(bb), p(roots), p(nodes), need, ctypes.byref(n_rows)) == CP2_ERR_INVALID
            assert word in last_error() and n_rows.value == 0x5E and (nodes == 0x5E).all() and (roots == 0x5E).all(), word
        assert L.cp2_dataset_block_multiproofs(ds.h, None, 0, None, None, None, 0, ctypes.byref(n_rows)) == CP2_OK and n_rows.value == 0
    finally:
        ds.free()


# ---- 2: verifying -------------------------------------------------------------------------------------------------------------------------
def plus_r(row):
    v = int.from_bytes(row.tobytes(), "little") + M.R_MOD
    return np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8) if v < 1 << 256 else None


@pytest.mark.parametrize("nb", [1, 2, 5, 8, 33])
def test_oracle_proofs_match_and_a_row_plus_r_still_matches(pkg, oracle, sctx, files_root, nb):
    C, _ = oracle
    geom = SMALL[nb]
    _, slots = slots_of(C, geom, "fake", files_root)
    roots = np.stack([s.root for s in slots])
    groups = some_groups(nb, np.random.default_rng(100 + nb), 12)
    g, b, data, nodes = call_of(slots, groups)
    st, hashed = sctx.blocks_verify_multi(*geom, roots, g, b, data, nodes)
    assert st.tolist() == [pkg.BLOCK_MATCH] * 12
    assert hashed.tobytes() == np.concatenate([slots[s].block_roots[B] for s, B in groups]).tobytes()
    lifted, n = nodes.copy(), 0
    for j in range(len(lifted)):
        up = plus_r(lifted[j])
        if up is not None:
            lifted[j], n = up, n + 1
    assert n > 0 or nb == 1
    assert sctx.blocks_verify_multi(*geom, roots, g, b, data, lifted, want_roots=False)[0].tolist() == [pkg.BLOCK_MATCH] * 12
    stated = roots.copy()                                               # a stated root + r is the same field element too
    k = next(k for k in range(N_SLOTS) if plus_r(stated[k]) is not None)
    stated[k] = plus_r(stated[k])
    assert sctx.blocks_verify_multi(*geom, stated, g, b, data, nodes, want_roots=False)[0].tolist() == [pkg.BLOCK_MATCH] * 12


def corrupted_call(slots, nb, seed):
    """Twelve groups in one call; groups 1, 3, 5, 7, 9 and 11 each take ONE corruption.  Returns (stated roots, groups, blocks, data, nodes,
    the names of the corruptions by group).  Groups 3, 5 and 9 are one low block each (two sent rows or more); group 7 states the root of
    another slot (root index 4: a fifth stated root); group 11 is one even block whose index is moved to its neighbour's, which keeps
    the size of its layout."""
    rng = np.random.default_rng(seed)
    bs = slots[0].data.shape[1]
    groups = []
    for k in range(12):
        if k == 11:
            B = [2 * int(rng.integers(0, nb // 2))]
        elif k in (3, 5, 9):
            B = [k // 4]
        else:
            B = M.pick(nb, M.KINDS[k % len(M.KINDS)], rng)
        groups.append((k % N_SLOTS, B))
    g, b, data, nodes = call_of(slots, groups)
    stated = np.concatenate([np.stack([s.root for s in slots]), slots[(7 + 1) % N_SLOTS].root[None]])
    off_req = np.cumsum([0] + [len(B) for _, B in groups])
    off_row = np.cumsum([0] + [len(M.layout(nb, B)) for _, B in groups])
    assert all(off_row[k + 1] - off_row[k] >= 2 for k in (3, 5, 9))
    data = data.copy().reshape(-1, bs)
    data[off_req[2] - 1, bs - 1] ^= 1                                   # the last byte of group 1's last block
    nodes[off_row[3], 0] ^= 1
    first, last = off_row[5], off_row[6] - 1
    assert not np.array_equal(nodes[first], nodes[last])
    nodes[[first, last]] = nodes[[last, first]]
    g[7] = (4, g[7][1])
    nodes[off_row[10] - 1, 28] ^= 1                                     # the last row of group 9
    b[off_req[11]] ^= 1
    what = {1: "a data byte", 3: "a sent row's low byte", 5: "two sent rows swapped", 7: "a wrong stated root", 9: "a sent row's top limb",
            11: "a block index moved to a neighbour's"}
    return stated, g, b, data.reshape(-1), nodes, what


@pytest.mark.parametrize("nb", [5, 8, 33])
def test_each_single_corruption_fails_exactly_its_own_group(pkg, oracle, sctx, files_root, nb):
    C, _ = oracle
    geom = SMALL[nb]
    _, slots = slots_of(C, geom, "fake", files_root)
    stated, g, b, data, nodes, what = corrupted_call(slots, nb, 200 + nb)
    st, _ = sctx.blocks_verify_multi(*geom, stated, g, b, data, nodes)
    want = [pkg.BLOCK_MISMATCH if k in what else pkg.BLOCK_MATCH for k in range(12)]
    assert st.tolist() == want, {k: what.get(k, "intact") for k in range(12) if st[k] != want[k]}


CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as g
job = json.loads(sys.argv[1])
pkg = g.load_package()
ctx = pkg.Context(0)
stated, groups, blocks, data, nodes = (np.load(job[k]) for k in ("stated", "groups", "blocks", "data", "nodes"))
st, roots = ctx.blocks_verify_multi(*job["geom"], stated, groups, blocks, data, nodes)
ctx.close()
print(json.dumps({"status": st.tolist(), "roots_sha": __import__("hashlib").sha256(roots.tobytes()).hexdigest()}), flush=True)
""" % ROOT


def test_groups_that_straddle_chunks_get_the_same_verdicts(pkg, oracle, sctx, files_root, tmp_path):
    """128 blocks of 64 KiB under CODEX_P2_STAGE_MB=1: chunks of 8 requests, so nearly every group lies in several chunks.  The child's
    verdicts and roots equal this process's (one chunk) and the planted pattern."""
    C, _ = oracle
    _, slots = slots_of(C, BIG, "fake", files_root)
    stated, g, b, data, nodes, what = corrupted_call(slots, 128, 328)
    assert max(c for _, c in g) > 16 and sum(c for _, c in g) > 64
    names = {}
    for k, a in (("stated", stated), ("groups", np.array(g, dtype=np.uint64)), ("blocks", np.array(b, dtype=np.uint64)), ("data", data), ("nodes", nodes)):
        names[k] = str(tmp_path / (k + ".npy"))
        np.save(names[k], a)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("CODEX_P2_")}
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(dict(names, geom=list(BIG)))], capture_output=True, text=True, timeout=200,
                       env=dict(clean, CODEX_P2_STAGE_MB="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    st, roots = sctx.blocks_verify_multi(*BIG, stated, g, b, data, nodes)
    want = [pkg.BLOCK_MISMATCH if k in what else pkg.BLOCK_MATCH for k in range(12)]
    assert st.tolist() == want and got["status"] == want
    assert got["roots_sha"] == hashlib.sha256(roots.tobytes()).hexdigest()


def test_verify_refusals_in_their_order_with_outputs_untouched(pkg, oracle, sctx, files_root):
    C, _ = oracle
    nb, geom = 8, SMALL[8]
    _, slots = slots_of(C, geom, "fake", files_root)
    L = sctx.L
    last_error = lambda: L.cp2_last_error(sctx.h).decode()          # noqa: E731
    stated = np.stack([s.root for s in slots])
    good = [(1, [0, 5]), (3, [6]), (0, [1, 2, 7])]
    g, b, data, nodes = call_of(slots, good)
    rows = len(nodes)
    p = lambda a: a.ctypes.data if a is not None else None           # noqa: E731

    def call(groups=g, blocks=b, n_rows=rows, h=sctx.h, geom=geom, stated=stated, data=data, nodes=nodes, with_status=True, n_roots=N_SLOTS):
        gg, bb = np.array(groups, dtype=np.uint64).reshape(-1, 2), np.array(blocks, dtype=np.uint64)
        status, out = np.full(len(gg), 0x5E5E5E5E, dtype=np.uint32), np.full((len(bb), 32), 0x5E, dtype=np.uint8)
        r = L.cp2_blocks_verify_multi(h, *geom, p(stated), n_roots, p(gg), len(gg), p(bb), p(data), p(nodes), n_rows, p(status) if with_status else None,
                                      p(out))
        return r, bool((status == 0x5E5E5E5E).all() and (out == 0x5E).all())

    assert call(h=None) == (CP2_ERR_INVALID, True)                                             # 1: a NULL context
    assert call(geom=(128, 4096, 255)) == (CP2_ERR_INVALID, True) and "geometry" in last_error()  # 2
    for kw in (dict(stated=None), dict(data=None), dict(nodes=None), dict(with_status=False)):  # 3: NULL arrays
        assert call(**kw) == (CP2_ERR_INVALID, True) and "must not be NULL" in last_error(), kw
    # 4 ... 8: every later rule is broken too, in a lower group: the order decides
    for groups, blocks, n_rows, word in (([(1, 2), (3, 0), (9, 3)], [0, 8, 1, 1, 7], rows, "group 1 holds no block"),
                                         ([(1, 2), (3, 1), (4, 3)], [8, 0, 6, 1, 1, 7], rows, "group 2: root index 4"),
                                         ([(1, 2), (3, 1), (0, 3)], [5, 5, 6, 1, 8, 7], rows, "group 2, request 4: block 8"),
                                         ([(1, 2), (3, 1), (0, 3)], [0, 5, 6, 2, 2, 7], rows + 1, "group 2, request 4: block 2 does not ascend"),
                                         (g, b, rows + 1, "n_rows = %d, the groups' layouts hold %d rows" % (rows + 1, rows))):
        assert call(groups=groups, blocks=blocks, n_rows=n_rows) == (CP2_ERR_INVALID, True), word
        assert word in last_error(), (word, last_error())
    assert L.cp2_blocks_verify_multi(sctx.h, *geom, None, 0, None, 0, None, None, None, 0, None, None) == CP2_OK      # n_groups == 0
    st, _ = sctx.blocks_verify_multi(*geom, stated, g, b, data, nodes)                          # and the same arguments, valid
    assert st.tolist() == [pkg.BLOCK_MATCH] * 3


# ---- 3: filling ---------------------------------------------------------------------------------------------------------------------------
def whole_path(slot, b):
    """merkleProof of block b from the oracle's tree: one sibling per level, bottom first, zero where it lies past its layer"""
    rows = []
    for l in range(M.depth(len(slot.block_roots))):
        sib = (b >> l) ^ 1
        rows.append(slot.layers[l][sib] if sib < len(slot.layers[l]) else np.zeros(32, dtype=np.uint8))
    return np.stack(rows)


def split_groups(nb, rng):
    """every block of every slot once, in two or three groups per slot, the groups of all slots shuffled: [(slot, B)]"""
    out = []
    for s in range(N_SLOTS):
        parts = min(nb, int(rng.integers(2, 4)))
        owner = rng.integers(0, parts, nb)
        owner[:parts] = np.arange(parts)
        out += [(s, [b for b in range(nb) if owner[b] == k]) for k in range(parts)]
    return [out[i] for i in rng.permutation(len(out))]


def multi_add(f, slots, groups):
    g, b, data, nodes = call_of(slots, groups)
    return f.add_multi(g, b, data, nodes)


def whole_add(f, slots, groups):
    pairs = [(s, b) for s, B in groups for b in B]
    data = np.concatenate([slots[s].data[b] for s, b in pairs])
    return f.add(pairs, data, np.stack([whole_path(slots[s], b) for s, b in pairs]))


def same_state(f, twin, nb, keeps):
    assert f.missing()[0].tobytes() == twin.missing()[0].tobytes()
    if keeps:
        every = [(s, b) for s in range(N_SLOTS) for b in range(nb)]
        for x, y in zip(f.block_proofs(every), twin.block_proofs(every)):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("keeps", [False, True])
@pytest.mark.parametrize("source", ["file", "fake"])
@pytest.mark.parametrize("nb", [1, 8, 128])
def test_a_multi_add_leaves_what_one_whole_path_add_leaves(pkg, oracle, sctx, files_root, tmp_path, nb, source, keeps):
    C, _ = oracle
    geom = SMALL[nb] if nb in SMALL else BIG
    base, slots = slots_of(C, geom, source, files_root)
    roots = np.stack([s.root for s in slots])
    bases = [str(tmp_path / name) if source == "file" else None for name in ("multi_slot", "twin_slot")]
    f, twin = (sctx.fill(config(pkg, geom, b), roots) for b in bases)
    built = filled = None
    try:
        if keeps:
            f.keep_nodes()
            twin.keep_nodes()
        groups = split_groups(nb, np.random.default_rng(300 + nb))
        half = len(groups) // 2
        calls = [groups[:half], groups[half:] + groups[:1]]                     # the second call repeats a group: DUPLICATEs
        for call in calls:
            got, want = multi_add(f, slots, call), whole_add(twin, slots, call)
            assert got[0].tolist() == want[0].tolist() and got[1] == want[1]
            same_state(f, twin, nb, keeps)
        assert f.missing()[1] == 0
        if source == "file":
            for s in range(N_SLOTS):
                assert open("%s%d.dat" % (bases[0], s), "rb").read() == open("%s%d.dat" % (bases[1], s), "rb").read() == slots[s].data.tobytes()
        filled = f.finish()
        built = build(sctx, config(pkg, geom, base), 2)
        assert filled.local_roots().tobytes() == built.local_roots().tobytes() == roots.tobytes()
        for ds in (filled, built):
            ds.set_roots()
        assert filled.proof_input(1, 1234567).json() == built.proof_input(1, 1234567).json()
        with pytest.raises(pkg.CodexP2Error, match="finished"):                  # the last refusal: a finished session
            multi_add(f, slots, groups[:1])
    finally:
        for h in (f, twin, filled, built):
            if h is not None:
                h.free()


def test_a_failed_group_leaves_nothing_and_is_new_when_sent_again(pkg, oracle, sctx, files_root):
    C, _ = oracle
    nb, geom = 8, SMALL[8]
    _, slots = slots_of(C, geom, "fake", files_root)
    f = sctx.fill(config(pkg, geom), np.stack([s.root for s in slots]))
    try:
        f.keep_nodes()
        groups = [(0, [0, 1, 6]), (2, [1, 3, 4]), (3, [7]), (2, [5])]
        g, b, data, nodes = call_of(slots, groups)
        every = [(s, x) for s in range(N_SLOTS) for x in range(nb)]
        before_missing, before_proofs = f.missing()[0].copy(), [x.copy() for x in f.block_proofs(every)]
        first_row = len(M.layout(nb, groups[0][1]))
        bad = nodes.copy()
        bad[first_row + 1, 5] ^= 4                                              # one row of group 1
        status, n_new = f.add_multi(g, b, data, bad)
        N, X = pkg.FILL_NEW, pkg.FILL_MISMATCH
        assert status.tolist() == [N, N, N, X, X, X, N, N] and n_new == 5
        # group 1 left nothing: what is missing and what is served differ from before only by the other groups' blocks
        twin = sctx.fill(config(pkg, geom), np.stack([s.root for s in slots]))
        twin.keep_nodes()
        assert whole_add(twin, slots, [groups[0], groups[2], groups[3]])[0].tolist() == [N] * 5
        same_state(f, twin, nb, True)
        assert len(f.missing()[0]) == len(before_missing) - 5 and [x.shape for x in f.block_proofs(every)] == [x.shape for x in before_proofs]
        status, n_new = f.add_multi([g[1]], groups[1][1], data.reshape(-1, geom[1])[3:6].reshape(-1), slots[2].rows(groups[1][1]))
        assert status.tolist() == [N, N, N] and n_new == 3
        assert whole_add(twin, slots, [groups[1]])[0].tolist() == [N] * 3
        same_state(f, twin, nb, True)
        twin.free()
    finally:
        f.free()


def test_a_block_in_two_proved_groups_is_new_once(pkg, oracle, sctx, files_root):
    C, _ = oracle
    nb, geom = 8, SMALL[8]
    _, slots = slots_of(C, geom, "fake", files_root)
    f = sctx.fill(config(pkg, geom), np.stack([s.root for s in slots]))
    try:
        status, n_new = multi_add(f, slots, [(1, [2, 5]), (1, [5, 6]), (1, [2])])
        N, D = pkg.FILL_NEW, pkg.FILL_DUPLICATE
        assert status.tolist() == [N, N, D, N, D] and n_new == 3                 # the lower index is NEW, the other DUPLICATE
        assert multi_add(f, slots, [(1, [5, 7])])[0].tolist() == [D, N]
    finally:
        f.free()


def test_fill_refusals_leave_the_session_and_the_outputs_alone(pkg, oracle, sctx, files_root):
    C, _ = oracle
    nb, geom = 8, SMALL[8]
    _, slots = slots_of(C, geom, "fake", files_root)
    f = sctx.fill(config(pkg, geom), np.stack([s.root for s in slots]))
    L = sctx.L
    last_error = lambda: L.cp2_last_error(sctx.h).decode()          # noqa: E731
    p = lambda a: a.ctypes.data if a is not None else None           # noqa: E731
    try:
        g, b, data, nodes = call_of(slots, [(1, [0, 5]), (3, [6]), (0, [1, 2, 7])])
        rows = len(nodes)
        for groups, blocks, n_rows, null, word in ((g, b, rows, "data", "must not be NULL"), ([(1, 2), (3, 0), (9, 3)], [0, 8, 1, 1, 7], rows, None, "group 1 holds no block"),
                                                   ([(1, 2), (3, 1), (4, 3)], [8, 0, 6, 1, 1, 7], rows, None, "group 2: slot 4"),
                                                   ([(1, 2), (3, 1), (0, 3)], [5, 5, 6, 1, 8, 7], rows, None, "group 2, request 4: block 8"),
                                                   ([(1, 2), (3, 1), (0, 3)], [0, 5, 6, 2, 2, 7], rows + 1, None, "request 4: block 2 does not ascend"),
                                                   (g, b, rows - 1, None, "n_rows = %d, the groups' layouts hold %d rows" % (rows - 1, rows))):
            gg, bb = np.array(groups, dtype=np.uint64), np.array(blocks, dtype=np.uint64)
            status, n_new = np.full(len(bb), 0x5E5E5E5E, dtype=np.uint32), ctypes.c_size_t(0x5E)
            r = L.cp2_fill_add_multi(f.h, p(gg), len(gg), p(bb), None if null == "data" else p(data), p(nodes), n_rows, p(status), ctypes.byref(n_new))
            assert r == CP2_ERR_INVALID and word in last_error(), (word, last_error())
            assert (status == 0x5E5E5E5E).all() and n_new.value == 0x5E and f.missing()[1] == N_SLOTS * nb
        n_new = ctypes.c_size_t(0x5E)
        assert L.cp2_fill_add_multi(f.h, None, 0, None, None, None, 0, None, ctypes.byref(n_new)) == CP2_OK and n_new.value == 0
    finally:
        f.free()
