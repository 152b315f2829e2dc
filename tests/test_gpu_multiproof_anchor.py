"""GPU suite: multiproofs against what a fill session knows -- cp2_fill_multiproof_want names the rows a group still needs,
cp2_dataset_block_tree_rows and cp2_fill_block_tree_rows serve rows by their place, cp2_fill_add_multi_anchored adds the group.  A session
filled this way must equal, after every step, a twin filled by cp2_fill_anchors -> truncated cp2_dataset_block_proofs ->
cp2_fill_add_anchored over the same requests: what is missing, the anchors of every block, every tree row by place (statuses and bytes)
and the per-request statuses; served rows are held to the C oracle's trees.  Every comparison is bit-exact.

Geometry: cell 128, block 4096 (32 cells a block), fake source (one variant on slot files), 1 to 3 slots.  A dataset and a fill session take
a power-of-two cell count only (cp2_fill_begin refuses the rest, which the last test states), so the calls run at 1, 2, 4, 8, 16 and 32
blocks; the odd layers of 3, 5, 9 and 33 blocks are covered where they can be built: in the plan against the model
(tests/test_multiproof_anchor_cpu.py) and at the launcher over oracle trees (tests/test_gpu_multiproof_anchor_unit.py)."""
import ctypes
import faulthandler

import numpy as np
import pytest

import multiproof_models as M

pytestmark = pytest.mark.gpu

CP2_OK, CP2_ERR_INVALID = 0, -1
CELL, BLOCK = 128, 4096


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


# ---- the oracle's side ------------------------------------------------------------------------------------------------------------------
class Slot:
    """one slot's bytes as (nBlocks, blockSize), and the C oracle's tree over its block roots"""

    def __init__(self, C, cells):
        cpb = BLOCK // CELL
        leaves = C.hash_cells(cells, CELL, threads=16)
        self.data = cells.reshape(-1, BLOCK)
        self.block_roots = np.stack([C.merkle_tree(leaves[b * cpb:(b + 1) * cpb])[-1][0] for b in range(leaves.shape[0] // cpb)])
        self.layers = C.merkle_tree(self.block_roots)
        self.root = self.layers[-1][0]


_cache = {}


def slots_of(C, nb, n_slots, base=None):
    """the slots of a geometry, computed once: fake source (seed 5), or slot files of random bytes under `base`"""
    key = (nb, n_slots, base)
    if key not in _cache:
        rng, out = np.random.default_rng(nb), []
        for s in range(n_slots):
            if base:
                cells = rng.integers(1, 256, 32 * nb * CELL, dtype=np.uint8)
                cells.tofile("%s%d.dat" % (base, s))
            else:
                cells = C.gen_fake_cells(C.slot_seed(5, s), 0, 32 * nb, CELL).reshape(-1)
            out.append(Slot(C, cells))
        _cache[key] = out
    return _cache[key]


def config(pkg, nb, n_slots, base=None):
    return pkg.make_config(maxDepth=16, maxLog2NSlots=2, cellSize=CELL, blockSize=BLOCK, nSlots=n_slots, nCells=32 * nb, nSamples=5, seed=5, file=base)


def build(ctx, cfg, mode):
    ctx.set_keep_trees(mode)
    try:
        ds = ctx.dataset(cfg)
    finally:
        ctx.set_keep_trees(-1)
    assert ds.tree_mode == mode
    return ds


def every_place(nb, n_slots):
    return [(s, l, i) for s in range(n_slots) for l, m in enumerate(M.layer_sizes(nb)) for i in range(m)]


def flat(groups):
    return [(s, len(B)) for s, B in groups], [b for _, B in groups for b in B]


def data_of(slots, groups):
    return np.concatenate([slots[s].data[B].reshape(-1) for s, B in groups])


def want_places(f, groups):
    """the want lists of the groups against f as it stands, as (slot, level, index) places in packed order"""
    g, b = flat(groups)
    li, per = f.multiproof_want(g, b)
    assert int(per.sum()) == li.shape[0]
    slot_of = np.repeat([s for s, _ in groups], per.astype(np.int64))
    return [(int(s), int(l), int(i)) for s, (l, i) in zip(slot_of, li)], per


def anchored_multi_add(f, peer, slots, groups):
    """the new way: the want list, the peer's rows by place, the add.  Returns (status, n_new, rows received)"""
    g, b = flat(groups)
    pl, _ = want_places(f, groups)
    rows = peer.block_tree_rows(pl) if pl else np.zeros((0, 32), dtype=np.uint8)
    if isinstance(rows, tuple):                            # a peer that is a session also says which rows it knows
        assert (rows[0] == 0).all()
        rows = rows[1]
    return f.add_multi_anchored(g, b, data_of(slots, groups), rows) + (len(pl),)


def anchored_add(f, ds, slots, groups):
    """the existing way: one truncated whole path per block.  Returns (status, n_new, siblings received)"""
    pairs = [(s, b) for s, B in groups for b in B]
    levels = f.anchors(pairs)
    _, paths = ds.block_proofs(pairs)
    packed = np.concatenate([paths[i, :int(a)] for i, a in enumerate(levels)] + [np.zeros((0, 32), dtype=np.uint8)])
    return f.add_anchored(pairs, data_of(slots, groups), levels, packed if packed.size else None) + (packed.shape[0],)


def state(f, nb, n_slots):
    every = [(s, b) for s in range(n_slots) for b in range(nb)]
    st, rows = f.block_tree_rows(every_place(nb, n_slots))
    return f.missing()[0].tobytes(), f.anchors(every).tobytes(), st.tobytes(), rows.tobytes()


def held_to_the_oracle(f, slots, nb):
    """every row the session calls known is the oracle's node at its place; every other row comes back as zeros"""
    pl = every_place(nb, len(slots))
    st, rows = f.block_tree_rows(pl)
    for (s, l, i), k, row in zip(pl, st, rows):
        assert row.tobytes() == (slots[s].layers[l][i].tobytes() if k == 0 else bytes(32)), (s, l, i, int(k))
    assert f.block_tree_rows(pl, statuses_only=True).tobytes() == st.tobytes()


def split_calls(nb, n_slots, rng):
    """every block of every slot once, in seeded random groups, one to three groups a call: [[(slot, B)]]"""
    groups = []
    for s in range(n_slots):
        order, at = [int(x) for x in rng.permutation(nb)], 0
        while at < nb:
            k = int(rng.integers(1, max(2, nb // 2) + 1))
            groups.append((s, sorted(order[at:at + k])))
            at += k
    groups = [groups[i] for i in rng.permutation(len(groups))]
    calls, at = [], 0
    while at < len(groups):
        k = int(rng.integers(1, 4))
        calls.append(groups[at:at + k])
        at += k
    return calls


# ---- 1: twin sessions -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,n_slots,source", [(1, 3, "fake"), (2, 2, "fake"), (4, 3, "fake"), (8, 3, "fake"), (16, 1, "fake"), (32, 2, "fake"), (8, 2, "file")])
def test_twin_sessions_stay_equal_step_by_step(pkg, oracle, sctx, tmp_path, nb, n_slots, source):
    C, _ = oracle
    base = str(tmp_path / "src_slot") if source == "file" else None
    slots = slots_of(C, nb, n_slots, base)
    roots = np.stack([s.root for s in slots])
    bases = [str(tmp_path / name) if source == "file" else None for name in ("multi_slot", "twin_slot")]
    built = build(sctx, config(pkg, nb, n_slots, base), 2)
    f, twin = (sctx.fill(config(pkg, nb, n_slots, b), roots) for b in bases)
    filled = None
    try:
        assert built.local_roots().tobytes() == roots.tobytes()
        f.keep_nodes()
        twin.keep_nodes()
        received, siblings = 0, 0
        for call in split_calls(nb, n_slots, np.random.default_rng(500 + nb)):
            got, want = anchored_multi_add(f, built, slots, call), anchored_add(twin, built, slots, call)
            assert got[0].tolist() == want[0].tolist() == [pkg.FILL_NEW] * len(got[0]) and got[1] == want[1]
            assert state(f, nb, n_slots) == state(twin, nb, n_slots)
            assert got[2] <= want[2]
            received, siblings = received + got[2], siblings + want[2]
        held_to_the_oracle(f, slots, nb)
        assert received <= n_slots * (nb - 1) and f.missing()[1] == 0
        if source == "file":
            for s in range(n_slots):
                assert open("%s%d.dat" % (bases[0], s), "rb").read() == open("%s%d.dat" % (bases[1], s), "rb").read() == slots[s].data.tobytes()
        filled = f.finish()
        assert filled.local_roots().tobytes() == roots.tobytes()
        with pytest.raises(pkg.CodexP2Error, match="finished"):
            f.multiproof_want([(0, 1)], [0])
        with pytest.raises(pkg.CodexP2Error, match="finished"):
            f.block_tree_rows([(0, 0, 0)])
    finally:
        for h in (f, twin, filled, built):
            if h is not None:
                h.free()


def test_one_group_of_everything_receives_no_row_and_no_node_is_hashed_twice(pkg, oracle, sctx):
    C, _ = oracle
    nb, n_slots = 16, 2
    slots = slots_of(C, nb, n_slots)
    f = sctx.fill(config(pkg, nb, n_slots), np.stack([s.root for s in slots]))
    try:
        f.keep_nodes()
        groups = [(s, list(range(nb))) for s in range(n_slots)]
        pl, per = want_places(f, groups)
        assert pl == [] and per.tolist() == [0, 0]
        g, b = flat(groups)
        status, n_new = f.add_multi_anchored(g, b, data_of(slots, groups), None)
        assert status.tolist() == [pkg.FILL_NEW] * (n_slots * nb) and n_new == n_slots * nb
        held_to_the_oracle(f, slots, nb)
        assert (f.block_tree_rows(every_place(nb, n_slots), statuses_only=True) == 0).all()
    finally:
        f.free()


# ---- 2: two half-filled sessions fill each other --------------------------------------------------------------------------------------------
def test_two_half_filled_sessions_fill_each_other(pkg, oracle, sctx):
    C, _ = oracle
    nb = 8
    slots = slots_of(C, nb, 1)
    cfg, roots = config(pkg, nb, 1), np.stack([s.root for s in slots])
    built = build(sctx, cfg, 2)
    low, high, thin = (sctx.fill(cfg, roots) for _ in range(3))
    try:
        for f, B in ((low, [0, 1, 2, 3]), (high, [4, 5, 6, 7]), (thin, [4])):
            f.keep_nodes()
            assert anchored_multi_add(f, built, slots, [(0, B)])[0].tolist() == [pkg.FILL_NEW] * len(B)
        # the halves serve each other what is wanted: the other half's subtree needs nothing but its blocks
        assert want_places(low, [(0, [5])])[0] == [(0, 0, 4), (0, 1, 3)] and want_places(high, [(0, [0, 1, 2, 3])])[0] == []
        for f, peer, B in ((low, high, [5]), (high, low, [0, 3]), (low, high, [4, 6, 7]), (high, low, [1, 2])):
            status, n_new, _ = anchored_multi_add(f, peer, slots, [(0, B)])
            assert status.tolist() == [pkg.FILL_NEW] * len(B) and n_new == len(B)
            held_to_the_oracle(f, slots, nb)
        assert low.missing()[1] == 0 and high.missing()[1] == 0
        # a peer that does not know a wanted row says so, serves zeros, and the add with them fails its group
        third = sctx.fill(cfg, roots)
        third.keep_nodes()
        assert anchored_multi_add(third, built, slots, [(0, [0, 1, 2, 3])])[0].tolist() == [pkg.FILL_NEW] * 4
        pl, _ = want_places(third, [(0, [6])])
        assert pl == [(0, 0, 7), (0, 1, 2)]
        st, rows = thin.block_tree_rows(pl)
        assert st.tolist() == [pkg.FILL_ROW_UNKNOWN, pkg.FILL_ROW_KNOWN] and rows[0].tobytes() == bytes(32) and rows[1].tobytes() == slots[0].layers[1][2].tobytes()
        before = state(third, nb, 1)
        status, n_new = third.add_multi_anchored([(0, 1)], [6], slots[0].data[6], rows)
        assert status.tolist() == [pkg.FILL_MISMATCH] and n_new == 0 and state(third, nb, 1) == before
        third.free()
    finally:
        for h in (low, high, thin, built):
            h.free()


# ---- 3: rows by place from a dataset ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("nb,n_slots", [(1, 2), (2, 3), (8, 3), (32, 1)])
def test_a_datasets_tree_rows_are_the_oracles_at_every_place(pkg, oracle, sctx, nb, n_slots, mode):
    C, _ = oracle
    slots = slots_of(C, nb, n_slots)
    ds = build(sctx, config(pkg, nb, n_slots), mode)
    try:
        pl = every_place(nb, n_slots)
        pl = [pl[i] for i in np.random.default_rng(nb).permutation(len(pl))] + pl[:3]       # any order, a place twice
        rows = ds.block_tree_rows(pl)
        assert rows.tobytes() == b"".join(slots[s].layers[l][i].tobytes() for s, l, i in pl)
        assert ds.block_tree_rows([]).shape == (0, 32)
    finally:
        ds.free()


def test_tree_rows_refusals_leave_the_outputs_alone(pkg, oracle, sctx):
    C, _ = oracle
    nb, n_slots = 8, 3
    slots = slots_of(C, nb, n_slots)
    cfg = config(pkg, nb, n_slots)
    L = sctx.L
    last_error = lambda: L.cp2_last_error(sctx.h).decode()          # noqa: E731
    p = lambda a: a.ctypes.data if a is not None else None           # noqa: E731
    bad = (([(0, 0, 0), (3, 0, 0)], "request 1: slot 3"), ([(0, 4, 0), (3, 0, 0)], "request 0: level 4"), ([(0, 0, 0), (1, 2, 2)], "request 1: index 2"),
           ([(0, 3, 1)], "request 0: index 1"))
    ds0 = build(sctx, cfg, 0)
    with pytest.raises(pkg.CodexP2Error, match="keeps only its slot roots"):
        ds0.block_tree_rows([(0, 0, 0)])
    ds0.free()
    ds = build(sctx, cfg, 2)
    f, plain = sctx.fill(cfg, np.stack([s.root for s in slots])), sctx.fill(cfg, np.stack([s.root for s in slots]))
    try:
        f.keep_nodes()
        rows, status = np.full((2, 32), 0x5E, dtype=np.uint8), np.full(2, 0x5E5E5E5E, dtype=np.uint32)
        for places, word in bad:
            pl = np.array(places, dtype=np.uint64)
            assert L.cp2_dataset_block_tree_rows(ds.h, p(pl), len(places), p(rows)) == CP2_ERR_INVALID and word in last_error(), (word, last_error())
            assert L.cp2_fill_block_tree_rows(f.h, p(pl), len(places), p(status), p(rows)) == CP2_ERR_INVALID and word in last_error(), (word, last_error())
            assert (rows == 0x5E).all() and (status == 0x5E5E5E5E).all()
        pl = np.array([(0, 0, 0), (1, 3, 0)], dtype=np.uint64)
        assert L.cp2_dataset_block_tree_rows(ds.h, None, 2, p(rows)) == CP2_ERR_INVALID and L.cp2_dataset_block_tree_rows(ds.h, p(pl), 2, None) == CP2_ERR_INVALID
        assert L.cp2_fill_block_tree_rows(f.h, p(pl), 2, None, p(rows)) == CP2_ERR_INVALID and "must not be NULL" in last_error()
        assert L.cp2_fill_block_tree_rows(plain.h, p(pl), 2, p(status), p(rows)) == CP2_ERR_INVALID and "cp2_fill_keep_nodes" in last_error()
        assert (rows == 0x5E).all() and (status == 0x5E5E5E5E).all()
        # the stated slot root is known from the start, and nothing else of an empty session is
        st, got = f.block_tree_rows([(0, 0, 0), (1, 3, 0), (2, 2, 1)])
        assert st.tolist() == [1, 0, 1] and got[1].tobytes() == slots[1].root.tobytes() and got[0].tobytes() == got[2].tobytes() == bytes(32)
    finally:
        for h in (f, plain, ds):
            h.free()


# ---- 4: failing groups ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cause", ["a data byte", "a sent row", "a right row at the wrong position"])
def test_a_failing_group_leaves_nothing_and_its_neighbours_land(pkg, oracle, sctx, cause):
    C, _ = oracle
    nb, n_slots = 8, 2
    slots = slots_of(C, nb, n_slots)
    cfg, roots = config(pkg, nb, n_slots), np.stack([s.root for s in slots])
    built = build(sctx, cfg, 2)
    f, twin = sctx.fill(cfg, roots), sctx.fill(cfg, roots)
    try:
        for h in (f, twin):
            h.keep_nodes()
            assert anchored_multi_add(h, built, slots, [(0, [6]), (1, [1])])[1] == 2
        groups = [(0, [0, 3]), (1, [4, 7]), (0, [5])]        # the middle group fails
        g, b = flat(groups)
        pl, per = want_places(f, groups)
        rows, data = built.block_tree_rows(pl), data_of(slots, groups).copy()
        r0, r1 = int(per[0]), int(per[0] + per[1])
        assert r1 - r0 >= 2
        if cause == "a data byte":
            data[3 * BLOCK + 17] ^= 1                                          # the second block of the group
        elif cause == "a sent row":
            rows[r0 + 1, 3] ^= 0x10
        else:
            assert not np.array_equal(rows[r0], rows[r1 - 1])
            rows[[r0, r1 - 1]] = rows[[r1 - 1, r0]]
        status, n_new = f.add_multi_anchored(g, b, data, rows)
        N, X = pkg.FILL_NEW, pkg.FILL_MISMATCH
        assert status.tolist() == [N, N, X, X, N] and n_new == 3
        # what the failing group would have left is not there: the session equals a twin that was never sent it
        assert anchored_multi_add(twin, built, slots, [groups[0], groups[2]])[0].tolist() == [N, N, N]
        assert state(f, nb, n_slots) == state(twin, nb, n_slots)
        held_to_the_oracle(f, slots, nb)
        assert anchored_multi_add(f, built, slots, [groups[1]])[0].tolist() == [N, N]   # sent again intact, it is new
    finally:
        for h in (f, twin, built):
            h.free()


# ---- 5: NEW and DUPLICATE -------------------------------------------------------------------------------------------------------------------
def test_new_and_duplicate(pkg, oracle, sctx):
    C, _ = oracle
    nb, n_slots = 8, 2
    slots = slots_of(C, nb, n_slots)
    cfg, roots = config(pkg, nb, n_slots), np.stack([s.root for s in slots])
    built = build(sctx, cfg, 2)
    f = sctx.fill(cfg, roots)
    N, D = pkg.FILL_NEW, pkg.FILL_DUPLICATE
    try:
        f.keep_nodes()
        assert anchored_multi_add(f, built, slots, [(0, [2, 5])])[:2][1] == 2
        # a group of present blocks: every top is a block root, nothing is wanted, all DUPLICATE
        assert want_places(f, [(0, [2, 5])])[0] == []
        status, n_new, got = anchored_multi_add(f, built, slots, [(0, [2, 5])])
        assert status.tolist() == [D, D] and n_new == 0 and got == 0
        # an absent block whose root is known (it was the sibling on a proved path): NEW from its bare bytes
        assert f.block_tree_rows([(0, 0, 3)], statuses_only=True).tolist() == [0] and want_places(f, [(0, [3, 4])])[0] == []
        status, n_new = f.add_multi_anchored([(0, 2)], [3, 4], data_of(slots, [(0, [3, 4])]), None)
        assert status.tolist() == [N, N] and n_new == 2
        bad = slots[0].data[6].copy()
        bad[0] ^= 1                                                                  # ... and wrong bytes are still found out
        assert f.block_tree_rows([(0, 1, 3)], statuses_only=True).tolist() == [0]
        pl, _ = want_places(f, [(0, [6])])
        assert f.add_multi_anchored([(0, 1)], [6], bad, built.block_tree_rows(pl))[0].tolist() == [pkg.FILL_MISMATCH]
        # a block in two proved groups of one call: both are laid out against the session as it stands; NEW, then DUPLICATE
        groups = [(1, [2, 5]), (1, [5, 6]), (1, [2])]
        status, n_new, _ = anchored_multi_add(f, built, slots, groups)
        assert status.tolist() == [N, N, D, N, D] and n_new == 3
        held_to_the_oracle(f, slots, nb)
    finally:
        for h in (f, built):
            h.free()


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_in_its_order_and_a_stale_list(pkg, oracle, sctx):
    C, _ = oracle
    nb, n_slots = 8, 3
    slots = slots_of(C, nb, n_slots)
    cfg, roots = config(pkg, nb, n_slots), np.stack([s.root for s in slots])
    built = build(sctx, cfg, 2)
    f, plain = sctx.fill(cfg, roots), sctx.fill(cfg, roots)
    L = sctx.L
    last_error = lambda: L.cp2_last_error(sctx.h).decode()          # noqa: E731
    p = lambda a: a.ctypes.data if a is not None else None           # noqa: E731
    try:
        f.keep_nodes()
        assert anchored_multi_add(f, built, slots, [(1, [1]), (0, [6])])[1] == 2
        good = [(1, [0, 5]), (2, [6]), (0, [1, 2, 7])]
        g, b = flat(good)
        pl, per = want_places(f, good)
        nodes, data, rows = built.block_tree_rows(pl), data_of(slots, good), len(pl)
        assert rows < sum(len(M.layout(nb, B)) for _, B in good)
        before = state(f, nb, n_slots)
        sets = ((g, b, rows, "data", "must not be NULL"), ([(1, 2), (2, 0), (9, 3)], [0, 8, 1, 1, 7], rows, None, "group 1 holds no block"),
                ([(1, 2), (2, 1), (3, 3)], [8, 0, 6, 1, 1, 7], rows, None, "group 2: slot 3"),
                ([(1, 2), (2, 1), (0, 3)], [5, 5, 6, 1, 8, 7], rows, None, "group 2, request 4: block 8"),
                ([(1, 2), (2, 1), (0, 3)], [0, 5, 6, 2, 2, 7], rows + 1, None, "request 4: block 2 does not ascend"),
                (g, b, rows + 1, None, "n_rows = %d, the groups' want lists against the session as it stands hold %d rows" % (rows + 1, rows)))
        for groups, blocks, n_rows, null, word in sets:
            gg, bb = np.array(groups, dtype=np.uint64), np.array(blocks, dtype=np.uint64)
            status, n_new = np.full(len(bb), 0x5E5E5E5E, dtype=np.uint32), ctypes.c_size_t(0x5E)
            r = L.cp2_fill_add_multi_anchored(f.h, p(gg), len(gg), p(bb), None if null == "data" else p(data), p(nodes), n_rows, p(status), ctypes.byref(n_new))
            assert r == CP2_ERR_INVALID and word in last_error(), (word, last_error())
            assert (status == 0x5E5E5E5E).all() and n_new.value == 0x5E and state(f, nb, n_slots) == before
            if null is None and n_rows == rows:                                      # the want call refuses the same requests, outputs untouched
                li, n, pg = np.full((16, 2), 0x5E, dtype=np.uint64), ctypes.c_size_t(0x5E), np.full(3, 0x5E, dtype=np.uint64)
                assert L.cp2_fill_multiproof_want(f.h, p(gg), len(gg), p(bb), p(li), 16, ctypes.byref(n), p(pg)) == CP2_ERR_INVALID and word in last_error()
                assert (li == 0x5E).all() and n.value == 0x5E and (pg == 0x5E).all()
        # without room the want call states the count and writes no row
        gg, bb = np.array(g, dtype=np.uint64), np.array(b, dtype=np.uint64)
        li, n = np.full((rows, 2), 0x5E, dtype=np.uint64), ctypes.c_size_t(0)
        assert L.cp2_fill_multiproof_want(f.h, p(gg), 3, p(bb), p(li), rows - 1, ctypes.byref(n), None) == CP2_OK and n.value == rows and (li == 0x5E).all()
        assert L.cp2_fill_multiproof_want(f.h, p(gg), 3, p(bb), p(li), rows, ctypes.byref(n), None) == CP2_OK and [(int(l), int(i)) for l, i in li] == [x[1:] for x in pl]
        # a session that keeps no nodes answers the plain layout, and is refused by the add
        li, per0 = plain.multiproof_want(g, b)
        assert [(int(l), int(i)) for l, i in li] == [x for _, B in good for x in M.layout(nb, B)]
        with pytest.raises(pkg.CodexP2Error, match="cp2_fill_add_multi"):
            plain.add_multi_anchored(g, b, data, np.concatenate([np.stack([slots[s].layers[l][i] for l, i in M.layout(nb, B)]) for s, B in good]))
        assert plain.missing()[1] == n_slots * nb
        # an add in between makes the list stale: the same call is refused, with both numbers, and a fresh list lands
        assert anchored_multi_add(f, built, slots, [(1, [4])])[1] == 1
        fresh, _ = want_places(f, good)
        assert len(fresh) < rows
        status, n_new = np.full(len(b), 0x5E5E5E5E, dtype=np.uint32), ctypes.c_size_t(0x5E)
        assert L.cp2_fill_add_multi_anchored(f.h, p(gg), 3, p(bb), p(data), p(nodes), rows, p(status), ctypes.byref(n_new)) == CP2_ERR_INVALID
        assert "n_rows = %d" % rows in last_error() and "hold %d rows" % len(fresh) in last_error() and (status == 0x5E5E5E5E).all()
        assert anchored_multi_add(f, built, slots, good)[0].tolist() == [pkg.FILL_NEW] * len(b)
        n_new = ctypes.c_size_t(0x5E)
        assert L.cp2_fill_add_multi_anchored(f.h, None, 0, None, None, None, 0, None, ctypes.byref(n_new)) == CP2_OK and n_new.value == 0
    finally:
        for h in (f, plain, built):
            h.free()


# ---- 7: with only the root known it is cp2_fill_add_multi -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 2, 8, 32])
def test_with_only_the_root_known_the_state_is_add_multis(pkg, oracle, sctx, nb):
    C, _ = oracle
    n_slots = 3
    slots = slots_of(C, nb, n_slots)
    cfg, roots = config(pkg, nb, n_slots), np.stack([s.root for s in slots])
    f, twin = sctx.fill(cfg, roots), sctx.fill(cfg, roots)
    try:
        f.keep_nodes()
        twin.keep_nodes()
        rng = np.random.default_rng(700 + nb)
        groups = [(s, sorted(int(x) for x in rng.choice(nb, size=int(rng.integers(1, nb + 1)), replace=False))) for s in range(n_slots)]
        g, b = flat(groups)
        li, per = f.multiproof_want(g, b)
        assert [(int(l), int(i)) for l, i in li] == [x for _, B in groups for x in M.layout(nb, B)]
        nodes = [slots[s].layers[l][i] for s, B in groups for l, i in M.layout(nb, B)]
        nodes = np.stack(nodes) if nodes else np.zeros((0, 32), dtype=np.uint8)
        got, want = f.add_multi_anchored(g, b, data_of(slots, groups), nodes), twin.add_multi(g, b, data_of(slots, groups), nodes)
        assert got[0].tolist() == want[0].tolist() and got[1] == want[1] == len(b)
        assert state(f, nb, n_slots) == state(twin, nb, n_slots)
        held_to_the_oracle(f, slots, nb)
    finally:
        f.free()
        twin.free()


def test_block_counts_that_are_no_power_of_two_cannot_be_filled(pkg, sctx):
    """why the calls above stop at powers of two: a session of 3, 5, 9 or 33 blocks of 32 cells is refused when it begins"""
    for nb in (3, 5, 9, 33):
        with pytest.raises(pkg.CodexP2Error, match="not a power of two"):
            sctx.fill(config(pkg, nb, 1), np.zeros((1, 32), dtype=np.uint8))
