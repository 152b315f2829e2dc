"""CPU suite: the models of tests/kernel_models.py against oracle/poseidon2_ref.py, the case plans of tests/test_gpu_kernel_units.py
against what that module says it covers (the k_verify_samples plan against tests/circuit_verdict.py), and the build of
tests/device_check/libkernel_unit.so."""
import os
import subprocess
import time

import numpy as np
import pytest

import circuit_verdict as V
import kernel_models as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")


# ---- the models --------------------------------------------------------------------------------------------------------------------
SMALL_TREES = [(cpb, nblocks) for cpb in (1, 2, 3, 4, 5) for nblocks in (1, 2, 3, 5, 8)]


def small_slot_trees(P, cpb, nblocks, n_slots):
    """Per slot (mini trees, big tree) over small distinct leaves, and the node table laid out as TreeGeom documents it."""
    g = K.tree_geom(cpb, nblocks, cpb * nblocks, n_slots)
    nodes, trees = {}, []
    for s in range(n_slots):
        mini = [P.merkle_tree([1000003 * s + 1009 * b + i + 1 for i in range(cpb)]) for b in range(nblocks)]
        big = P.merkle_tree([t[-1][0] for t in mini])
        trees.append((mini, big))
        for b, t in enumerate(mini):
            for k, layer in enumerate(t[:-1]):
                for i, v in enumerate(layer):
                    nodes[g.boff[k] + (s * nblocks + b) * g.bsz[k] + i] = v
        for k, layer in enumerate(big):
            for i, v in enumerate(layer):
                nodes[g.toff[k] + s * g.tsz[k] + i] = v
    assert sorted(nodes) == list(range(g.total_rows))                 # the layout has no hole and no overlap
    assert len(set(nodes.values())) == len(nodes)                       # a value names its node
    return g, nodes, trees


@pytest.mark.parametrize("cpb,nblocks", SMALL_TREES)
def test_path_rows_model_picks_the_nodes_of_the_merged_padded_proof(oracle, cpb, nblocks):
    _, P = oracle
    g, nodes, trees = small_slot_trees(P, cpb, nblocks, 2)
    depth = K.path_depth(g)
    for s, (mini, big) in enumerate(trees):
        assert nodes[K.root_row(g, s)] == big[-1][0]
        for cell in range(cpb * nblocks):
            bot = P.merkle_proof(mini[cell // cpb], cell % cpb)
            top = P.merkle_proof(big, cell // cpb)
            merged = P.merge_merkle_proofs(bot, top)
            assert merged["leafIndex"] == cell
            want = P.pad_merkle_proof(merged, depth + 3)["merklePath"]
            for md in (depth - 1, depth, depth + 3):
                rows = K.path_rows_model(g, s, cell, md)
                assert [0 if r == K.PAD_ROW else nodes[r] for r in rows] == want[:md], (s, cell, md)
                addr, leaf = K.path_addr_model(g, 4096, s, cell, md)
                assert addr == [0 if r == K.PAD_ROW else 4096 + 32 * r for r in rows]
                assert leaf == 4096 + 32 * (s * g.n_cells + cell)


@pytest.mark.parametrize("n_blocks", (1, 2, 3, 5, 6, 7, 8, 9))
def test_walk_model_is_reconstruct_root(oracle, n_blocks):
    _, P = oracle
    layers = P.merkle_tree([77 * i + 5 for i in range(n_blocks)])
    for b in range(n_blocks):
        proof = P.merkle_proof(layers, b)
        assert K.walk_model(proof["leafValue"], b, n_blocks, proof["merklePath"], P.compress) == P.reconstruct_root(proof) == layers[-1][0]
        for wrong in (b - 1, b + 1):
            if 0 <= wrong < n_blocks:
                assert K.walk_model(proof["leafValue"], wrong, n_blocks, proof["merklePath"], P.compress) == P.reconstruct_root(dict(proof, leafIndex=wrong))


def test_tree_geom_layer_sizes():
    assert K.layer_sizes(1) == [1, 1] and K.layer_sizes(2) == [2, 1] and K.layer_sizes(5) == [5, 3, 2, 1]
    g = K.tree_geom(4, 3, 12, 2)
    assert (g.nb, g.nt, g.bsz, g.tsz) == (3, 3, [4, 2, 1], [3, 2, 1])
    assert g.boff == [0, 24, 36] and g.toff == [36, 42, 46] and g.total_rows == 48       # the block roots are layer 0 of the big trees


def test_scrub_model_by_hand():
    rng = np.random.default_rng(5)
    fresh = rng.integers(0, 256, size=(5 * 3, 32), dtype=np.uint8)
    kept = rng.integers(0, 256, size=(7 * 3, 32), dtype=np.uint8)
    for item in range(3):
        kept[7 * item:7 * item + 3] = fresh[5 * item:5 * item + 3]
    kept[7 * 1 + 2, 31] ^= 0x80              # item 1 row 2: g = 5
    fresh[5 * 2 + 0, 0] ^= 1                 # item 2 row 0: g = 6
    bits, counts = K.scrub_model(fresh, kept, 3, 5, 7, 3)
    assert bits.size == K.SCRUB_TILE // 64 and bits[0] == (1 << 5) | (1 << 6) and not bits[1:].any() and counts.tolist() == [2]
    bits, counts = K.scrub_model(fresh[:4097].repeat(300, axis=0)[:4097], np.zeros((4097, 32), np.uint8), 4097, 4097, 4097, 1)
    assert bits.size == 2 * K.SCRUB_TILE // 64 and counts.tolist() == [4096, 1] and bits[64] == 1 and not bits[65:].any()


def test_batched_compress_is_the_oracles_compress(oracle):
    """The layer test takes its expected rows from the C oracle's permutation over (x, y, key) states, many at a time; that is its compress."""
    C, P = oracle
    rng = np.random.default_rng(11)
    xy = rng.integers(0, 256, size=(8, 2, 32), dtype=np.uint8)
    xy[:, :, 31] &= 0x1F
    for i in range(8):
        key = i % 4
        state = np.concatenate([xy[i, 0], xy[i, 1], C.felt_bytes(key)])
        got = C.permute_batch(state.reshape(1, 96))[0, :32]
        assert np.array_equal(got, C.compress(xy[i, 0], xy[i, 1], key))
        x, y = (int.from_bytes(xy[i, j].tobytes(), "little") for j in (0, 1))
        assert int.from_bytes(got.tobytes(), "little") == P.compress(x, y, key)


# ---- the plans ---------------------------------------------------------------------------------------------------------------------
def test_scrub_plan():
    cases = K.scrub_plan()
    dense = [c for c in cases if c.fstride == c.rows == c.kstride]
    assert {c.rows * c.n_items for c in dense if c.n_items == 1} == set(K.SCRUB_TOTALS)
    assert {c.rows * c.n_items for c in dense if c.n_items > 1} >= {63, 64, 65, 255, 256, 4095, 4096, 4097, 8192}
    assert {(c.rows, c.fstride, c.kstride) for c in cases if not (c.fstride == c.rows == c.kstride)} == {(1, 1, 2), (3, 5, 7), (4097, 4100, 4097), (64, 64, 65)}
    assert {c.n_items for c in cases if (c.rows, c.kstride) == (1, 2)} == set(K.SCRUB_TOTALS)
    tile = K.SCRUB_TILE
    for layout in K.SCRUB_STRIDED:                                      # each strided layout crosses a tile seam, three of them end in a partial wave
        totals = {c.rows * c.n_items for c in cases if (c.rows, c.fstride, c.kstride) == layout}
        assert any(t > tile for t in totals) and (layout[0] == 64 or any(t % 64 for t in totals)), layout
    by_layout = {}
    for c in cases:
        by_layout.setdefault((c.rows, c.fstride, c.kstride, c.n_items), set()).add(c.planted)
    for (rows, fs, ks, n), planted in by_layout.items():
        want = {"none", "all", "row0", "last", "1%"} | ({"63/64"} if rows * n > 63 else set()) | ({"4095/4096"} if rows * n > 4095 else set())
        assert planted == want, (rows, fs, ks, n)
    used, small, sides = set(), set(), set()
    for c in cases:
        rows = K.scrub_planted_rows(c)
        bit, side = K.scrub_planted_bits(c)
        assert rows.size == bit.size == side.size and np.unique(rows).size == rows.size and (rows.size == 0 or rows.max() < c.rows * c.n_items)
        used |= set(bit.tolist())
        if c.planted in ("row0", "last", "63/64", "4095/4096"):         # one or two rows: a dropped XOR term cannot hide behind another row
            small |= set(bit.tolist())
        sides |= set(side.tolist())
    assert used == set(range(256)) and sides == {0, 1}
    assert {b // 32 for b in small} == set(range(8)) and len(small) >= 128
    assert [c.no for c in cases] == list(range(len(cases)))


def test_repair_plan():
    cases = K.repair_plan()
    assert {(c.n, c.kind, c.tail) for c in cases} == {(n, k, t) for n in (1, 63, 64, 65, 257, 1000) for k in ("permutation", "repeats") for t in ("plain", "last", "bound")}
    words = set()
    for c in cases:
        flips = K.repair_flips(c)
        assert all(0 <= i < c.n for i, _ in flips) and not (c.tail == "bound" and any(i == c.n - 1 for i, _ in flips))
        words |= {bit // 32 for _, bit in flips}
    assert words == set(range(8))
    assert {bit for c in cases for _, bit in K.repair_flips(c)} == set(range(256))
    assert any(K.repair_flips(c) for c in cases if c.n == 1) and any(not K.repair_flips(c) for c in cases if c.n == 1)


def test_sample_plan():
    cases = K.sample_plan()
    assert {(c.cpb, c.nblocks) for c in cases if c.n_cells == c.cpb * c.nblocks} == {(a, b) for a in (1, 2, 4, 32) for b in (1, 2, 64, 1 << 15)}
    odd = {(c.cpb, c.nblocks, c.n_cells) for c in cases if c.n_cells != c.cpb * c.nblocks}
    assert odd and all(n & (n - 1) == 0 and n < a * b for a, b, n in odd)
    assert any(any(m % 2 for m in K.layer_sizes(b)[:-1]) for a, b, n in odd) and any(any(m % 2 and m > 1 for m in K.layer_sizes(a)[:-1]) for a, b, n in odd)
    assert {c.ns for c in cases} == {1, 5, 100} and {c.ns * c.n_items for c in cases} >= {1, 255, 256, 257}
    assert all(c.n_slots == 3 for c in cases if c.form == "list" or c.n_items <= 3)
    depth = {(c.cpb, c.nblocks): K.path_depth(K.tree_geom(c.cpb, c.nblocks, c.cpb * c.nblocks, 3)) for c in cases}
    assert min(depth.values()) > 1
    for geo in depth:
        mine = [c for c in cases if (c.cpb, c.nblocks) == geo]
        assert {c.md - depth[geo] for c in mine} == {-1, 0, 3} and {c.form for c in mine} == {"list", "range"}
        assert {(c.ns, c.n_items) for c in mine} >= set(K.SAMPLE_LANES)
    for lanes in K.SAMPLE_LANES:
        mine = [c for c in cases if (c.ns, c.n_items) == lanes]
        assert {c.md - depth[(c.cpb, c.nblocks)] for c in mine} == {-1, 0, 3}
        assert {c.form for c in mine if c.n_slots == 3} == ({"list", "range"} if lanes[1] <= 3 else {"list"})
    big_range = [c for c in cases if c.form == "range" and c.n_items > 3]
    assert {c.n_items for c in big_range} == {255, 256, 257} and all(c.nblocks <= 64 and c.slot0 + c.n_items == c.n_slots for c in big_range)
    assert all(c.slot0 + c.n_items <= c.n_slots for c in cases if c.form == "range")
    assert max(K.tree_geom(c.cpb, c.nblocks, c.n_cells, c.n_slots).total_rows for c in cases) * 32 <= 256 << 20     # what the node buffer takes
    cp = K.compact_plan()
    assert {n for n, _ in cp} == {1 << 31, 1 << 32, 1 << 33, 1 << 40, 1 << 63}
    for n in K.COMPACT_N_CELLS:
        cpbs = {c for m, c in cp if m == n}
        assert any(c % 2 == 1 and c > 1 for c in cpbs) and any(c > 1 and c & (c - 1) == 0 for c in cpbs)
    assert K.reaches_high(1 << 32, 1 << 33) and not K.reaches_high((1 << 32) - 1, 1 << 33)
    assert K.reaches_high(1 << 31, 1 << 32) and not K.reaches_high((1 << 31) - 1, 1 << 32) and K.reaches_high(1 << 30, 1 << 31)


def test_gather_plans():
    rows = K.gather_rows_plan()
    assert {w for w, _ in rows} == {4, 32, 36, 2048}
    for w in K.GATHER_ROWS_WIDTHS:
        assert any(n * (w // 4) > K.GRID_WORDS for ww, n in rows if ww == w) and any(n * (w // 4) <= 512 for ww, n in rows if ww == w)
    assert (32, 131073) in rows
    addr = K.gather_addr_plan()
    assert {(w, a) for w, a, _ in addr} >= {(w, a) for w in (1, 3, 31, 32, 33, 100, 2048, 2050) for a in (0, 1, 2)}
    over = {K.gather_addr_wordwise(w, a) for w, a, n in addr if n * (w // 4 if K.gather_addr_wordwise(w, a) else w) > K.GRID_WORDS}
    assert over == {True, False}
    assert max(n * w for w, a, n in addr) <= 8 << 20 and max(n * w for w, n in rows) <= 8 << 20


def test_layer_plan():
    plan = K.layer_plan()
    assert {(m, s, b) for m, s, b, _, _ in plan} == {(m, s, b) for m in (1, 2, 3, 4, 5, 255, 256, 257, 511, 513) for s in (1, 3, 257) for b in (0, 1)}
    for (m, s, b) in {(m, s, b) for m, s, b, _, _ in plan}:
        gaps = {(i - m, o - (m + 1) // 2) for mm, ss, bb, i, o in plan if (mm, ss, bb) == (m, s, b)}
        assert gaps >= {(0, 0), (1, 1), (5, 5)}
    assert any(s == 257 and m % 2 == 1 and i > m and o > (m + 1) // 2 for m, s, b, i, o in plan)        # many segments, an odd tail in each, gaps


def test_fake_cell_of_walks_the_units_of_a_dataset_in_order():
    """A dataset's cells listed unit by unit -- units_per_slot units of cells_per_slot cells to a slot -- from unit first_unit on are what
    fake_cell_of gives for g = 0, 1, ...; without units the same with one unit to a slot, first_unit unread."""
    for cps in (1, 3, 64):
        for ups in (1, 2, 4):
            units = [(u // ups, (u % ups) * cps + i) for u in range(12) for i in range(cps)]
            for fu in (0, 5):
                start = fu if ups > 1 else 0
                assert [K.fake_cell_of(g, cps, ups, fu) for g in range(6 * cps)] == units[start * cps:(start + 6) * cps]
    # cells_per_slot == 0: every cell lies in the batch's unit 0, cell g of it
    assert [K.fake_cell_of(g, 0, ups, 5) for g in (0, 9, 1 << 40) for ups in (1, 2, 4)] == [(s, g) for g in (0, 9, 1 << 40) for s in (0, 2, 1)]


def test_fake_single_plan():
    plan = K.fake_single_plan()
    assert 200 <= len(plan) <= 400 and [c.no for c in plan] == list(range(len(plan)))
    shapes = {(c.n, c.cell_size, c.offset) for c in plan}
    assert shapes == {(n, cs, a) for n in (1, 63, 64, 65, 257) for cs in (1, 127, 128, 2048, 2049) for a in (0, 4)}
    for wide in (True, False):                                   # every mapping through both write-outs
        got = {(c.cells_per_slot, c.first, c.units_per_slot, c.first_unit, c.listed) for c in plan if K.fake_is_wide(c.cell_size, c.offset) == wide}
        assert got == {(cps, f, ups, fu, ls) for cps in (0, 1, 3, 64) for f in (0, 7, (1 << 32) - 2) for ups in (1, 2, 4) for fu in (0, 5)
                       for ls in (False, True)}
    assert {(c.seed0, c.cells_per_slot) for c in plan} == {(s, cps) for s in K.FAKE_GROUP_SEEDS for cps in (0, 1, 3, 64)}
    wraps = edges = unit_edges = 0
    for c in plan:
        cells = K.fake_single_cells(c)
        where = [K.fake_cell_of(g, c.cells_per_slot, c.units_per_slot, c.first_unit) for g in cells]
        assert len(cells) == c.n and all(0 <= g < (1 << 64) for g in cells)
        if c.listed and c.n >= 3:                                # not monotone, a repeat, and (more than one slot) a jump back and forth
            assert cells[0] > cells[1] < cells[2] and cells[0] == cells[2]
            assert c.cells_per_slot == 0 or where[0][0] != where[1][0]
        if not c.listed and c.cells_per_slot and c.n >= 63:      # a run crosses a slot edge inside its first wave
            crosses = len({s for s, _ in where[:64]}) > 1
            assert crosses or c.cells_per_slot == 64
            edges += crosses
            unit_edges += c.units_per_slot > 1 and any(a[0] == b[0] and b[1] % c.cells_per_slot == 0 for a, b in zip(where[:64], where[1:64]))
        wraps += any(c.seed0 + 1001 * s >= (1 << 64) for s, _ in where)
    assert wraps >= 10 and edges >= 50 and unit_edges >= 20


def test_fake_many_plan():
    plan = K.fake_many_plan()
    assert set(plan) == {(p, n, c, a) for p in (1, 3, 100) for n in (1, 63, 64, 65, 257, 301) for c in (1, 127, 128, 2048, 2049) for a in (0, 4, 1)}
    assert any(n % p for p, n, _, _ in plan if p > 1)                                                      # a partial last group
    groups = [K.fake_group(g) for g in range(301)]
    assert len(set(groups)) == 301 and len({s for s, _ in groups}) == 301
    assert any(f < (1 << 32) <= f + 99 for _, f in groups) and any(f < (1 << 32) <= f + 2 for _, f in groups)
    assert all(0 <= s < (1 << 64) and f + 100 < (1 << 64) for s, f in groups)


def test_walk_plan():
    assert K.WALK_N_BLOCKS == tuple(range(1, 18)) + (31, 32, 33)
    for n in K.WALK_N_BLOCKS:
        depth = len(K.layer_sizes(n)) - 1
        reqs = K.walk_plan(n)
        for b in range(n):
            mine = [r for r in reqs if r.block == b]
            assert {r.root for r in mine if r.kind == "true"} == {0, 1}
            assert sorted(r.level for r in mine if r.kind == "sibling") == list(range(depth))
            assert sum(r.kind == "fresh" for r in mine) == 1 and sum(r.kind == "other root" for r in mine) == 1
            assert {r.index for r in mine if r.kind == "neighbour"} == {x for x in (b - 1, b + 1) if 0 <= x < n}
            assert all(r.index == b for r in mine if r.kind != "neighbour")


# ---- k_verify_samples: the builder, the packer, the plan ----------------------------------------------------------------------------------
def _log2(n):
    return n.bit_length() - 1


def _bases(launch):
    return [it for it in launch.items if it.kind == "base"]


def _indices(it):
    return [V.sample_index(it.d, None, c) for c in range(len(it.d["cellData"]))]


def test_verify_plan_agrees_with_the_circuit(capsys):
    """Every input the plan calls accepted gets (0, [1] * ns) from circuit_verdict.verdict, every expectation a mutant's tag states is
    the model's, and the model's own time over the whole plan stays bounded (its hashing memoised)."""
    t0 = time.time()
    plan = K.verify_plan()
    t_build = time.time() - t0
    kinds, open_ = {}, 0
    with K.memoised_hashing():
        for launch in plan:
            cfg = K.verify_cfg(launch.geom)
            for it in launch.items:
                kinds[it.kind] = kinds.get(it.kind, 0) + 1
                got = K.verify_expected(it.d, launch.geom)
                assert len(got) == launch.ns + 1 == len(it.d["cellData"]) + 1
                if it.kind in ("base", "top", "top past accepted", "edge base"):
                    assert V.verdict(it.d, cfg) == (0, [1] * launch.ns), (launch.name, it.tag)
                    assert it.expect == (1,) * (launch.ns + 1)
                if it.expect is None:
                    open_ += 1
                else:
                    assert it.expect == got, (launch.name, it.tag, it.expect, got)
                if it.kind in ("cell", "path read", "proof read", "dataSetRoot"):            # exactly its own byte, or the top byte
                    assert it.expect.count(0) == 1, it.tag
                if it.kind in ("path above", "proof above", "cell, not compared"):
                    assert it.expect == (1,) * (launch.ns + 1), it.tag
                if it.kind in ("slotRoot", "entropy", "top past"):
                    assert it.expect is None
                if it.kind == "refused":
                    assert got == (0,) * (launch.ns + 1) == it.expect
    t_all = time.time() - t0
    with capsys.disabled():
        print("\n[kernel units] verify plan: %d launches, %d inputs, %d lanes; %d expectations stated by the plan, %d the model's alone; "
              "built in %.1f s, model %.1f s" % (len(plan), K.verify_plan_cases(), sum(len(x.items) * (x.ns + 1) for x in plan),
                                                K.verify_plan_cases() - open_, open_, t_build, t_all - t_build))
        print("[kernel units] verify plan by kind: %s" % ", ".join("%s %d" % kv for kv in sorted(kinds.items())))
    assert t_all < 60


def test_verify_plan_geometries_and_branches():
    launches = [K.verify_geometry_launch(gi) for gi in range(len(K.VERIFY_GEOMS))]
    assert [x.geom for x in launches] == [(3, 1, 0, 1), (2, 2, 1, 2), (5, 2, 3, 3), (6, 3, 5, 4), (8, 2, 4, 67)]
    for launch in launches:
        md, bd, m, nf = launch.geom
        bases = _bases(launch)
        assert 2 <= launch.ns <= 5 and launch.items[:len(bases)] == bases
        ks = [_log2(it.d["nCellsPerSlot"]) for it in bases]
        assert set(ks) == set(range(1, md + 1))                                          # every k, in one launch
        first = ks[:md]
        assert all(a != b for a, b in zip(first, first[1:]))                              # neighbouring inputs differ in k
        pairs = {(it.d["nSlotsPerDataSet"], it.d["slotIndex"]) for it in bases}
        assert len(pairs) >= min(3, sum(n for n in range(1, (1 << m) + 1)))              # m = 0 has the one pair only
        assert {n for n, _ in pairs} >= {1, 1 << m}
        assert all(len(r) == nf for it in launch.items for r in it.d["cellData"])
        # index extremes, by the model
        at_md = [i for it in bases if _log2(it.d["nCellsPerSlot"]) == md for i in _indices(it)]
        assert 0 in at_md and (1 << md) - 1 in at_md, launch.name
        if md > bd:
            cpb = 1 << bd
            assert any(i & (cpb - 1) == cpb - 1 and i >> bd != (1 << (md - bd)) - 1 for i in at_md), launch.name
    by_geom = {x.geom: _bases(x) for x in launches}
    # k < bd: the middle walk's one compression takes path index bd, everything between is padding
    for geom in ((2, 2, 1, 2), (5, 2, 3, 3), (6, 3, 5, 4), (8, 2, 4, 67)):
        md, bd, m, nf = geom
        low = [it for it in by_geom[geom] if _log2(it.d["nCellsPerSlot"]) < bd]
        assert low
        for it in low:
            k = _log2(it.d["nCellsPerSlot"])
            for path in it.d["merklePaths"]:
                assert all(path[:k]) and not any(path[k:bd]) and not any(path[bd + 1:]) and (md == bd or path[bd] != 0)
    # md == bd: the sample compares 0 with slotRoot
    assert all(it.d["slotRoot"] == 0 for it in by_geom[(2, 2, 1, 2)]) and all(it.d["slotRoot"] != 0 for it in by_geom[(5, 2, 3, 3)])
    # m == 0: the top lane compares 0 with dataSetRoot
    assert all(it.d["dataSetRoot"] == 0 and it.d["slotProof"] == [] for it in by_geom[(3, 1, 0, 1)])
    assert {g[3] for g in by_geom} == {1, 2, 3, 4, 67}                                   # the sponge's 1 at j == nf and at j + 1 == nf
    assert (8, 2, 4, 67) in by_geom and K.verify_cfg((8, 2, 4, 67))["cellSize"] == 2048   # the product's cell


def test_verify_plan_top_walk_is_exhaustive():
    assert K.VERIFY_TOP_M == (0, 1, 3, 5)
    launches = {(m, 0): K.verify_top_launch(m, 0) for m in K.VERIFY_TOP_M}
    launches[(3, 2)] = K.verify_top_launch(3, 2)
    for (m, ns), launch in launches.items():
        assert launch.ns == ns and launch.geom[2] == m
        seen = {}
        for it in launch.items:
            seen.setdefault((it.d["nSlotsPerDataSet"], it.d["slotIndex"]), []).append(it.kind)
            assert len(it.d["cellData"]) == ns
        assert set(seen) == {(n, si) for n in range(1, (1 << m) + 1) for si in range(1 << m)}
        for (n, si), kinds in seen.items():
            assert kinds == (["top"] if si < n else ["top past", "top past accepted"]), (m, n, si)
        # the odd-node key (+2) below the highest level that is read: slotIndex the last of an odd nSlots, and the layers above it
        if m >= 3:
            assert any(n % 2 == 1 and si == n - 1 and n > 2 for (n, si) in seen)
    plan = K.verify_plan()
    assert [x for x in plan if x.ns == 0 and x.name.startswith("top walk")] == [launches[(m, 0)] for m in K.VERIFY_TOP_M]
    assert launches[(3, 2)] in plan


def test_verify_plan_mutates_every_felt():
    for gi, geom in enumerate(K.VERIFY_GEOMS):
        md, bd, m, nf = geom
        launch = K.verify_geometry_launch(gi)
        felts = set(range(nf)) if nf != 67 else {0, 1, 32, 65, 66}
        levels_read = set()
        for base in _bases(launch):
            mine = [it for it in launch.items if it.kind != "base" and it.tag.startswith(base.tag + "; ")]
            changed = set()
            for it in mine:
                diff = [(key, base.d[key], it.d[key]) for key in V.KEYS if base.d[key] != it.d[key]]
                assert len(diff) == 1
                key, a, b = diff[0]
                if key in ("cellData", "merklePaths"):
                    at = [(s, j) for s in range(launch.ns) for j in range(len(a[s])) if a[s][j] != b[s][j]]
                    assert len(at) == 1 and b[at[0][0]][at[0][1]] == (a[at[0][0]][at[0][1]] + 1) % K.R_MOD
                    changed.add((key,) + at[0])
                    if it.kind == "path read":
                        levels_read.add(at[0][1])
                elif key == "slotProof":
                    at = [j for j in range(m) if a[j] != b[j]]
                    assert len(at) == 1 and b[at[0]] == (a[at[0]] + 1) % K.R_MOD
                    changed.add((key, at[0]))
                else:
                    assert b == (a + 1) % K.R_MOD
                    changed.add((key,))
            want = {("cellData", s, j) for s in range(launch.ns) for j in felts} | {("merklePaths", s, j) for s in range(launch.ns) for j in range(md)}
            want |= {("slotProof", j) for j in range(m)} | {("dataSetRoot",), ("slotRoot",), ("entropy",)}
            assert changed == want and len(mine) == len(want), (launch.name, base.tag)
        kinds = {it.kind for it in launch.items}
        if md > bd:
            assert levels_read == set(range(md)) and {"cell", "path read", "path above"} <= kinds
        else:
            assert not levels_read and "cell, not compared" in kinds and "cell" not in kinds
        assert kinds >= ({"proof read", "proof above"} if m > 1 else {"proof read"} if m else set())
        # mutants travel in their base's launch, after the bases, base after base in turn
        n_bases = len(_bases(launch))
        tail = launch.items[n_bases:2 * n_bases]
        assert len({it.tag.split("; ")[0] for it in tail}) == n_bases


def test_verify_plan_field_edges_layouts_and_refused_shapes():
    edge = K.verify_edge_launch()
    bases = [it for it in edge.items if it.kind == "edge base"]
    md, bd, m, nf = edge.geom
    assert {_log2(it.d["nCellsPerSlot"]) - bd for it in bases} == {-1, 0, 2}
    assert {v for it in bases for r in it.d["cellData"] for v in r} == set(K.VERIFY_EDGES) == {0, 1, K.R_MOD - 1, 1 << 253, (1 << 29) - 1, 1 << 29, 1 << 58, 1 << 232}
    assert {v for it in bases for v in K.verify_free_siblings(it.d, edge.geom)} == set(K.VERIFY_EDGES)
    mutated = bases[:3]
    assert {_log2(it.d["nCellsPerSlot"]) - bd for it in mutated} == {-1, 0, 2}
    for base in mutated:
        for key in ("dataSetRoot", "slotRoot"):
            mine = [it for it in edge.items if it.kind == "edge " + key and it.tag.startswith(base.tag + "; ")]
            assert {it.d[key] for it in mine} == {base.d[key] + 1, base.d[key] - 1, base.d[key] ^ (1 << 253)}
            assert all(it.expect[-1] == 0 for it in mine) and all(it.expect == (0,) * (edge.ns + 1) for it in mine if key == "slotRoot")
    # nothing at or above r is fed where the kernel reads it
    for launch in K.verify_plan():
        cfg = K.verify_cfg(launch.geom)
        for it in launch.items:
            if V.shape_ok(it.d, cfg):
                felts = [it.d["dataSetRoot"], it.d["entropy"], it.d["slotRoot"]] + it.d["slotProof"] + [v for r in it.d["cellData"] + it.d["merklePaths"] for v in r]
                assert all(0 <= v < K.R_MOD for v in felts), (launch.name, it.tag)
    layouts = K.verify_layout_launches()
    sizes = [(len(x.items), x.ns) for x in layouts]
    assert {n * ns % 64 for n, ns in sizes} >= {0, 1, 63}
    assert any(n * ns and n * ns % 256 == 0 for n, ns in sizes)
    assert {n * (ns + 1) for n, ns in sizes} >= {1, 255, 256, 257, 513}
    for launch in layouts:
        n, ns = len(launch.items), launch.ns
        if n > 1:
            assert launch.items[0].expect[-1] == 0 and (ns == 0 or launch.items[-1].expect[ns - 1] == 0)      # both sides of lane n * ns
            assert len({it.d["nCellsPerSlot"] for it in launch.items}) == 3 and len({it.d["nSlotsPerDataSet"] for it in launch.items}) == 3
    refused = K.verify_refused_launch()
    cfg = K.verify_cfg(refused.geom)
    ff = K.VERIFY_UNWRITTEN
    assert ff.to_bytes(32, "little") == b"\xff" * 32
    assert [it.kind == "refused" for it in refused.items] == [False, True] * (len(refused.items) // 2)
    assert {it.d["nCellsPerSlot"] for it in refused.items if it.kind == "refused"} == {0, 3}
    for it in refused.items:
        if it.kind == "refused":
            assert not V.shape_ok(it.d, cfg) and set(it.d["slotProof"]) == {ff} and {v for r in it.d["cellData"] + it.d["merklePaths"] for v in r} == {ff}
            assert it.expect == (0,) * (refused.ns + 1)
        else:
            assert V.shape_ok(it.d, cfg)
    assert {it.kind for it in refused.items} >= {"base", "cell", "dataSetRoot", "refused"}


def test_verify_pack_round_trips():
    """The arrays hold the dicts, laid out as the comment above VerifyGeom says; prm[3] is circuit_verdict.shape_ok."""
    for launch in K.verify_plan():
        md, bd, m, nf = launch.geom
        dicts = [it.d for it in launch.items]
        prm, heads, cells, paths = K.verify_pack(dicts, launch.geom)
        n, ns = len(dicts), launch.ns
        assert prm.dtype == np.uint64 and prm.shape == (n, 4)
        assert all(a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"] for a in (heads, cells, paths))
        assert heads.shape == (n, 3 + m, 32) and cells.shape == (n, ns, nf, 32) and paths.shape == (n, ns, md, 32)
        back, shape = K.verify_unpack(prm, heads, cells, paths)
        assert back == dicts
        assert shape == [1 if V.shape_ok(d, K.verify_cfg(launch.geom)) else 0 for d in dicts]
    launch = K.verify_geometry_launch(2)
    d = launch.items[1].d
    prm, heads, cells, paths = K.verify_pack([launch.items[0].d, d], launch.geom)
    assert prm[1].tolist() == [d["nCellsPerSlot"], d["nSlotsPerDataSet"], d["slotIndex"], 1]
    flat = heads.reshape(-1)
    at = (3 + 3) * 32                                                                       # input 1: after input 0's 3 + m felts
    assert [int.from_bytes(flat[at + 32 * i:at + 32 * i + 32].tobytes(), "little") for i in range(6)] == [d["dataSetRoot"], d["entropy"], d["slotRoot"]] + d["slotProof"]
    assert int.from_bytes(cells.reshape(-1)[((1 * 3 + 2) * 3 + 1) * 32:][:32].tobytes(), "little") == d["cellData"][2][1]
    assert int.from_bytes(paths.reshape(-1)[((1 * 3 + 2) * 5 + 4) * 32:][:32].tobytes(), "little") == d["merklePaths"][2][4]
    e = K.verify_pack([], launch.geom)
    assert e[0].shape == (0, 4) and e[1].shape == (0, 6, 32)


def test_verify_build_is_accepted_where_the_producer_has_no_counterpart():
    """The builder alone, at the placements it makes by hand: k < bd, md == bd, m == 0; and with the oracle's hashing as it is."""
    for (md, bd, m, nf, n_cells, n_slots, si) in ((5, 3, 2, 3, 2, 3, 2), (5, 3, 2, 2, 4, 1, 0), (3, 3, 1, 1, 8, 2, 1), (3, 3, 0, 4, 2, 1, 0), (4, 1, 0, 2, 16, 1, 0)):
        d = K.verify_build(md, bd, m, nf, 3, n_cells, n_slots, si, 99, K.verify_values("alone", md, bd, m, nf))
        assert V.verdict(d, K.verify_cfg((md, bd, m, nf)) if nf in K.VERIFY_CELL_SIZE else None) == (0, [1, 1, 1])
        assert (d["slotRoot"] == 0) == (md == bd) and (d["dataSetRoot"] == 0) == (m == 0)


# ---- the check library -------------------------------------------------------------------------------------------------------------
def dynamic_symbols(path, defined):
    out = subprocess.check_output(["nm", "-D", "--defined-only" if defined else "--undefined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_check_library_builds_and_forwards_to_the_product(pkg):
    """make builds it (hipcc for gfx950, the product's flags); it defines the ku_ forwarders and takes every launcher from
    libcodex_p2.so, whose code objects are therefore the ones that run."""
    subprocess.check_call(["make", "-C", PKG_DIR, "../tests/device_check/libkernel_unit.so"], stdout=subprocess.DEVNULL)
    lib = os.path.join(ROOT, "tests", "device_check", "libkernel_unit.so")
    launchers = ("scrub_compare", "repair_compare", "sample_paths", "sample_many", "gather_rows", "gather_addr", "gen_fake_cells", "gen_fake_cells_many",
                 "compress_layer", "block_path_roots", "block_path_commit", "verify_samples")
    mine, wanted, product = dynamic_symbols(lib, True), dynamic_symbols(lib, False), dynamic_symbols(pkg.LIB_PATH, True)
    assert {"ku_" + n for n in launchers} | {"ku_sizeof_tree_geom", "ku_sizeof_many_req", "ku_sizeof_verify_geom", "ku_scrub_tile"} <= mine
    for n in launchers:
        sym = [s for s in wanted if s.startswith("_ZN4cp2k%d%s" % (len("launch_" + n), "launch_" + n))]
        assert len(sym) == 1 and sym[0] in product, n
    assert not [s for s in mine if "cp2k" in s or s.startswith("cp2_")]
    needed = subprocess.check_output(["readelf", "-d", lib], text=True)
    assert "libcodex_p2.so." in needed and "$ORIGIN/../../codex-storage-proofs-circuits_amd" in needed
