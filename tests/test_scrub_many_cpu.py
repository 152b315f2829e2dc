"""CPU suite: the references behind cp2_datasets_scrub_many (tests/scrub_many_models.py) and the host side of its name table.

The numpy model of k_scrub_compare_many against kernel_models.scrub_model on every case of kernel_models.scrub_plan() (a contiguous
address table is the strided kernel), then with the items scattered; the class grouping and the merge of the classes' reports against
brute force; and tests/host_check/fill_names_check.cpp -- turns filled from a name table over real files on several threads -- built
with AddressSanitizer + UBSan and again with ThreadSanitizer.  No GPU."""
import os
import random
import subprocess

import numpy as np

import kernel_models as K
import scrub_many_models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_arrays(c):
    """fresh and kept of a case of the plan, as tests/test_gpu_kernel_units.py makes them"""
    rng = np.random.default_rng([0x5C2B, c.no])
    total = c.rows * c.n_items
    fresh = rng.integers(0, 256, size=(c.n_items * c.fstride, 32), dtype=np.uint8)
    kept = rng.integers(0, 256, size=(c.n_items * c.kstride, 32), dtype=np.uint8)
    item, r = np.divmod(np.arange(total, dtype=np.int64), c.rows)
    fo, ko = item * c.fstride + r, item * c.kstride + r
    kept[ko] = fresh[fo]
    rows = K.scrub_planted_rows(c)
    bit, side = K.scrub_planted_bits(c)
    mask = (1 << (bit % 8)).astype(np.uint8)
    f, k = side == 0, side == 1
    fresh[fo[rows[f]], bit[f] // 8] ^= mask[f]
    kept[ko[rows[k]], bit[k] // 8] ^= mask[k]
    return fresh, kept


def test_contiguous_address_table_is_the_strided_kernel_on_every_case_of_the_plan():
    plan = K.scrub_plan()
    assert len(plan) > 300
    for c in plan:
        fresh, kept = plan_arrays(c)
        want = K.scrub_model(fresh, kept, c.rows, c.fstride, c.kstride, c.n_items)
        addr = np.arange(c.n_items, dtype=np.int64) * c.kstride * 32
        got = M.scrub_many_model(fresh, c.fstride, kept.reshape(-1), addr, c.rows, c.n_items)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), c
        assert int(got[1].sum()) == K.scrub_planted_rows(c).size


def test_scattered_items_by_hand_and_against_a_row_loop():
    # three items of two rows at offsets 96, 0 and 200 (a gap of 8 bytes before it): one differing row in items 0 and 2
    fresh = np.arange(6 * 32, dtype=np.uint8).reshape(6, 32)
    mem = np.full(300, 0xEE, dtype=np.uint8)
    for item, at in enumerate((96, 0, 200)):
        mem[at:at + 64] = fresh[2 * item:2 * item + 2].reshape(-1)
    mem[96 + 32 + 31] ^= 1                                        # item 0 row 1, its last byte
    mem[200] ^= 0x80                                              # item 2 row 0, its first byte
    bits, counts = M.scrub_many_model(fresh, 2, mem, [96, 0, 200], 2, 3)
    assert bits.size == K.SCRUB_TILE // 64 and int(bits[0]) == 0b010010 and not bits[1:].any() and counts.tolist() == [2]
    assert M.decode(bits, 2, 3) == [(0, 1), (2, 0)]
    # random: shuffled items, fstride > rows, against a loop over the rows
    rng = np.random.default_rng(7)
    for rows, fstride, n_items in ((1, 1, 70), (3, 5, 1400), (16, 16, 257), (64, 70, 65)):
        fresh = rng.integers(0, 256, size=(n_items * fstride, 32), dtype=np.uint8)
        order = rng.permutation(n_items)
        gap = 48
        addr = np.zeros(n_items, dtype=np.int64)
        mem = rng.integers(0, 256, size=n_items * (rows * 32 + gap), dtype=np.uint8)
        for place, item in enumerate(order):
            addr[item] = place * (rows * 32 + gap)
            mem[addr[item]:addr[item] + rows * 32] = fresh[item * fstride:item * fstride + rows].reshape(-1)
        planted = sorted(set(int(x) for x in rng.integers(0, rows * n_items, size=9)) | {0, rows * n_items - 1})
        for g in planted:
            mem[addr[g // rows] + (g % rows) * 32 + int(rng.integers(0, 32))] ^= 0x10
        bits, counts = M.scrub_many_model(fresh, fstride, mem, addr, rows, n_items)
        assert M.decode(bits, rows, n_items) == [(g // rows, g % rows) for g in planted]
        want_counts = np.bincount(np.array(planted) // K.SCRUB_TILE, minlength=K.scrub_groups(rows * n_items))
        assert counts.tolist() == want_counts.tolist()


def random_requests(rnd, n):
    geoms = [(64, 256, 64), (64, 256, 128), (2048, 65536, 4096)]
    out = []
    for _ in range(n):
        cs, bs, nc = rnd.choice(geoms)
        out.append(M.Request(cs, bs, nc, rnd.choice((0, 1, 2)), rnd.random() < 0.85, rnd.randrange(0, 9), rnd.choice((1, 1, 1, 2, 6))))
    return out


def test_class_grouping_against_brute_force():
    rnd = random.Random(11)
    for n in (0, 1, 2, 7, 40):
        reqs = random_requests(rnd, n)
        classes, fake = M.group_classes(reqs)
        assert fake == [i for i, q in enumerate(reqs) if not q.from_file]
        # every (request, slot) of a file-sourced request in exactly one class, the class of its key; items in request order
        seen = []
        for cls in classes:
            assert cls.items and cls.items == sorted(cls.items)
            for i, s in cls.items:
                q = reqs[i]
                assert q.from_file and (q.cell_size, q.block_size, q.n_cells, q.level) == cls.key
            seen += cls.items
        want = [(i, q.first_slot + s) for i, q in enumerate(reqs) if q.from_file for s in range(q.n_local)]
        assert sorted(seen) == sorted(want) and len(seen) == len(want)
        assert len({cls.key for cls in classes}) == len(classes)
    # one geometry each: every class is one request -- the loop
    reqs = [M.Request(64, 256, 64 << i, 1, True, i, 1) for i in range(5)]
    classes, _ = M.group_classes(reqs)
    assert [cls.items for cls in classes] == [[(i, i)] for i in range(5)]
    # a dataset listed twice: two requests, two runs of items
    classes, _ = M.group_classes([reqs[0], reqs[1], reqs[0]])
    assert classes[0].items == [(0, 0), (2, 0)] and classes[1].items == [(1, 1)]


def test_merge_order_cap_and_complete_counts_against_brute_force():
    rnd = random.Random(12)
    for trial in range(60):
        reqs = random_requests(rnd, rnd.choice((1, 3, 12)))
        classes, _ = M.group_classes(reqs)
        rows_of = {0: 1, 1: 16, 2: 64}
        item_rows = []
        for cls in classes:
            item_rows.append([sorted(rnd.sample(range(rows_of[cls.key[3]]), rnd.choice((0, 0, 1, min(3, rows_of[cls.key[3]])))))
                              for _ in cls.items])
        every = sorted((i, s, r) for cls, per in zip(classes, item_rows) for (i, s), rs in zip(cls.items, per) for r in rs)
        brute_counts = [sum(1 for t in every if t[0] == i) for i in range(len(reqs))]
        for cap in (0, 1, 2, len(every) // 2, len(every), len(every) + 5):
            reports = [M.class_report(cls, per, cap) for cls, per in zip(classes, item_rows)]
            assert all(len(r[0]) <= cap for r in reports)
            triples, n_bad, counts = M.merge_reports(len(reqs), classes, reports, cap)
            assert triples == every[:cap] and n_bad == len(every) and counts == brute_counts, (trial, cap)


def test_fill_from_a_name_table_against_real_files_asan_ubsan_and_tsan(tmp_path):
    """csrc/fill_pipeline.hpp with a name table (what trees_build_file_list hands the pipe): files of unequal lengths -- short, exact,
    long, missing -- under unrelated names in shuffled order, several threads, every buffer against a plain read; short files read as
    zeros, a missing file fails the join and is named.  No GPU, no HIP."""
    src = os.path.join(ROOT, "tests", "host_check", "fill_names_check.cpp")
    inc = "-I" + os.path.join(ROOT, "codex-storage-proofs-circuits_amd", "csrc")
    for name, flags, shapes in (("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "60"), ("tsan", ["-fsanitize=thread"], "24")):
        exe = str(tmp_path / ("fill_names_" + name))
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wall", *flags, inc, "-o", exe, src])
        scratch = tmp_path / ("files_" + name)
        scratch.mkdir()
        r = subprocess.run([exe, str(scratch), shapes], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-4000:])
        assert "fill names ok: %s shapes" % shapes in r.stdout and "ThreadSanitizer" not in r.stderr, (name, r.stdout, r.stderr[-2000:])
        assert " 0 turns named a missing file" not in r.stdout and " 0 cells past a short file" not in r.stdout
        assert list(scratch.iterdir()) == []
