"""CPU checks of cp2_datasets_build_many: the name is exported and carries the same signature in the header, the ctypes binding and the
Nim binding; the scatter model (tests/build_many_models.py) equals a plain row loop; the model of the plan is held against brute force
over explicit layouts -- every (request, local slot, layer) row written exactly once, no two destinations of a request overlapping, every
kept row covered, in all three modes --; and the product's plan (csrc/build_many_plan.hpp), compiled stand-alone under AddressSanitizer +
UBSan, agrees with the model on seeded random calls."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import build_many_models as M
import nim_api as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
NAME = "cp2_datasets_build_many"
GEOMS = ((64, 256, 64), (64, 256, 128), (64, 128, 16), (32, 256, 8))     # cell size, block size, cells per slot


def test_the_name_is_exported_and_bound(pkg):
    protos, procs = N.header_prototypes(HEADER), N.nim_importc(NIM)
    L = pkg.load_library()
    assert NAME in set(pkg.exported_symbols())
    assert protos[NAME] == procs[NAME], (protos[NAME], procs[NAME])
    assert protos[NAME][0] == "i32" and len(protos[NAME][1]) == 5 and protos[NAME][1][0] == "handle:ctx" and protos[NAME][1][3] == "usize"
    assert getattr(L, NAME).restype is ctypes.c_int and len(L._cp2_signatures[NAME][1]) == 5
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    assert NAME in history and re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER)
    assert callable(pkg.Context.build_many)


def test_null_ctx_is_refused_and_out_is_cleared(pkg):
    L = pkg.load_library()
    out = (ctypes.c_void_p * 2)(5, 7)
    rg = (ctypes.c_uint64 * 4)(0, 1, 0, 1)
    cfgs = (pkg.Config * 2)()
    assert L.cp2_datasets_build_many(None, cfgs, rg, 2, out) == -1
    assert out[0] is None and out[1] is None
    assert L.cp2_datasets_build_many(None, None, None, 0, None) == -1


# ---- the scatter model against a plain row loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,sstride,n_items", [(1, 1, 1), (1, 3, 9), (3, 3, 5), (3, 5, 22), (16, 17, 7), (64, 70, 3), (5, 5, 0), (0, 2, 4)])
def test_scatter_model_equals_the_row_loop(rows, sstride, n_items):
    rng = np.random.default_rng([0xB11D, rows, sstride, n_items])
    src = rng.integers(0, 256, size=(max(1, n_items * sstride), 32), dtype=np.uint8)
    span = rows * 32 + 48
    mem = rng.integers(0, 256, size=16 + max(1, n_items) * span, dtype=np.uint8)
    place = rng.permutation(n_items)                                       # shuffled items, 16 bytes past a 32-byte boundary, gaps between
    addr = 16 + place.astype(np.int64) * span
    addr[::3] = 0                                                          # every third item keeps nothing
    before = mem.copy()
    a = M.scatter_model(src, sstride, mem.copy(), addr, rows, n_items)
    b = M.scatter_loop(src, sstride, mem.copy(), addr, rows, n_items)
    assert np.array_equal(a, b)
    touched = np.zeros(mem.size, dtype=bool)
    for i in range(n_items):
        if addr[i]:
            touched[addr[i]:addr[i] + rows * 32] = True
            assert np.array_equal(a[addr[i]:addr[i] + rows * 32].reshape(-1, 32), src[i * sstride:i * sstride + rows])
    assert np.array_equal(a[~touched], before[~touched])                   # gaps, the rows of the zero items, what follows the last row


# ---- the plan against brute force -------------------------------------------------------------------------------------------------------
def random_requests(rnd, n_classes):
    geoms = rnd.sample(GEOMS, n_classes)
    reqs = []
    for _ in range(rnd.randint(6, 14)):
        g = rnd.choice(geoms)
        reqs.append(M.Request(g[0], g[1], g[2], rnd.randint(1, 9), rnd.randint(1, 7), rnd.random() < 0.85))
    reqs.append(reqs[rnd.randrange(len(reqs))])                            # a repeat: an independent dataset
    reqs.append(M.Request(geoms[0][0], geoms[0][1], geoms[0][2], 3, 7, True))
    return reqs


def straddling_stage(reqs, rnd):
    """staging bytes whose batches put a multi-slot request of the last request's class across a batch boundary"""
    g = reqs[-1][:3]
    items = [s for q in reqs if q.from_file and q[:3] == g for s in range(q.n_local)]
    sizes = [b for b in range(2, 9) if any(items[i] > 0 for i in range(b, len(items), b))]
    return 2 * 32 * M.kept_layers(g[0], g[1], g[2], 1)[1] * rnd.choice(sizes) + rnd.randint(0, 31)


def label_rows(labels):
    """labels as 32-byte rows: four little-endian 64-bit words"""
    return np.asarray(labels, dtype="<u8").reshape(-1, 4).view(np.uint8).reshape(-1, 32)


@pytest.mark.parametrize("mode", [2, 0, 1])
@pytest.mark.parametrize("seed", range(6))
def test_plan_writes_every_kept_row_exactly_once(seed, mode):
    rnd = random.Random(seed * 3 + mode)
    reqs = random_requests(rnd, 2 + seed % 2)
    stage = straddling_stage(reqs, rnd)
    classes, fake = M.plan(reqs, stage)
    assert fake == [i for i, q in enumerate(reqs) if not q.from_file]
    assert len(classes) == len({(q.cell_size, q.block_size, q.n_cells) for q in reqs if q.from_file})
    # every request's own buffer in one flat memory, shuffled, 16 bytes past a 32-byte boundary, with gaps; fake-source requests: none
    kinds = {"b": 1, "t": 2}
    base, want, at = [0] * len(reqs), {}, 4096 + 16
    for i in rnd.sample(range(len(reqs)), len(reqs)):
        q = reqs[i]
        if not q.from_file:
            continue
        lay = M.kept_layout(q.cell_size, q.block_size, q.n_cells, q.n_local, mode)
        assert len(lay) == q.n_local * M.kept_layers(q.cell_size, q.block_size, q.n_cells, mode)[2]
        base[i], want[i] = at, lay
        at += len(lay) * 32 + 48
    mem = np.full(at, 0xEE, dtype=np.uint8)
    writes = np.zeros(at // 16 + 2, dtype=np.int32)                           # per 16 bytes: how often written
    straddles = 0
    for cls in classes:
        layers, item_rows, _ = M.kept_layers(cls.key[0], cls.key[1], cls.key[2], mode)
        assert cls.batch == max(1, min(len(cls.items), (stage // 2) // (item_rows * 32)))
        assert cls.items == [(i, s) for i, q in enumerate(reqs) if q.from_file and (q.cell_size, q.block_size, q.n_cells) == cls.key for s in range(q.n_local)]
        for i0 in range(0, len(cls.items), cls.batch):
            n = min(cls.batch, len(cls.items) - i0)
            straddles += int(i0 > 0 and cls.items[i0][1] > 0)
            # the batch as the builder leaves it: every layer of its n items, each row labelled (kind, layer, global item, row)
            full = M.full_layout(cls.key[0], cls.key[1], cls.key[2], n)
            assert len(full) == n * item_rows
            src = label_rows([(kinds[k], layer, i0 + j, r) for k, layer, j, r in full])
            table = M.addr_table(cls, layers, reqs, base, i0, n)
            assert len(table) == len(layers) * n
            for li, lay in enumerate(layers):
                addr = np.asarray(table[li * n:(li + 1) * n], dtype=np.int64)
                M.scatter_model(src[n * lay.src_prefix:], lay.rows, mem, addr, lay.rows, n)
                for a in addr:
                    assert a % 16 == 0 and a != 0
                    writes[a // 16:a // 16 + 2 * lay.rows] += 1
    assert straddles > 0, "no multi-slot request across a batch boundary: the case does not test what it claims"
    item_of = {}
    for cls in classes:
        for j, it in enumerate(cls.items):
            item_of.setdefault(it[0], {})[it[1]] = j
    covered = np.zeros_like(writes)
    for i, lay in want.items():
        expect = label_rows([(kinds[k], layer, item_of[i][s], r) for k, layer, s, r in lay])
        got = mem[base[i]:base[i] + len(lay) * 32].reshape(-1, 32)
        assert np.array_equal(got, expect), "request %d: its buffer is not the layout cp2_dataset_build gives it" % i
        covered[base[i] // 16:base[i] // 16 + 2 * len(lay)] = 1
    assert np.array_equal(writes, covered)                                   # exactly once where a request keeps a row, never anywhere else
    assert (mem.reshape(-1)[np.repeat(covered[:at // 16] == 0, 16)[:at]] == 0xEE).all()


def test_addr_zero_requests_are_left_out():
    reqs = [M.Request(64, 256, 64, 0, 2, True), M.Request(64, 256, 64, 0, 1, True)]
    classes, _ = M.plan(reqs, 1 << 20)
    layers = M.kept_layers(64, 256, 64, 2)[0]
    table = M.addr_table(classes[0], layers, reqs, [0, 4096], 0, 3)
    assert all(table[li * 3 + j] == 0 for li in range(len(layers)) for j in (0, 1)) and all(table[li * 3 + 2] for li in range(len(layers)))


# ---- the product's plan, stand-alone under the sanitizers, against the model ----------------------------------------------------------------
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bm") / "build_many_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "build_many_plan_check.cpp")])
    return exe


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("seed", range(8))
def test_product_plan_equals_the_model(check, tmp_path, seed):
    rnd = random.Random(1000 + seed)
    reqs = random_requests(rnd, 2 + seed % 2)
    stage = straddling_stage(reqs, rnd)
    for mode in (2, 0, 1):
        base, at = [], 1 << 20
        for q in reqs:
            base.append(at if q.from_file else 0)
            at += (q.n_local * M.kept_layers(q.cell_size, q.block_size, q.n_cells, mode)[2] * 32 + 255) // 256 * 256
        f = tmp_path / ("call%d.txt" % mode)
        f.write_text(M.describe(reqs, base, stage, mode))
        assert run(check, "plan", f) == M.expected(reqs, base, stage, mode)


def test_product_plan_at_the_workload_of_the_rate_tool(check, tmp_path):
    """4096 one-slot requests of 8 MiB (2048-byte cells, 64 KiB blocks) under the default 2 GiB staging chunk"""
    reqs = [M.Request(2048, 65536, 4096, k % 11, 1, True) for k in range(4096)]
    base = [(1 << 30) + 8192 * k for k in range(4096)]
    f = tmp_path / "call.txt"
    f.write_text(M.describe(reqs, base, 1 << 31, 2))
    got = run(check, "plan", f)
    assert got == M.expected(reqs, base, 1 << 31, 2)
    assert "kept_rows 255" in got and got.count("\nbatch ") == -(-4096 // ((1 << 30) // (M.kept_layers(2048, 65536, 4096, 1)[1] * 32)))


def test_product_table_refuses_a_row_outside_its_buffer(check, tmp_path):
    """a request whose buffer is a slot smaller than what was planned for it (never, in the product: the guard in front of the kernel)"""
    reqs = [M.Request(64, 256, 64, 0, 1, True), M.Request(64, 256, 64, 0, 2, True), M.Request(64, 256, 64, 0, 1, True)]
    for mode in (2, 0, 1):
        text = M.describe(reqs, [4096, 65536, 1 << 20], 1 << 20, mode)
        f = tmp_path / "call.txt"
        f.write_text(text)
        assert "table refused" not in run(check, "plan", f)
        f.write_text(text + "shrink 1\n")
        assert "table refused" in run(check, "plan", f)


REFUSALS = [
    ((4, 0, 0, 10, 3, 64, 256, 64, 1), "n_local is 0"),
    ((4, 3, 2, 10, 3, 64, 256, 64, 1), "slots 3 + 2 are not inside the dataset's 4"),
    ((4, 5, 1, 10, 3, 64, 256, 64, 1), "slots 5 + 1 are not inside the dataset's 4"),
    ((4, 0, 1, -1, 3, 64, 256, 64, 1), "max_depth and max_log2_nslots must not be negative"),
    ((4, 0, 1, 10, 3, 32768, 65536, 64, 1), "slot-file cells of 32768 bytes (at most 16384)"),
    ((4, 0, 1, 10, 3, 0, 256, 64, 0), "cell_size, block_size and n_cells must not be 0"),
    ((4, 0, 1, 10, 3, 64, 200, 64, 1), "block_size 200 is no multiple of cell_size 64"),
    ((4, 0, 1, 10, 3, 64, 256, 66, 1), "n_cells 66 is no multiple of the 4 cells of a block"),
    ((4, 0, 1, 10, 3, 64, 256, 64, 1), "-"),
    ((4, 0, 1, 10, 3, 32768, 65536, 64, 0), "-"),
]


@pytest.mark.parametrize("args,text", REFUSALS)
def test_product_refusal_words(check, args, text):
    assert run(check, "refusal", *args) == "refusal %s\n" % text
