"""CPU checks of the verified read-back (cp2_datasets_read_blocks, cp2_dataset_read_blocks): the two names are exported and carry the same
signature in the header, the ctypes binding and the Nim binding; the host plan (csrc/read_blocks_plan.hpp), compiled stand-alone under
AddressSanitizer + UBSan, agrees with the Python model (tests/read_blocks_models.py) on seeded random calls -- refusals with their
indices, read order, chunks, packed path offsets, both address tables -- and its reader obeys the builders' read rule on real files."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import nim_api as N
import read_blocks_models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
WANT = {
    "cp2_datasets_read_blocks": ("i32", ["handle:ctx", "ptr(handle:dataset)", "usize", "ptr(u64)", "usize", "i32", "ptr(u8)", "ptr(u8)", "ptr(u8)",
                                         "ptr(u64)", "ptr(u32)", "ptr(usize)"]),
    "cp2_dataset_read_blocks": ("i32", ["handle:dataset", "ptr(u64)", "usize", "i32", "ptr(u8)", "ptr(u8)", "ptr(u8)", "ptr(u32)", "ptr(usize)"]),
}


def test_the_two_names_are_exported_and_bound(pkg):
    protos = N.header_prototypes(HEADER)
    procs = N.nim_importc(NIM)
    L = pkg.load_library()
    assert set(WANT) <= set(pkg.exported_symbols())
    for name, sig in WANT.items():
        assert protos[name] == sig, name
        assert procs[name] == sig, name
        assert getattr(L, name).restype is ctypes.c_int
        assert len(L._cp2_signatures[name][1]) == len(sig[1]), name
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    assert all(name in history for name in WANT)
    assert re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER)
    assert HEADER.index("int cp2_dataset_block_proofs(") < HEADER.index("int cp2_datasets_read_blocks(") < HEADER.index("int cp2_fill_begin(")
    assert [int(v) for v in re.findall(r"#define CP2_READ_(?:CHECK_ONLY|OK|DAMAGED)\s+(\d+)", HEADER)] == [1, 0, 1]
    assert (pkg.READ_CHECK_ONLY, pkg.READ_OK, pkg.READ_DAMAGED) == (1, 0, 1)
    assert callable(pkg.Context.read_blocks) and callable(pkg.Dataset.read_blocks)


def test_null_handles_are_refused(pkg):
    L = pkg.load_library()
    st = (ctypes.c_uint32 * 1)(77)
    ok = ctypes.c_size_t(55)
    rq = (ctypes.c_uint64 * 3)(0, 0, 0)
    assert L.cp2_datasets_read_blocks(None, None, 0, rq, 1, 0, None, None, None, None, st, ctypes.byref(ok)) == -1
    assert L.cp2_dataset_read_blocks(None, rq, 1, 0, None, None, None, st, ctypes.byref(ok)) == -1
    assert st[0] == 77 and ok.value == 55


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rb") / "read_blocks_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "read_blocks_check.cpp")])
    return exe


def run(exe, mode, text, tmp, *more):
    f = tmp / "call.txt"
    f.write_text(text)
    r = subprocess.run([exe, mode, str(f)] + [str(m) for m in more], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    return r.stdout


def random_datasets(rng, n):
    ds, nodes = [], 0x7f0000000000
    for k in range(n):
        if k and rng.random() < 0.2:                         # the same handle listed again
            j = rng.randrange(k)
            d = M.Dataset(**{**ds[j].__dict__})
            d.same_as = ds[j].same_as
        else:
            d = M.Dataset(n_cells=32 * rng.choice([1, 2, 3, 4, 5, 8, 13, 32]), first_slot=rng.randrange(5), n_local=rng.randrange(1, 4),
                          mode=rng.choice([1, 2]), from_file=rng.random() < 0.8, base="b%d_" % k, seed=rng.randrange(99), nodes=nodes, same_as=k).layout()
            nodes += 0x100000 + 16 * rng.randrange(1, 9) * 2
        ds.append(d)
    return ds


def random_requests(rng, ds, n):
    req = []
    for _ in range(n):
        if req and rng.random() < 0.25:
            req.append(rng.choice(req))                      # a repeat
            continue
        k = rng.randrange(len(ds))
        req.append((k, ds[k].first_slot + rng.randrange(ds[k].n_local), rng.randrange(ds[k].n_blocks)))
    return req


def parse_plan(out):
    chunks, rest = [], {}
    for line in out.splitlines():
        w = line.split()
        if w[0] == "chunk":
            chunks.append([])
        elif w[0] == "group":
            chunks[-1].append((int(w[1]), int(w[2]), [int(x) for x in w[3:]]))
        else:
            rest[w[0]] = [int(x) for x in w[1:]]
    return chunks, rest


def test_plan_against_the_model(check, tmp_path):
    rng = random.Random(20260)
    for trial in range(40):
        ds = random_datasets(rng, rng.randrange(1, 6))
        req = random_requests(rng, ds, rng.randrange(0, 40))
        chunk = rng.choice([1, 2, 3, 7, 8, 64])
        have = ("ds", "req", "data", "status") + (("paths", "path_off") if trial % 2 else ())
        assert M.refusal(ds, req, 0, have) is None
        chunks, rest = parse_plan(run(check, "plan", M.describe(ds, req, chunk, 0, have), tmp_path))
        assert chunks == M.read_plan(ds, req, chunk), trial
        assert rest["path_off"] == M.path_off(ds, req), trial
        assert rest["addr"] == M.addr_table(ds, req), trial
        assert all(a % 16 == 0 for a in rest["addr"])
        assert rest["chunk_of"] == [M.chunk_size(1 << 20, 4096, len(req)) if req else 0]
        # every file-sourced request is read exactly once, in its own chunk
        read = sorted(i for c in chunks for g in c for i in g[2])
        assert read == [i for i, r in enumerate(req) if ds[r[0]].from_file]


def test_the_chunks_of_a_one_mebibyte_stage():
    assert M.chunk_size(1 << 20, 65536, 17) == 8 and M.chunk_size(1 << 31, 65536, 17) == 17 and M.chunk_size(1 << 20, 1 << 20, 5) == 1


def test_refusals_against_the_model(check, tmp_path):
    rng = random.Random(7)
    base = random_datasets(rng, 3)
    for d in base:
        d.mode, d.from_file = 2, True
        d.layout()
    ok_req = random_requests(rng, base, 6)
    full = ("ds", "req", "data", "status")

    def variant(**kw):
        ds = [M.Dataset(**{**d.__dict__}) for d in base]
        return ds, list(ok_req), kw.get("flags", 0), kw.get("have", full)

    cases = []
    cases.append(variant(flags=2))
    cases.append(variant(have=full + ("paths",)))
    cases.append(variant(have=full + ("path_off",)))
    cases.append(variant(have=("req", "data", "status")))
    cases.append(variant(have=("ds", "data", "status")))
    cases.append(variant(have=("ds", "req", "data")))
    cases.append(variant(have=("ds", "req", "status")))
    for what in ("null", "foreign", "cell", "block", "roots", "units", "layers"):
        for k in (1, 2):
            ds, req, fl, have = variant()
            d = ds[k]
            if what == "null": d.null = True
            if what == "foreign": d.foreign = True
            if what == "cell": d.cell_size = 64
            if what == "block": d.block_size = 8192
            if what == "roots": d.mode = 0
            if what == "units": d.whole = False
            if what == "layers": d.offs, d.sizes = d.offs[:-1], d.sizes[:-1]
            cases.append((ds, req, fl, have))
    for i in (0, 3, 5):
        for what in ("dataset", "slot low", "slot high", "block"):
            ds, req, fl, have = variant()
            k, s, b = req[i]
            d = ds[k]
            if what == "slot low" and d.first_slot == 0:
                continue
            req[i] = {"dataset": (len(ds), s, b), "slot low": (k, d.first_slot - 1, b), "slot high": (k, d.first_slot + d.n_local, b),
                      "block": (k, s, d.n_blocks)}[what]
            cases.append((ds, req, fl, have))
    kinds = set()
    for ds, req, fl, have in cases:
        want = M.refusal(ds, req, fl, have)
        assert want is not None
        out = run(check, "plan", M.describe(ds, req, 4, fl, have), tmp_path)
        assert out.startswith("refused read blocks: "), out
        assert M.REFUSAL_WORDS[want[0]] in out, (want, out)
        if want[1] is not None:
            assert ("dataset %d:" % want[1] if want[0].startswith("dataset") else "request %d:" % want[1]) in out, (want, out)
        kinds.add(want[0])
    assert kinds == set(M.REFUSAL_WORDS)
    # check only lets data be NULL; nothing at all is fine with n == 0
    ds, req, _, _ = variant()
    assert not run(check, "plan", M.describe(ds, req, 4, 1, ("ds", "req", "status")), tmp_path).startswith("refused")
    out = run(check, "plan", M.describe(ds, [], 4, 0, ()), tmp_path)
    assert "path_off 0" in out and "refused" not in out


def file_datasets(tmp_path):
    a = M.Dataset(n_cells=32 * 4, n_local=2, base=str(tmp_path / "a_"), same_as=0).layout()     # 4 blocks of 4096 bytes a slot
    b = M.Dataset(n_cells=32 * 4, n_local=2, base=str(tmp_path / "b_"), same_as=1, nodes=1 << 20).layout()
    return [a, b]


def test_reader_on_real_files(check, tmp_path):
    rng = np.random.default_rng(5)
    ds = file_datasets(tmp_path)
    bytes_of = {}
    for name, size in (("a_0", 4 * 4096), ("a_1", 4096 + 1000), ("b_0", 4 * 4096), ("b_1", 2 * 4096)):
        bytes_of[name] = rng.integers(0, 256, size, dtype=np.uint8)
        (tmp_path / (name + ".dat")).write_bytes(bytes_of[name].tobytes())
    # whole blocks, a repeat, the same slot number under two base names, a block that straddles the end, blocks wholly past the end
    req = [(0, 0, 3), (1, 0, 3), (0, 1, 1), (0, 0, 0), (0, 1, 2), (1, 1, 2), (0, 0, 3), (1, 1, 1), (0, 1, 0)]
    for chunk in (1, 4, 64):
        out = tmp_path / "rows.bin"
        assert run(check, "read", M.describe(ds, req, chunk), tmp_path, out).startswith("read ok %d" % len(req))
        rows = np.frombuffer(out.read_bytes(), dtype=np.uint8).reshape(len(req), 4096)
        for i, (k, s, b) in enumerate(req):
            have = bytes_of["%s_%d" % ("ab"[k], s)][b * 4096:(b + 1) * 4096]
            want = np.zeros(4096, dtype=np.uint8)
            want[:have.size] = have
            assert np.array_equal(rows[i], want), (chunk, i)
    assert 0 < bytes_of["a_1"][4096:].size < 4096 and bytes_of["b_1"].size == 2 * 4096
    # zero requests
    assert run(check, "read", M.describe(ds, [], 4), tmp_path, tmp_path / "none.bin").startswith("read ok 0")
    # a missing file: "cannot open", names the file
    os.remove(tmp_path / "b_0.dat")
    out = run(check, "read", M.describe(ds, req, 4), tmp_path, tmp_path / "x.bin")
    assert out.strip() == "error cannot open " + str(tmp_path / "b_0.dat")
    # a directory in the file's place: a read error, not zeros
    (tmp_path / "b_0.dat").mkdir()
    out = run(check, "read", M.describe(ds, req, 64), tmp_path, tmp_path / "x.bin")
    assert out.startswith("error cannot read " + str(tmp_path / "b_0.dat") + ": "), out
    assert not (tmp_path / "x.bin").exists()
