"""GPU suite: launch_repair_judge_many on its own (csrc/kernels.hpp), through the forwarder of tests/device_check/repair_many_unit.hip.

cp2_datasets_repair_blocks_many reaches k_repair_judge_many only behind a host that builds every descriptor from a dataset's layout; here
the launcher gets its inputs directly.  One launch mixes trees of 1, 2, 3, 5, 8 and 64 blocks (odd sizes for the odd-last key rule) and
requests without a path (len 0: the row itself against `want`) with requests that walk their tree's whole depth, in a seeded shuffle, so
every wave holds both kinds and several depths.  The trees and paths are the oracle's (c_oracle.merkle_tree, poseidon2_ref.merkle_proof),
built once for the module; the `want` rows lie scattered over several allocations at addresses that are multiples of 16 and not of 32.

Each set of requests runs four ways: true (every verdict 0); a bit flipped in the fresh root (every verdict 1); a bit flipped in one
sibling, or in the want row of a request without a path (1); and one sibling, the slot root or the kept row handed in as value + r, which
is the same field element (0).  The verdicts sit between guard bytes that must not change, the packed paths are followed by guard bytes
too.  Two cross-checks must be bit exact: the len-0 requests through launch_repair_compare_addr (which compares bytes: the value + r way
is not held against it), and the path requests of every tree size through launch_block_path_roots, both through the forwarders that exist.

Sizes: n in {1, 63, 64, 65, 257}, and 600 requests launched in slices of 256."""
import ctypes
import faulthandler
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = os.path.join(ROOT, "tests", "device_check")
GUARD = 256
SIZES = ((1, 0), (63, 0), (64, 0), (65, 0), (257, 0), (600, 256))          # (n, slice)
WAYS = ("true", "fresh bit", "sibling bit", "plus r")
TREES = (1, 2, 3, 5, 8, 64)
N_ALLOC = 5
REQ = np.dtype([("want", "<u8"), ("blk", "<u8"), ("n_blocks", "<u8"), ("path_at", "<u8"), ("len", "<u4"), ("reserved", "<u4")])


@pytest.fixture(autouse=True)
def time_limit():
    """every case under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def check_lib(pkg, name):
    path = os.path.join(DEV, name)
    if not os.path.exists(path):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/" + name], stdout=subprocess.DEVNULL)
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def libs(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    vp, sz, i32, u64, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32
    rmu, rbu, ku = check_lib(pkg, "librepair_many_unit.so"), check_lib(pkg, "libread_blocks_unit.so"), check_lib(pkg, "libkernel_unit.so")
    rmu.rmu_repair_judge_many.restype, rmu.rmu_repair_judge_many.argtypes = i32, [vp, vp, vp, sz, vp, sz]
    rmu.rmu_req_bytes.restype = sz
    assert rmu.rmu_req_bytes() == REQ.itemsize == 40
    rbu.rbu_repair_compare_addr.restype, rbu.rbu_repair_compare_addr.argtypes = i32, [vp, vp, sz, vp, sz]
    ku.ku_block_path_roots.restype, ku.ku_block_path_roots.argtypes = i32, [vp, vp, vp, vp, u64, u32, sz, vp, vp]
    return rmu, rbu, ku


@pytest.fixture(scope="module")
def trees(oracle):
    """per tree size: the oracle's layers as integers, its root, and the proof of every block -- computed once, never changed"""
    c_oracle, ref = oracle
    rng = np.random.default_rng(950)
    out = {}
    for nb in TREES:
        leaves = [int.from_bytes(rng.bytes(32), "little") % ref.R_MOD for _ in range(nb)]
        layers = [c_oracle.array_to_felts(layer) for layer in c_oracle.merkle_tree(c_oracle.felts_to_array(leaves))]
        assert layers[0] == leaves and len(layers[-1]) == 1
        proofs = [ref.merkle_proof(layers, b) for b in range(nb)]
        assert all(len(p["merklePath"]) == max(1, (nb - 1).bit_length()) for p in proofs)
        if nb in (3, 5):
            assert ref.reconstruct_root(proofs[nb - 1]) == layers[-1][0]     # the odd last node: the oracle's own two halves agree
        out[nb] = (layers, layers[-1][0], proofs)
    return out


def up(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def felt(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint8)


def make_case(trees, r_mod, n, way):
    """(fresh rows, packed path rows, want rows, per request (n_blocks, blk, len, path_at), expected verdicts)"""
    rng = np.random.default_rng(n * 31 + WAYS.index(way))
    kinds = [(TREES[i % len(TREES)], i % (2 * len(TREES)) >= len(TREES)) for i in range(n)]   # every tree size with and without a path ...
    kinds = [kinds[i] for i in rng.permutation(n)]                                            # ... in a seeded shuffle
    fresh, want, paths, meta = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), [], []
    for i, (nb, walk) in enumerate(kinds):
        layers, root, proofs = trees[nb]
        b = int(rng.integers(0, nb)) if i % 5 else nb - 1                     # the last block often: the odd tail's key
        leaf, sibs = layers[0][b], list(proofs[b]["merklePath"]) if walk else []
        target = root if walk else leaf
        if way == "fresh bit":
            leaf ^= 1 << int(rng.integers(0, 250))
        elif way == "sibling bit":
            if walk:
                sibs[int(rng.integers(0, len(sibs)))] ^= 1 << int(rng.integers(0, 250))
            else:
                target ^= 1 << int(rng.integers(0, 250))
        elif way == "plus r":
            if walk and i % 3:
                sibs[int(rng.integers(0, len(sibs)))] += r_mod
            else:
                target += r_mod
        fresh[i], want[i] = felt(leaf), felt(target)
        meta.append((nb, b, len(sibs), len(paths)))
        paths += [felt(s) for s in sibs]
    expect = np.full(n, 1 if way in ("fresh bit", "sibling bit") else 0, dtype=np.uint32)
    return fresh, (np.stack(paths) if paths else np.zeros((0, 32), np.uint8)), want, meta, expect


def scatter(torch, rng, want):
    """the want rows dealt over N_ALLOC allocations, row j of an allocation at its base + 16 + 64 * j; returns (tensors, addresses)"""
    n = want.shape[0]
    owner = rng.integers(0, N_ALLOC, n)
    hosts = [rng.integers(0, 256, 16 + 64 * (int((owner == a).sum()) + 1), dtype=np.uint8) for a in range(N_ALLOC)]
    offs, seen = np.zeros(n, dtype=np.int64), [0] * N_ALLOC
    for i in range(n):
        offs[i] = 16 + 64 * seen[owner[i]]
        seen[owner[i]] += 1
        hosts[owner[i]][offs[i]:offs[i] + 32] = want[i]
    devs = [up(torch, h) for h in hosts]
    addr = np.array([devs[owner[i]].data_ptr() + int(offs[i]) for i in range(n)], dtype=np.uint64)
    assert all(int(a) % 32 == 16 for a in addr)
    return devs, addr


def guarded(torch, n_words):
    pre = np.full(GUARD + 4 * n_words + GUARD, 0xA5, dtype=np.uint8)
    return pre, up(torch, pre)


def verdicts_of(pre, dev, n_words):
    g = dev.cpu().numpy()
    assert np.array_equal(g[:GUARD], pre[:GUARD]) and np.array_equal(g[GUARD + 4 * n_words:], pre[GUARD + 4 * n_words:])
    return g[GUARD:GUARD + 4 * n_words].view(np.uint32).copy()


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("n,slice_", SIZES)
def test_mixed_depths_and_kinds_in_one_launch(libs, trees, oracle, n, slice_, way):
    import torch
    rmu, rbu, ku = libs
    r_mod = oracle[1].R_MOD
    fresh, paths, want, meta, expect = make_case(trees, r_mod, n, way)
    rng = np.random.default_rng(n + 1000 * WAYS.index(way))
    keep, addr = scatter(torch, rng, want)
    reqs = np.zeros(n, dtype=REQ)
    for i, (nb, b, ln, at) in enumerate(meta):
        reqs[i] = (addr[i], b, nb, at, ln, 0)
    if n >= 63:        # every wave of 64 lanes holds both kinds and more than one depth
        for w0 in range(0, n - 62, 64):
            lens = {int(x) for x in reqs["len"][w0:w0 + 64]}
            assert 0 in lens and len(lens) >= 3
    tail = np.full(GUARD, 0x5A, dtype=np.uint8)
    d_fresh, d_reqs = up(torch, fresh), up(torch, reqs)
    d_paths = up(torch, np.concatenate([paths.reshape(-1), tail]))
    pre, out = guarded(torch, n)
    assert rmu.rmu_repair_judge_many(d_fresh.data_ptr(), d_paths.data_ptr(), d_reqs.data_ptr(), n, out.data_ptr() + GUARD, slice_) == 0
    torch.cuda.synchronize()
    got = verdicts_of(pre, out, n)
    print("n %d %s: %d verdict(s) 1 of %d, expected %d" % (n, way, int(got.sum()), n, int(expect.sum())))
    assert np.array_equal(got, expect)
    assert np.array_equal(d_paths.cpu().numpy()[paths.size:], tail) and np.array_equal(d_fresh.cpu().numpy(), fresh.reshape(-1))
    # ---- the requests without a path through launch_repair_compare_addr (bytes against bytes: not the value + r way) --------------------------
    flat = [i for i in range(n) if meta[i][2] == 0]
    if flat and way != "plus r":
        d_f, d_a = up(torch, fresh[flat]), up(torch, addr[flat])
        pre2, out2 = guarded(torch, len(flat))
        assert rbu.rbu_repair_compare_addr(d_f.data_ptr(), d_a.data_ptr(), len(flat), out2.data_ptr() + GUARD, slice_) == 0
        torch.cuda.synchronize()
        assert np.array_equal(verdicts_of(pre2, out2, len(flat)), got[flat])
    # ---- the path requests of every tree size through launch_block_path_roots: its own layout, the same rows --------------------------------
    for nb in TREES:
        sub = [i for i in range(n) if meta[i][0] == nb and meta[i][2]]
        if not sub:
            continue
        depth = meta[sub[0]][2]
        p = np.concatenate([paths[meta[i][3]:meta[i][3] + depth] for i in sub])
        root_block = np.array([[q, meta[i][1]] for q, i in enumerate(sub)], dtype=np.uint64)
        d_f, d_p, d_rb, d_roots = up(torch, fresh[sub]), up(torch, p), up(torch, root_block), up(torch, want[sub])
        pre3, out3 = guarded(torch, len(sub))
        assert ku.ku_block_path_roots(d_f.data_ptr(), d_p.data_ptr(), d_rb.data_ptr(), d_roots.data_ptr(), nb, depth, len(sub), out3.data_ptr() + GUARD, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(verdicts_of(pre3, out3, len(sub)), got[sub]), nb
    del keep


def test_a_zero_or_misaligned_want_is_a_mismatch_and_nothing_to_launch_is_fine(libs, trees):
    import torch
    rmu = libs[0]
    leaf = trees[1][0][0][0]
    fresh = np.stack([felt(leaf)] * 4)
    kept = up(torch, np.concatenate([np.zeros(16, np.uint8), felt(leaf), np.zeros(16, np.uint8)]))
    reqs = np.zeros(4, dtype=REQ)
    for i, a in enumerate((kept.data_ptr() + 16, 0, kept.data_ptr() + 24, kept.data_ptr() + 16)):
        reqs[i] = (a, 0, 1, 0, 0, 0)
    d_fresh, d_reqs = up(torch, fresh), up(torch, reqs)
    pre, out = guarded(torch, 4)
    assert rmu.rmu_repair_judge_many(d_fresh.data_ptr(), None, d_reqs.data_ptr(), 4, out.data_ptr() + GUARD, 0) == 0      # no paths: every len is 0
    torch.cuda.synchronize()
    assert verdicts_of(pre, out, 4).tolist() == [0, 1, 1, 0]
    assert rmu.rmu_repair_judge_many(d_fresh.data_ptr(), None, d_reqs.data_ptr(), 0, out.data_ptr() + GUARD, 0) == 0
    assert rmu.rmu_repair_judge_many(None, None, d_reqs.data_ptr(), 4, out.data_ptr() + GUARD, 0) == 1                   # hipErrorInvalidValue, nothing launched
    assert verdicts_of(pre, out, 4).tolist() == [0, 1, 1, 0]
