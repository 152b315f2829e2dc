"""What the four block-path kernels cost at their launchers, with device events around each call.

fill_rate.py, fill_anchor_rate.py and block_proofs_rate.py time whole adds, where a 64 KiB block costs 1119 permutations and its path at
most 17: they cannot see k_block_path_roots, k_block_path_commit, k_block_path_commit_nodes or k_block_path_commit_anchored.  This tool
calls launch_block_path_* through the forwarder libraries of tests/device_check, on true requests, so that every lane matches and the
copy loops run: every block of ONE slot of 2^--depth blocks, whose tree is built on the device with launch_compress_layer, repeated to
2^--log2-requests requests.  All requests of a launch prove the same tree, so what they store are the bytes that stand there already.
Legs:
  roots       launch_block_path_roots, roots_out given
  commit      launch_block_path_commit
  nodes       launch_block_path_commit_nodes
  anch_full   launch_block_path_commit_anchored, every level equal to depth (the anchor is the stated slot root)
  anch_mixed  the same launcher, levels drawn uniformly from 0..depth with --seed, packed paths, each anchor the kept row at that level
After --warmup rounds of every leg, --rounds rounds of the legs alternated; per leg the median, the minimum, the maximum and the spread
(max - min) in milliseconds.  Every verdict word is checked to be 0 after the warm-up.  Prints one JSON line; --json writes it to a file.

    python tools/path_walk_rate.py [--depth 17] [--log2-requests 20] [--rounds 7] [--warmup 2] [--json new.json]

A/B of two builds: run the tool from each checkout with --json, then
    python tools/path_walk_rate.py --compare parent.json new.json [--out profiles/path_walk_ab.txt]
A leg passes when the second file's median is not above the first's by more than the larger of the two files' spreads of that leg: the
noise the measurement itself shows.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("roots", "commit", "nodes", "anch_full", "anch_mixed")
NO_ROW = (1 << 64) - 1


def compare(parent_path, new_path, out):
    parent, new = (json.load(open(p)) for p in (parent_path, new_path))
    lines = ["leg          parent median / spread ms     this median / spread ms     difference ms   margin ms   verdict"]
    ok = True
    for leg in LEGS:
        p, q = parent["legs"][leg], new["legs"][leg]
        margin, diff = max(p["spread_ms"], q["spread_ms"]), q["median_ms"] - p["median_ms"]
        good = diff <= margin
        ok = ok and good
        lines.append("%-12s %12.4f / %-12.4f %12.4f / %-12.4f %+12.4f %11.4f   %s" % (
            leg, p["median_ms"], p["spread_ms"], q["median_ms"], q["spread_ms"], diff, margin, "not slower" if good else "SLOWER"))
    lines.append("requests per launch %d, depth %d, rounds %d after %d warm-up rounds; parent on %s, this on %s" % (
        new["requests"], new["depth"], new["rounds"], new["warmup"], parent["device"], new["device"]))
    lines.append("all legs pass" if ok else "at least one leg is slower than the parent by more than the spread")
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=17)
    ap.add_argument("--log2-requests", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0x9A7B)
    ap.add_argument("--json", default=None)
    ap.add_argument("--compare", nargs=2, metavar=("PARENT_JSON", "NEW_JSON"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare[0], a.compare[1], a.out)
    assert 1 <= a.depth <= a.log2_requests <= 24
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    import torch
    g.load_package().load_library()
    vp, sz, u64, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib = lambda name: ctypes.CDLL(os.path.join(ROOT, "tests", "device_check", name))      # noqa: E731
    ku, fnu, fau = lib("libkernel_unit.so"), lib("libfill_nodes_unit.so"), lib("libfill_anchor_unit.so")
    for f, args in ((ku.ku_compress_layer, [vp, vp, sz, sz, i32, sz, sz]),
                    (ku.ku_block_path_roots, [vp, vp, vp, vp, u64, u32, sz, vp, vp]),
                    (ku.ku_block_path_commit, [vp, vp, vp, vp, vp, u64, u32, sz, vp, vp, u64]),
                    (fnu.fnu_block_path_commit_nodes, [vp, vp, vp, vp, vp, vp, vp, u64, u32, sz, vp, vp, u64, vp]),
                    (fau.fau_block_path_commit_anchored, [vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, u64, u32, sz, vp, vp, u64, vp])):
        f.restype, f.argtypes = i32, args

    depth, nb, n = a.depth, 1 << a.depth, 1 << a.log2_requests
    sizes = [nb >> l for l in range(depth + 1)]
    offs = [sum(sizes[:l]) for l in range(depth + 1)]                   # the compact layout of one local slot
    n_rows = sum(sizes)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)

    # the slot's tree: random block roots below 2^253 < r, the layers above by launch_compress_layer
    leaves = rng.integers(0, 256, size=(nb, 32), dtype=np.uint8)
    leaves[:, 31] &= 0x1F
    tree = torch.zeros((n_rows, 32), dtype=torch.uint8, device=dev)
    tree[:nb] = torch.from_numpy(leaves).to(dev)
    row_ptr = lambda t, r: t.data_ptr() + 32 * r                          # noqa: E731
    for l in range(depth):
        assert ku.ku_compress_layer(row_ptr(tree, offs[l]), row_ptr(tree, offs[l + 1]), sizes[l], 1, int(l == 0), sizes[l], sizes[l + 1]) == 0
    torch.cuda.synchronize()

    # the requests: every block, with its whole path gathered from the tree, repeated to n
    blocks = torch.arange(nb, dtype=torch.int64, device=dev).repeat(n // nb)
    lv = torch.arange(depth, dtype=torch.int64, device=dev)
    sib_rows = torch.tensor(offs[:depth], dtype=torch.int64, device=dev)[None, :] + ((blocks[:, None] >> lv[None, :]) ^ 1)
    paths = tree[sib_rows.reshape(-1)].contiguous()                      # n x depth rows
    fresh = tree[blocks].contiguous()
    slot_block = torch.stack([torch.zeros_like(blocks), blocks], dim=1).contiguous()
    dest = blocks.clone()                                                 # layer 0 of slot 0 starts at row 0
    slot_roots = tree[n_rows - 1:].clone()
    layer_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    layer_size = torch.tensor(sizes, dtype=torch.int64, device=dev)
    verdict = torch.empty(n, dtype=torch.int32, device=dev)
    roots_out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    scratch = torch.empty((2 * n * depth, 32), dtype=torch.uint8, device=dev)

    # the anchored legs' tables: levels, the prefix sum, the packed siblings, the anchor rows
    def anchored_tables(levels_host):
        levels = torch.from_numpy(levels_host.astype(np.int32)).to(dev)
        off_host = np.concatenate([[0], np.cumsum(levels_host, dtype=np.int64)])
        packed = paths.reshape(n, depth, 32)[lv[None, :] < levels[:, None].to(torch.int64)].contiguous()
        assert packed.shape[0] == int(off_host[-1]) > 0
        lvl64 = levels.to(torch.int64)
        anchor = torch.where(lvl64 == depth, torch.full_like(blocks, -1), layer_off[lvl64] + (blocks >> lvl64))   # -1: UINT64_MAX
        return levels, torch.from_numpy(off_host[:-1].copy()).to(dev), packed, anchor.contiguous()

    full = anchored_tables(np.full(n, depth, dtype=np.int64))
    mixed = anchored_tables(rng.integers(0, depth + 1, size=n, dtype=np.int64))
    assert 2 * full[2].shape[0] <= scratch.shape[0]

    def anchored(t):
        levels, off, packed, anchor = t
        return fau.fau_block_path_commit_anchored(fresh.data_ptr(), packed.data_ptr(), levels.data_ptr(), off.data_ptr(), 0, slot_block.data_ptr(),
                                                  slot_roots.data_ptr(), dest.data_ptr(), anchor.data_ptr(), layer_off.data_ptr(),
                                                  layer_size.data_ptr(), nb, depth, n, verdict.data_ptr(), tree.data_ptr(), n_rows, scratch.data_ptr())

    calls = {
        "roots": lambda: ku.ku_block_path_roots(fresh.data_ptr(), paths.data_ptr(), slot_block.data_ptr(), slot_roots.data_ptr(), nb, depth, n,
                                                verdict.data_ptr(), roots_out.data_ptr()),
        "commit": lambda: ku.ku_block_path_commit(fresh.data_ptr(), paths.data_ptr(), slot_block.data_ptr(), slot_roots.data_ptr(), dest.data_ptr(),
                                                  nb, depth, n, verdict.data_ptr(), tree.data_ptr(), n_rows),
        "nodes": lambda: fnu.fnu_block_path_commit_nodes(fresh.data_ptr(), paths.data_ptr(), slot_block.data_ptr(), slot_roots.data_ptr(),
                                                         dest.data_ptr(), layer_off.data_ptr(), layer_size.data_ptr(), nb, depth, n,
                                                         verdict.data_ptr(), tree.data_ptr(), n_rows, scratch.data_ptr()),
        "anch_full": lambda: anchored(full),
        "anch_mixed": lambda: anchored(mixed),
    }

    def timed(leg):
        verdict.fill_(-1)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rc = calls[leg]()
        t1.record()
        torch.cuda.synchronize()
        assert rc == 0, "%s: launch error %d" % (leg, rc)
        return t0.elapsed_time(t1)

    before = tree.clone()
    for _ in range(a.warmup):
        for leg in LEGS:
            timed(leg)
            assert int(torch.count_nonzero(verdict)) == 0, "%s: a true request was refused" % leg
    assert torch.equal(tree, before), "a true request changed the tree it proves"
    ms = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            ms[leg].append(timed(leg))
    record = {"requests": n, "depth": depth, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
              "legs": {leg: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v),
                             "mreq_per_s": n / statistics.median(v) / 1e3} for leg, v in ms.items()}}
    line = json.dumps(record)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
