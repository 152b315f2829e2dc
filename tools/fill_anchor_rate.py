"""What an anchored add costs and what it saves: cp2_fill_add_anchored against cp2_fill_add with the nodes kept, on the same bytes.

A session that keeps nodes can take a block with only the siblings below the lowest node it already holds above it (cp2_fill_anchors,
cp2_fill_add_anchored); the last device step is k_block_path_commit_anchored instead of k_block_path_commit_nodes.  A 64 KiB block costs
32 x 34 + 31 = 1119 permutations and a path at most 17, so the expectation is a rate that cannot be told from the plain add's: what is
saved is path bytes.  The source is fake, so no file system is in any number.  fill_serve_rate.py's two shapes -- --slots 128 fake slots
of --slot-mib 8 MiB (16 384 blocks of 64 KiB, depth 7), and the same number of blocks into ONE fake slot of 2^--deep-log2 cells (depth 17)
-- from pageable and from pinned memory, three legs alternated, every timed leg into a fresh keeping session (begun, and keeping turned
on, outside the timing):
  keep       cp2_fill_add, every block with its whole path, one call
  anch_full  (a) cp2_fill_add_anchored with every level equal to depth: the same requests, paths and bytes, one call
  anch_low   (b) the blocks in a shuffled order (the same order every round) in batches of --batch, each batch at the levels
             cp2_fill_anchors names just before it; the timing holds the anchor queries and the adds, not the packing of the paths, which
             is the peers' work
In one process, after a warm-up of each leg, --repeats rounds of the legs alternated; medians, and the spread of the rounds of each leg.
Prints one JSON line and, with --out, writes it with a heading.

    python tools/fill_anchor_rate.py [--slots 128] [--slot-mib 8] [--deep-log2 22] [--batch 1024] [--repeats 2] [--out profiles/fill_anchor_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

CELL, BLOCK = 2048, 65536
CPB = BLOCK // CELL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--slot-mib", type=int, default=8)
    ap.add_argument("--deep-log2", type=int, default=22)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as g
    import torch
    pkg = g.load_package()
    ctx = pkg.Context(0)
    slot_bytes = a.slot_mib << 20
    n_cells, nb = slot_bytes // CELL, slot_bytes // BLOCK
    n_req = a.slots * nb
    record = {"repeats": a.repeats, "batch": a.batch}

    def timed(f):
        ctx.sync()
        t = time.perf_counter()
        r = f()
        return time.perf_counter() - t, r

    def build(cfg):
        ctx.set_keep_trees(2)
        try:
            return ctx.dataset(cfg)
        finally:
            ctx.set_keep_trees(-1)

    def adds(cfg, roots, reqs, paths, cand, n_blocks_of_slot):
        n, depth = len(reqs), int(paths.shape[1])
        order = np.random.default_rng(7).permutation(n)
        reqs_sh, paths_sh = np.ascontiguousarray(reqs[order]), np.ascontiguousarray(paths[order])
        cand_sh = np.ascontiguousarray(cand.reshape(n, BLOCK)[order])
        full_levels = np.full(n, depth, dtype=np.uint32)
        flat = paths.reshape(-1, 32)
        counted = {}

        def session():
            f = ctx.fill(cfg, roots)                              # (begin, keep_nodes and free are outside the timing)
            f.keep_nodes()
            return f

        def keep(data):
            f = session()
            dt, (st, n_new) = timed(lambda: f.add(reqs, data, paths))
            f.free()
            assert n_new == n and (st == 0).all()
            return dt

        def anch_full(data):
            f = session()
            dt, (st, n_new) = timed(lambda: f.add_anchored(reqs, data, full_levels, flat))
            f.free()
            assert n_new == n and (st == 0).all()
            return dt

        def anch_low(data):
            f = session()
            total, siblings, bare = 0.0, 0, 0
            for k in range(0, n, a.batch):
                sb = reqs_sh[k:k + a.batch]
                dt, levels = timed(lambda: f.anchors(sb))
                total += dt
                packed = np.concatenate([paths_sh[k + i][:int(lv)] for i, lv in enumerate(levels)] + [np.zeros((0, 32), np.uint8)])
                dt, (st, n_new) = timed(lambda: f.add_anchored(sb, data[k:k + a.batch], levels, packed))
                total += dt
                assert n_new == len(sb) and (st == 0).all()
                siblings += int(levels.sum())
                bare += int((levels == 0).sum())
            f.free()
            counted.update(siblings=siblings, bare=bare)
            return total

        out = {"depth": depth, "blocks": n}
        for tag, data, data_sh in (("", cand, cand_sh), ("_pin", torch.from_numpy(cand).pin_memory().numpy(), torch.from_numpy(cand_sh).pin_memory().numpy())):
            legs = {"keep": lambda: keep(data), "anch_full": lambda: anch_full(data), "anch_low": lambda: anch_low(data_sh)}
            times = {k: [] for k in legs}
            for f in legs.values():                               # warm-up
                f()
            for _ in range(a.repeats):
                for k, f in legs.items():
                    times[k].append(f())
            med = {k: statistics.median(v) for k, v in times.items()}
            gb = cand.nbytes / 1e9
            for k in legs:
                out[k + tag + "_s"] = round(med[k], 4)
                out[k + tag + "_GBps"] = round(gb / med[k], 2)
                out[k + tag + "_spread"] = round((max(times[k]) - min(times[k])) / med[k], 4)     # between the alternated rounds, of the median
            out["anch_full" + tag + "_over_keep"] = round(med["keep"] / med["anch_full"], 3)
            out["anch_low" + tag + "_over_keep"] = round(med["keep"] / med["anch_low"], 3)
            del data, data_sh
        out.update({"path_bytes_whole": n * depth * 32, "path_bytes_lowest": counted["siblings"] * 32, "siblings_lowest": counted["siblings"],
                    "blocks_without_a_sibling": counted["bare"], "n_blocks_minus_one": n - n // n_blocks_of_slot if n % n_blocks_of_slot == 0 else None,
                    "depth_x_n_blocks": n * depth})
        return out

    try:
        # ---- slots: every block of every fake slot
        cfg = pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (a.slots - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=a.slots,
                              nCells=n_cells, nSamples=100, seed=1)
        cand = np.concatenate([ctx.gen_fake_cells(ctx.slot_seed(1, s), 0, n_cells, CELL).reshape(-1) for s in range(a.slots)])
        reqs = np.array([(s, b) for s in range(a.slots) for b in range(nb)], dtype=np.uint64)
        ds = build(cfg)
        roots = ds.local_roots()
        _, paths = ds.block_proofs(reqs)
        ds.free()
        record["slots"] = {"workload": "%d fake slots x %d MiB (2^%d cells x 2048 B, 64 KiB blocks); %d blocks (%d MiB), each sent once" %
                           (a.slots, a.slot_mib, n_cells.bit_length() - 1, n_req, n_req * BLOCK >> 20)}
        record["slots"].update(adds(cfg, roots, reqs, paths, cand, nb))
        del cand
        # ---- deep: the first n_req blocks of one fake slot of 2^deep_log2 cells
        deep_cells = 1 << a.deep_log2
        dcfg = pkg.make_config(maxDepth=32, maxLog2NSlots=1, cellSize=CELL, blockSize=BLOCK, nSlots=1, nCells=deep_cells, nSamples=100, seed=1)
        ds = build(dcfg)
        n_deep = min(n_req, deep_cells // CPB)
        cand = ctx.gen_fake_cells(ctx.slot_seed(1, 0), 0, n_deep * CPB, CELL).reshape(-1)
        reqs = np.array([(0, b) for b in range(n_deep)], dtype=np.uint64)
        roots = ds.local_roots()
        _, paths = ds.block_proofs(reqs)
        ds.free()
        record["deep"] = {"workload": "a session over one fake slot of 2^%d cells x 2048 B (%d blocks); its first %d blocks (%d MiB)" %
                          (a.deep_log2, deep_cells // CPB, n_deep, n_deep * BLOCK >> 20)}
        record["deep"].update(adds(dcfg, roots, reqs, paths, cand, deep_cells // CPB))
    finally:
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        args = ["--slots %d" % a.slots, "--slot-mib %d" % a.slot_mib, "--deep-log2 %d" % a.deep_log2, "--batch %d" % a.batch, "--repeats %d" % a.repeats]
        with open(a.out, "w") as f:
            f.write("tools/fill_anchor_rate.py on one MI355X (%s; medians of alternated rounds after a warm-up of each leg):\n%s\n" % (" ".join(args), line))


if __name__ == "__main__":
    main()
