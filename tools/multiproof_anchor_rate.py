"""What a multiproof add against kept nodes costs and what it saves: cp2_fill_add_multi_anchored against cp2_fill_add_multi on the same bytes
and rows, and against cp2_fill_add_anchored in rows received.

fill_rate.py's shape: --slots 128 fake slots of --slot-mib 8 MiB (16 384 blocks of 64 KiB, depth 7), every timed leg into a fresh keeping
session (begun, and keeping turned on, outside the timing).  The source is fake, so no file system is in any number.
  multi       cp2_fill_add_multi, one group per slot holding every block of the slot (0 rows), one call: the yardstick
  anchored    cp2_fill_add_multi_anchored with the same groups: only the root is known, so the same bytes, rows, jobs and commit list, with
              the verdicts from k_multiproof_tops / k_multiproof_fold instead of the comparing jobs
The gate is the project's standing one: the median of `anchored` at most 1.10 of the yardstick's plus the spread between the yardstick's
rounds; the ratio is written down.  A second leg, recorded and not gated: the blocks in a shuffled order (the same every round) in
--batches batches, each batch one group per slot it touches, with the rows cp2_fill_multiproof_want names taken from a compact dataset by
place (cp2_dataset_block_tree_rows); the rows received are set against the siblings cp2_fill_anchors would ask for on a twin session that
takes the same batches through cp2_fill_add_anchored.  The timing of that leg holds the want queries and the adds, not the peers' serving.
In one process, after a warm-up of each leg, --repeats rounds alternated; medians.  Prints one JSON line and, with --out, writes it with a
heading.

    python tools/multiproof_anchor_rate.py [--slots 128] [--slot-mib 8] [--batches 16] [--repeats 3] [--out profiles/multiproof_anchor_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

CELL, BLOCK = 2048, 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--slot-mib", type=int, default=8)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as g
    pkg = g.load_package()
    ctx = pkg.Context(0)
    slot_bytes = a.slot_mib << 20
    n_cells, nb = slot_bytes // CELL, slot_bytes // BLOCK
    n = a.slots * nb

    def timed(f):
        ctx.sync()
        t = time.perf_counter()
        r = f()
        return time.perf_counter() - t, r

    def session(cfg, roots):
        f = ctx.fill(cfg, roots)                                  # (begin, keep_nodes and free are outside the timing)
        f.keep_nodes()
        return f

    try:
        cfg = pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (a.slots - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=a.slots,
                              nCells=n_cells, nSamples=100, seed=1)
        cand = np.concatenate([ctx.gen_fake_cells(ctx.slot_seed(1, s), 0, n_cells, CELL).reshape(-1) for s in range(a.slots)]).reshape(n, BLOCK)
        ctx.set_keep_trees(2)
        try:
            ds = ctx.dataset(cfg)
        finally:
            ctx.set_keep_trees(-1)
        roots = ds.local_roots()
        groups, blocks = [(s, nb) for s in range(a.slots)], [b for _ in range(a.slots) for b in range(nb)]
        none = np.zeros((0, 32), dtype=np.uint8)

        def multi():
            f = session(cfg, roots)
            dt, (st, n_new) = timed(lambda: f.add_multi(groups, blocks, cand, none))
            f.free()
            assert n_new == n and (st == 0).all()
            return dt

        def anchored():
            f = session(cfg, roots)
            dt, (st, n_new) = timed(lambda: f.add_multi_anchored(groups, blocks, cand, none))
            f.free()
            assert n_new == n and (st == 0).all()
            return dt

        order = np.random.default_rng(7).permutation(n)
        per = (n + a.batches - 1) // a.batches
        counted = {}

        def shuffled():
            f, twin = session(cfg, roots), session(cfg, roots)
            total, rows, siblings = 0.0, 0, 0
            for k in range(0, n, per):
                idx = np.sort(order[k:k + per])                   # by (slot, block): one group per slot the batch touches
                slots, counts = np.unique(idx // nb, return_counts=True)
                gs, bs = list(zip(slots.tolist(), counts.tolist())), (idx % nb).tolist()
                data = np.ascontiguousarray(cand[idx])
                dt, (li, per_group) = timed(lambda: f.multiproof_want(gs, bs))
                total += dt
                places = np.column_stack([np.repeat(slots, per_group.astype(np.int64)), li]) if len(li) else np.zeros((0, 3), dtype=np.uint64)
                sent = ds.block_tree_rows(places) if len(li) else none
                dt, (st, n_new) = timed(lambda: f.add_multi_anchored(gs, bs, data, sent))
                total += dt
                assert n_new == len(idx) and (st == 0).all()
                rows += len(li)
                pairs = np.column_stack([idx // nb, idx % nb]).astype(np.uint64)
                levels = twin.anchors(pairs)
                _, paths = ds.block_proofs(pairs)
                packed = np.concatenate([paths[i, :int(lv)] for i, lv in enumerate(levels)] + [none])
                st, n_new = twin.add_anchored(pairs, data, levels, packed if packed.size else None)
                assert n_new == len(idx) and (st == 0).all()
                siblings += int(levels.sum())
            f.free()
            twin.free()
            counted.update(rows=rows, siblings=siblings)
            return total

        legs = {"multi": multi, "anchored": anchored, "shuffled": shuffled}
        times = {k: [] for k in legs}
        for f in legs.values():                                   # warm-up
            f()
        for _ in range(a.repeats):
            for k, f in legs.items():
                times[k].append(f())
        ds.free()
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = max(times["multi"]) - min(times["multi"])
        gb = cand.nbytes / 1e9
        record = {"workload": "%d fake slots x %d MiB (64 KiB blocks of 2048 B cells); %d blocks (%d MiB), each sent once" % (a.slots, a.slot_mib, n, n * BLOCK >> 20),
                  "repeats": a.repeats, "batches": a.batches}
        for k in legs:
            record[k + "_s"] = round(med[k], 4)
            record[k + "_GBps"] = round(gb / med[k], 2)
        record.update({"multi_spread_s": round(spread, 4), "anchored_over_multi_time": round(med["anchored"] / med["multi"], 3),
                       "gate": "anchored_s <= 1.10 x multi_s + multi_spread_s", "gate_holds": bool(med["anchored"] <= 1.10 * med["multi"] + spread),
                       "shuffled_rows_received": counted["rows"], "shuffled_anchored_siblings": counted["siblings"], "n_blocks_minus_one_x_slots": n - a.slots,
                       "whole_path_siblings": n * (nb - 1).bit_length()})
    finally:
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/multiproof_anchor_rate.py on one MI355X (--slots %d --slot-mib %d --batches %d --repeats %d; medians of alternated rounds after a "
                    "warm-up of each leg):\n%s\n" % (a.slots, a.slot_mib, a.batches, a.repeats, line))
    return 0 if record["gate_holds"] else 1


if __name__ == "__main__":
    sys.exit(main())
