"""What serving costs a fill session: cp2_fill_add with the nodes kept against a plain session, cp2_fill_block_proofs against
cp2_dataset_block_proofs, and cp2_fill_keep_nodes on a half-full session against cp2_fill_finish.

A session that keeps nodes (cp2_fill_keep_nodes) ends every add in k_block_path_commit_nodes: the walk of k_block_path_commit plus, per
request, 2 x depth conversions to canonical form and 4 x depth + 2 16-byte stores.  The source is fake, so no file system is in any number.
  (a) add     fill_rate.py's two shapes -- --slots 128 fake slots of --slot-mib 8 MiB (16 384 blocks of 64 KiB, depth 7), and the same number
              of blocks into ONE fake slot of 2^--deep-log2 cells (depth 17) -- from pageable and from pinned memory, a plain session and a
              keeping one alternated.  Every timed add goes into a fresh session (begun, and keeping turned on, outside the timing).
  (b) proofs  the 16 384 blocks of the full keeping session asked from it, against the finished compact dataset asked the same.
  (c) keep    cp2_fill_keep_nodes on a session that holds every second block, against cp2_fill_finish on the full one.
In one process, after a warm-up of each leg, --repeats rounds of the legs alternated; medians.  --plain-only runs the plain legs of (a)
alone and needs nothing this tool's own tree adds, so with --root DIR (another checkout of the project, built) it measures that tree's
cp2_fill_add on the same bytes: the A/B against an earlier commit.  Prints one JSON line and, with --out, writes it with a heading
(--append: after what the file holds).

    python tools/fill_serve_rate.py [--slots 128] [--slot-mib 8] [--deep-log2 22] [--repeats 2] [--plain-only] [--root DIR] [--out FILE]
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
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import __graft_entry__ as g
    import torch
    pkg = g.load_package()
    ctx = pkg.Context(0)
    slot_bytes = a.slot_mib << 20
    n_cells, nb = slot_bytes // CELL, slot_bytes // BLOCK
    n_req = a.slots * nb
    record = {"tree": a.label or "this tree", "repeats": a.repeats}

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

    def medians(legs):
        times = {k: [] for k in legs}
        for k, f in legs.items():                                 # warm-up
            f()
        for _ in range(a.repeats):
            for k, f in legs.items():
                times[k].append(f())
        return {k: statistics.median(v) for k, v in times.items()}

    def adds(cfg, roots, reqs, paths, cand, pinned):
        def fill(data, keep):
            f = ctx.fill(cfg, roots)                              # (begin, keep_nodes and free are outside the timing)
            if keep:
                f.keep_nodes()
            dt, (st, n_new) = timed(lambda: f.add(reqs, data, paths))
            f.free()
            assert n_new == len(reqs) and (st == 0).all()
            return dt

        legs = {"plain": lambda: fill(cand, False), "plain_pin": lambda: fill(pinned, False)}
        if not a.plain_only:
            legs = {"plain": legs["plain"], "keep": lambda: fill(cand, True), "plain_pin": legs["plain_pin"], "keep_pin": lambda: fill(pinned, True)}
        med = medians(legs)
        gb = cand.nbytes / 1e9
        out = {"depth": int(paths.shape[1])}
        out.update({k + "_s": round(v, 4) for k, v in med.items()})
        out.update({k + "_GBps": round(gb / v, 2) for k, v in med.items()})
        if not a.plain_only:
            out["keep_over_plain"] = round(med["plain"] / med["keep"], 3)
            out["keep_pin_over_plain_pin"] = round(med["plain_pin"] / med["keep_pin"], 3)
        return out

    try:
        # ---- slots: every block of every fake slot, in (slot, block) order
        cfg = pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (a.slots - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=a.slots,
                              nCells=n_cells, nSamples=100, seed=1)
        cand = np.concatenate([ctx.gen_fake_cells(ctx.slot_seed(1, s), 0, n_cells, CELL).reshape(-1) for s in range(a.slots)])
        pinned = torch.from_numpy(cand).pin_memory().numpy()
        reqs = np.array([(s, b) for s in range(a.slots) for b in range(nb)], dtype=np.uint64)
        ds = build(cfg)
        roots = ds.local_roots()
        want_roots, paths = ds.block_proofs(reqs)
        record["add_slots"] = {"workload": "%d fake slots x %d MiB (2^%d cells x 2048 B, 64 KiB blocks); %d blocks (%d MiB), each sent once" %
                               (a.slots, a.slot_mib, n_cells.bit_length() - 1, n_req, n_req * BLOCK >> 20)}
        record["add_slots"].update(adds(cfg, roots, reqs, paths, cand, pinned))

        if not a.plain_only:
            # ---- (b) the proofs of all blocks from the full keeping session, and from the dataset it finishes into
            f = ctx.fill(cfg, roots)
            f.keep_nodes()
            assert f.add(reqs, pinned, paths)[1] == n_req
            st, got_roots, got_paths = f.block_proofs(reqs)
            assert (st == 0).all() and got_roots.tobytes() == want_roots.tobytes() and got_paths.tobytes() == paths.tobytes()
            med = medians({"session": lambda: timed(lambda: f.block_proofs(reqs))[0], "dataset": lambda: timed(lambda: ds.block_proofs(reqs))[0],
                           "session_statuses_only": lambda: timed(lambda: f.block_proofs(reqs, statuses_only=True))[0]})
            f.free()
            record["proofs"] = {"requests": n_req, "depth": int(paths.shape[1]), "session_s": round(med["session"], 5), "dataset_s": round(med["dataset"], 5),
                                "session_statuses_only_s": round(med["session_statuses_only"], 5),
                                "dataset_over_session": round(med["dataset"] / med["session"], 3)}

            # ---- (c) keep_nodes on a half-full session against finish on the full one
            half = np.ascontiguousarray(reqs[::2])
            half_data = np.ascontiguousarray(pinned.reshape(n_req, BLOCK)[::2])
            half_paths = np.ascontiguousarray(paths[::2])

            def keep_half():
                h = ctx.fill(cfg, roots)
                assert h.add(half, half_data, half_paths)[1] == len(half)
                dt, _ = timed(h.keep_nodes)
                h.free()
                return dt

            def finish_full():
                h = ctx.fill(cfg, roots)
                assert h.add(reqs, pinned, paths)[1] == n_req
                dt, filled = timed(h.finish)
                filled.free()
                h.free()
                return dt

            med = medians({"keep_nodes_half": keep_half, "finish": finish_full})
            record["keep_nodes"] = {"slots": a.slots, "blocks_per_slot": nb, "present": len(half), "keep_nodes_half_s": round(med["keep_nodes_half"], 5),
                                    "finish_s": round(med["finish"], 5), "keep_over_finish": round(med["keep_nodes_half"] / med["finish"], 2)}
        ds.free()
        del pinned, cand
        # ---- deep: the first n_req blocks of one fake slot of 2^deep_log2 cells
        deep_cells = 1 << a.deep_log2
        dcfg = pkg.make_config(maxDepth=32, maxLog2NSlots=1, cellSize=CELL, blockSize=BLOCK, nSlots=1, nCells=deep_cells, nSamples=100, seed=1)
        ds = build(dcfg)
        n_deep = min(n_req, deep_cells // CPB)
        cand = ctx.gen_fake_cells(ctx.slot_seed(1, 0), 0, n_deep * CPB, CELL).reshape(-1)
        pinned = torch.from_numpy(cand).pin_memory().numpy()
        reqs = np.array([(0, b) for b in range(n_deep)], dtype=np.uint64)
        roots = ds.local_roots()
        _, paths = ds.block_proofs(reqs)
        ds.free()
        record["add_deep"] = {"workload": "a session over one fake slot of 2^%d cells x 2048 B (%d blocks); its first %d blocks (%d MiB)" %
                              (a.deep_log2, deep_cells // CPB, n_deep, n_deep * BLOCK >> 20)}
        record["add_deep"].update(adds(dcfg, roots, reqs, paths, cand, pinned))
    finally:
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        args = ["--slots %d" % a.slots, "--slot-mib %d" % a.slot_mib, "--deep-log2 %d" % a.deep_log2, "--repeats %d" % a.repeats] + (["--plain-only"] if a.plain_only else [])
        with open(a.out, "a" if a.append else "w") as f:
            f.write("tools/fill_serve_rate.py on one MI355X (%s; medians of alternated rounds after a warm-up of each leg):\n%s\n" % (" ".join(args), line))


if __name__ == "__main__":
    main()
