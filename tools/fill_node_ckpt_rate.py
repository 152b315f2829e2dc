"""Time of cp2_fill_save_nodes and cp2_fill_resume_nodes against the entry points they extend, on the same session in one process.

A keeping session (cp2_fill_keep_nodes from the start) receives every second block of every slot with its whole path: half the blocks are
present, and every row of the compact layout is known -- the block roots of the absent blocks as siblings, every upper node as an ancestor
or a sibling.  After a resume presence gives back the present block roots only, so every other saved row is a candidate that
k_nodes_restore_layer has to authenticate top-down from the stated roots: the most a checkpoint of that size can ask of it.
  slots   --slots 128 slots of --slot-mib 8 MiB (2^12 cells x 2048 B, 64 KiB blocks: 128 blocks a slot) under --dir
  deep    one slot of 2^--deep-log2 cells (2^22: 8 GiB, 131 072 blocks); --deep-log2 0 leaves it out
After a warm-up of each leg, --repeats rounds of the legs alternated:
  save                cp2_fill_save                                  save_nodes            cp2_fill_save_nodes
  base_trust          cp2_fill_resume + cp2_fill_keep_nodes, files trusted     nodes_trust     cp2_fill_resume_nodes, files trusted
  base_recheck        the same with the re-check                     nodes_recheck         cp2_fill_resume_nodes with the re-check
Medians and the spread of the rounds (max - min over the median) per leg.  Prints one JSON line and, with --out, writes it with a heading.

    python tools/fill_node_ckpt_rate.py --dir DIR [--slots 128] [--slot-mib 8] [--deep-log2 22] [--repeats 2] [--out FILE]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

CELL, BLOCK = 2048, 65536
CPB = BLOCK // CELL
PIECE_BLOCKS = 8192                        # blocks per add while filling: 512 MiB of candidates in host memory at a time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="an empty or new directory for the slot files and checkpoints; removed at the end")
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--slot-mib", type=int, default=8)
    ap.add_argument("--deep-log2", type=int, default=22)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = g.load_package()
    ctx = pkg.Context(0)
    record = {"repeats": a.repeats}

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

    def leg(name, n_slots, n_cells):
        d = os.path.join(a.dir, name)
        os.makedirs(d)
        nb = n_cells // CPB
        geom = dict(maxDepth=32, maxLog2NSlots=max(1, (n_slots - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=n_slots, nCells=n_cells,
                    nSamples=100, seed=1)
        fake = build(pkg.make_config(**geom))                     # the roots and paths a peer would send; the files hold the same bytes
        roots = fake.local_roots()
        cfg = pkg.make_config(file=os.path.join(d, "slot"), **geom)
        f = ctx.fill(cfg, roots)
        f.keep_nodes()
        for s in range(n_slots):
            for b0 in range(0, nb, PIECE_BLOCKS):
                m = min(PIECE_BLOCKS, nb - b0)
                reqs = np.array([(s, b) for b in range(b0, b0 + m, 2)], dtype=np.uint64)
                cells = ctx.gen_fake_cells(ctx.slot_seed(1, s), b0 * CPB, m * CPB, CELL).reshape(m, BLOCK)
                assert f.add(reqs, np.ascontiguousarray(cells[::2]).reshape(-1), fake.block_proofs(reqs)[1])[1] == len(reqs)
        fake.free()
        half = n_slots * ((nb + 1) // 2)
        assert f.missing(0)[1] == n_slots * nb - half
        every = np.array([(s, b) for s in range(n_slots) for b in range(0, nb, 2)], dtype=np.uint64)
        assert (f.block_proofs(every, statuses_only=True) == pkg.FILL_PROOF_OK).all()
        ckpt, nckpt = os.path.join(d, "session.ckpt"), os.path.join(d, "session.nodes")

        def base(trust):
            def go():
                r = ctx.fill_resume(cfg, roots, ckpt, trust_files=trust)
                r.keep_nodes()
                return r
            dt, r = timed(go)
            ok = r.n_dropped == 0 and r.missing(0)[1] == n_slots * nb - half
            r.free()
            return dt, ok

        def nodes(trust):
            dt, r = timed(lambda: ctx.fill_resume_nodes(cfg, roots, nckpt, trust_files=trust))
            ok = r.n_dropped == 0 and r.n_unproved == 0 and r.n_rejected == 0 and r.n_restored > 0 and r.missing(0)[1] == n_slots * nb - half
            record.setdefault("restored_rows_" + name, r.n_restored)
            r.free()
            return dt, ok

        f.save(ckpt)
        f.save_nodes(nckpt)
        r = ctx.fill_resume_nodes(cfg, roots, nckpt, trust_files=True)          # the resumed session serves what the saved one served
        assert (r.block_proofs(every, statuses_only=True) == pkg.FILL_PROOF_OK).all()
        r.free()
        legs = {
            "save": lambda: (timed(lambda: f.save(ckpt))[0], True),
            "save_nodes": lambda: (timed(lambda: f.save_nodes(nckpt))[0], True),
            "base_trust": lambda: base(True),
            "nodes_trust": lambda: nodes(True),
            "base_recheck": lambda: base(False),
            "nodes_recheck": lambda: nodes(False),
        }
        times = {k: [] for k in legs}
        for k, fn in legs.items():                               # warm-up
            assert fn()[1], k
        for _ in range(a.repeats):
            for k, fn in legs.items():
                dt, ok = fn()
                assert ok, k
                times[k].append(dt)
        med = {k: statistics.median(v) for k, v in times.items()}
        out = {"workload": "%d slot file(s) x %d MiB (2^%d cells x 2048 B, 64 KiB blocks), every second block present, every row known, page-cached" %
               (n_slots, n_cells * CELL >> 20, n_cells.bit_length() - 1),
               "blocks_present": half, "depth": (nb - 1).bit_length() or 1,
               "checkpoint_MiB": round(os.path.getsize(ckpt) / 2**20, 3), "checkpoint_with_nodes_MiB": round(os.path.getsize(nckpt) / 2**20, 3)}
        out.update({k + "_s": round(v, 5) for k, v in med.items()})
        out.update({k + "_spread": round((max(v) - min(v)) / med[k], 4) for k, v in times.items()})
        out["save_nodes_over_save"] = round(med["save_nodes"] / med["save"], 3)
        out["nodes_trust_minus_base_ms"] = round((med["nodes_trust"] - med["base_trust"]) * 1e3, 3)
        out["nodes_recheck_over_base"] = round(med["nodes_recheck"] / med["base_recheck"], 4)
        f.free()
        shutil.rmtree(d)
        return out

    try:
        record["slots"] = leg("slots", a.slots, (a.slot_mib << 20) // CELL)
        if a.deep_log2:
            record["deep"] = leg("deep", 1, 1 << a.deep_log2)
    finally:
        ctx.close()
        shutil.rmtree(a.dir, ignore_errors=True)
    line = json.dumps(record)
    print(line)
    if a.out:
        args = ["--slots %d" % a.slots, "--slot-mib %d" % a.slot_mib, "--deep-log2 %d" % a.deep_log2, "--repeats %d" % a.repeats]
        with open(a.out, "w") as fh:
            fh.write("tools/fill_node_ckpt_rate.py on one MI355X (%s; medians of alternated save / save_nodes / base_trust / nodes_trust / "
                     "base_recheck / nodes_recheck rounds after a warm-up, spread = (max - min) / median of the rounds; slot files "
                     "page-cached):\n%s\n" % (" ".join(args), line))


if __name__ == "__main__":
    main()
