"""Rate of cp2_fill_adopt against cp2_fill_resume's re-check and cp2_dataset_scrub over the same slot files, and the time of a judgement alone.

An adopt reads every absent block its slot files cover, hashes it on repair's data path and keeps the block roots (the re-check's reads and
data path), then builds the tree above them and keeps what reaches a node the session knows (k_adopt_layer per layer, k_adopt_resolve).  A
resume with the re-check reads and hashes the same bytes and compares each block root with a kept row; cp2_dataset_scrub reads them through
the builders' ingestion pipe.  All run over the same files, page-cached (they were written moments before), in the same process.
  slots   --slots 128 slots of --slot-mib 8 MiB (2^12 cells x 2048 B, 64 KiB blocks: 128 blocks a slot), filled from fake cells into slot
          files under --dir
  deep    one slot of 2^--deep-log2 cells (2^22: 8 GiB, 131 072 blocks); --deep-log2 0 leaves it out
Legs, alternated for --repeats rounds after a warm-up of each:
  adopt           a fresh node-keeping session over the intact files: every block read, every block adopted from the stated roots alone
  resume_recheck  cp2_fill_resume of a checkpoint that calls every block present, with the re-check
  scrub           cp2_dataset_scrub of the dataset the filled session became
  adopt_no_read   CP2_ADOPT_NO_READ in a session whose stated roots are wrong, after one reading adopt: every block is a remembered
                  candidate and stays one, so each call is the two kernels over the whole tree plus the flag bytes up and down
adopt_over_recheck = recheck_s / adopt_s (the two share the read path: parity is expected); adopt_over_scrub = scrub_s / adopt_s.  Prints
one JSON line and, with --out, writes it with a heading.

    python tools/fill_adopt_rate.py --dir DIR [--slots 128] [--slot-mib 8] [--deep-log2 22] [--repeats 2] [--out FILE]
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
        total = n_slots * nb
        geom = dict(maxDepth=32, maxLog2NSlots=max(1, (n_slots - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=n_slots, nCells=n_cells,
                    nSamples=100, seed=1)
        fake = build(pkg.make_config(**geom))                     # the roots and paths a peer would send; the files hold the same bytes
        roots = fake.local_roots()
        cfg = pkg.make_config(file=os.path.join(d, "slot"), **geom)
        f = ctx.fill(cfg, roots)
        for s in range(n_slots):
            for b0 in range(0, nb, PIECE_BLOCKS):
                m = min(PIECE_BLOCKS, nb - b0)
                reqs = np.array([(s, b) for b in range(b0, b0 + m)], dtype=np.uint64)
                cand = ctx.gen_fake_cells(ctx.slot_seed(1, s), b0 * CPB, m * CPB, CELL).reshape(-1)
                assert f.add(reqs, cand, fake.block_proofs(reqs)[1])[1] == m
        fake.free()
        assert f.missing(0)[1] == 0
        ckpt = os.path.join(d, "session.ckpt")
        f.save(ckpt)
        f.free()
        ds = ctx.fill_resume(cfg, roots, ckpt, trust_files=True).finish()      # the dataset whose scrub reads the same files

        def adopt():
            s = ctx.fill(cfg, roots)
            s.keep_nodes()
            dt, r = timed(s.adopt)
            ok = r == (total, total) and s.missing(0)[1] == 0
            s.free()
            return dt, ok

        def resume():
            dt, r = timed(lambda: ctx.fill_resume(cfg, roots, ckpt))
            ok = r.n_dropped == 0 and r.missing(0)[1] == 0
            r.free()
            return dt, ok

        wrong = np.array(roots, copy=True)
        wrong[:, 0] ^= 1                                          # no stated root is the files': every candidate stays one
        stuck = ctx.fill(cfg, wrong)
        stuck.keep_nodes()
        assert stuck.adopt() == (total, 0)
        legs = {
            "adopt": adopt,
            "resume_recheck": resume,
            "scrub": lambda: (lambda r: (r[0], r[1][2] == 0))(timed(ds.scrub)),
            "adopt_no_read": lambda: (lambda r: (r[0], r[1] == (0, 0)))(timed(lambda: stuck.adopt(no_read=True))),
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
        data_gb = n_slots * n_cells * CELL / 1e9
        out = {"workload": "%d slot file(s) x %d MiB (2^%d cells x 2048 B, 64 KiB blocks), every block absent and intact on disk, page-cached" %
               (n_slots, n_cells * CELL >> 20, n_cells.bit_length() - 1), "blocks": total}
        out.update({k + "_s": round(v, 5) for k, v in med.items()})
        out["adopt_GBps"] = round(data_gb / med["adopt"], 2)
        out["resume_recheck_GBps"] = round(data_gb / med["resume_recheck"], 2)
        out["scrub_GBps"] = round(data_gb / med["scrub"], 2)
        out["adopt_over_recheck"] = round(med["resume_recheck"] / med["adopt"], 3)
        out["adopt_over_scrub"] = round(med["scrub"] / med["adopt"], 3)
        stuck.free()
        ds.free()
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
            fh.write("tools/fill_adopt_rate.py on one MI355X (%s; medians of alternated adopt / resume_recheck / scrub / adopt_no_read rounds "
                     "after a warm-up; slot files page-cached):\n%s\n" % (" ".join(args), line))


if __name__ == "__main__":
    main()
