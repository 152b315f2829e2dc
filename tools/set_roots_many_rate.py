"""Rate of cp2_datasets_set_roots_many against the loop over cp2_dataset_set_roots it replaces, and of its level kernel against
k_compress_layer on the same leaves.

Data (defaults = tools/build_many_rate.py's shape): --slots 4096 slot files of --slot-mib MiB (2048-byte cells, 64 KiB blocks), written
once; 4096 one-slot compact datasets of the 4096-slot configuration, built with cp2_datasets_build_many.  What is timed never reads the
slot data, so the slot size only sets how long the preparation takes.  Every dataset is handed all 4096 slot roots.  Legs, timed in one
process over the same datasets (a dataset that has a tree gets the new one, so every round does the whole work):
  (a) loop    cp2_dataset_set_roots of each of the 4096 datasets, one call after the other: existing code, the yardstick
  (b) many    one cp2_datasets_set_roots_many of the same 4096 requests
  (c) device  between device synchronisations, on the same 4096 x 4096 leaves already on the device: the ragged level launches
              (launch_compress_layers_ragged through the forwarder of tests/device_check, trees tree-major) against cp2_merkle_trees_dev
              with nseg = 4096 (k_compress_layer, trees layer-major, leaves in place); the 4096 roots of the two must be equal: asserted
  (d) mixed   one cp2_datasets_set_roots_many of 4096 one-slot datasets cycling through --mixed n_slots (1, 3, 64, 100, 1000, 4096), and
              the loop over the same, as measured
A warm-up of every leg first ((a) over the first --warm-loop datasets only), then --repeats rounds of (a), (b) and --device-repeats of
the two sides of (c), alternated; medians.  DONE when the ragged levels take <= (1 + 0.10 + the relative spread of the k_compress_layer
rounds) x the k_compress_layer time: both sides do the same compressions in the same number of launches and the ragged side adds the
table look-up; the margin is the one tools/build_many_rate.py and tools/scrub_many_rate.py use.  (a) / (b) is recorded as measured, with
the call's CP2_TRACE line (upload, levels, download, commit) from one more untimed call beside it.  Prints one JSON line and, with --out,
writes it with a heading.

    python tools/set_roots_many_rate.py [--slots 4096] [--slot-mib 8] [--repeats 2] [--device-repeats 5] [--warm-loop 256] [--dir D] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import set_roots_many_models as M  # noqa: E402
from build_many_rate import write_files  # noqa: E402

CELL, BLOCK = 2048, 65536
UNIT = os.path.join(ROOT, "tests", "device_check", "libset_roots_many_unit.so")


def caught_trace(f, word):
    """f() with CP2_TRACE set and the library's stderr caught: the trace lines that hold `word`"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tf:
        os.dup2(tf.fileno(), 2)
        os.environ["CP2_TRACE"] = "1"
        try:
            f()
        finally:
            del os.environ["CP2_TRACE"]
            os.dup2(keep, 2)
            os.close(keep)
        tf.seek(0)
        return [ln.strip() for ln in tf.read().decode(errors="replace").splitlines() if "[cp2 trace]" in ln and word in ln]


def device_leg(pkg, ctx, n_trees, n_leaves, repeats):
    """(c): seconds of the ragged level launches and of cp2_merkle_trees_dev (k_compress_layer) over the same leaves, per round"""
    import torch
    lib = ctypes.CDLL(UNIT)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.srm_compress_layers_ragged.restype, lib.srm_compress_layers_ragged.argtypes = ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, sz]
    total = M.total(n_leaves)
    gen = torch.Generator(device="cuda").manual_seed(11)
    leaves = torch.randint(0, 256, (n_trees, n_leaves, 32), dtype=torch.uint8, device="cuda", generator=gen)
    leaves[:, :, 31] = 0                                                        # field elements: below 2^248
    flat = torch.zeros((total * n_trees, 32), dtype=torch.uint8, device="cuda")      # layer-major: layer k of every tree, then layer k + 1
    flat[:n_trees * n_leaves] = leaves.view(-1, 32)
    ragged = torch.zeros((n_trees, total, 32), dtype=torch.uint8, device="cuda")     # tree-major: every layer of tree r, then tree r + 1
    ragged[:, :n_leaves] = leaves
    del leaves
    tab, prefix, tree_of, off, cnt, work = M.ragged_tables(M.plan([n_leaves] * n_trees))
    d_tab, d_prefix, d_tree = (torch.from_numpy(x.view(np.uint8).copy()).cuda() for x in (tab, prefix, tree_of))

    def run_ragged():
        st = lib.srm_compress_layers_ragged(ragged.data_ptr(), d_tab.data_ptr(), d_prefix.data_ptr(), d_tree.data_ptr(), off.ctypes.data,
                                            cnt.ctypes.data, work.ctypes.data, len(off))
        assert st == 0, st

    def run_layer():
        ctx.merkle_trees_dev(flat.data_ptr(), n_leaves, n_trees, flat.data_ptr())

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    timed(run_ragged), timed(run_layer)                                          # warm-up
    rounds = {"ragged": [], "layer": []}
    for _ in range(repeats):
        rounds["ragged"].append(timed(run_ragged))
        rounds["layer"].append(timed(run_layer))
    roots_layer = flat[(total - 1) * n_trees:].cpu().numpy()
    roots_ragged = ragged[:, total - 1].cpu().numpy()
    assert np.array_equal(roots_layer, roots_ragged), "the roots of the ragged levels differ from k_compress_layer's"
    return rounds, len(off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--slot-mib", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--device-repeats", type=int, default=5)
    ap.add_argument("--warm-loop", type=int, default=256)
    ap.add_argument("--mixed", default="1,3,64,100,1000,4096")
    ap.add_argument("--dir", default=None, help="where the slot files go (default: a temporary directory, removed at the end)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = g.load_package()
    ctx = pkg.Context(0)
    d = tempfile.mkdtemp(prefix="set_roots_many_rate_", dir=a.dir)
    n, cells = a.slots, (a.slot_mib << 20) // CELL
    try:
        base = os.path.join(d, "slot_")
        write_files(base, n, cells * CELL)

        def config(n_slots):
            return pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (n - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=n_slots, nCells=cells,
                                   nSamples=100, seed=1, file=base)

        ctx.set_keep_trees(2)
        try:
            many = ctx.build_many([(config(n), k, 1) for k in range(n)])
            sizes = [min(n, int(x)) for x in a.mixed.split(",")]
            mixed = ctx.build_many([(config(sizes[k % len(sizes)]), k % sizes[k % len(sizes)], 1) for k in range(n)])
        finally:
            ctx.set_keep_trees(-1)
        all_roots = np.concatenate([ds.local_roots() for ds in many])
        assert all_roots.shape == (n, 32) and len({bytes(r) for r in all_roots}) == n
        mixed_roots = [all_roots[:int(ds.cfg.n_slots)] for ds in mixed]

        def loop(datasets, roots):
            for ds, r in zip(datasets, roots):
                ds.set_roots(r)

        def timed(f):
            ctx.sync()
            t = time.perf_counter()
            out = f()
            return time.perf_counter() - t, out

        every = [all_roots] * n
        legs = (("loop", lambda k=n: loop(many[:k], every[:k])), ("many", lambda: ctx.set_roots_many(many, every)))
        timed(lambda: legs[0][1](max(1, min(n, a.warm_loop))))                   # warm-up
        timed(legs[1][1])
        rounds = {"loop": [], "many": []}
        for _ in range(a.repeats):
            s, _ = timed(legs[0][1])
            rounds["loop"].append(s)
            want = [many[k].root().tobytes() for k in (0, n // 2, n - 1)]
            s, own = timed(legs[1][1])
            rounds["many"].append(s)
            assert own.all() and [many[k].root().tobytes() for k in (0, n // 2, n - 1)] == want, "the one pass differs from the loop"
        med = {k: statistics.median(v) for k, v in rounds.items()}
        # (d) mixed n_slots: the one call, then the loop over the same
        timed(lambda: ctx.set_roots_many(mixed, mixed_roots))
        d_many = statistics.median(timed(lambda: ctx.set_roots_many(mixed, mixed_roots))[0] for _ in range(a.repeats))
        got = [mixed[k].root().tobytes() for k in range(0, n, max(1, n // 64))]
        d_loop = statistics.median(timed(lambda: loop(mixed, mixed_roots))[0] for _ in range(a.repeats))
        assert got == [mixed[k].root().tobytes() for k in range(0, n, max(1, n // 64))], "mixed: the one pass differs from the loop"
        trace = caught_trace(lambda: ctx.set_roots_many(many, every), "set roots many:")
        trace_mixed = caught_trace(lambda: ctx.set_roots_many(mixed, mixed_roots), "set roots many:")
        for ds in many + mixed:
            ds.free()
        ctx.trim()
        # (c) the device part alone
        dev, levels = device_leg(pkg, ctx, n, n, a.device_repeats)
        m_r, m_l = statistics.median(dev["ragged"]), statistics.median(dev["layer"])
        spread = (max(dev["layer"]) - min(dev["layer"])) / m_l
        margin = 0.10 + spread
        record = {
            "workload": "%d one-slot compact datasets of a %d-slot configuration (slot files of %d MiB), every one given all %d roots; one box's figures" % (n, n, a.slot_mib, n),
            "repeats": a.repeats,
            "a_loop_s": round(med["loop"], 4), "b_many_s": round(med["many"], 4), "a_over_b_time": round(med["loop"] / med["many"], 2),
            "a_ms_per_dataset": round(med["loop"] / n * 1e3, 4), "b_ms_per_dataset": round(med["many"] / n * 1e3, 4),
            "rounds_s": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
            "b_trace": trace,
            "c_levels": levels, "c_ragged_s": round(m_r, 5), "c_compress_layer_s": round(m_l, 5),
            "c_rounds_s": {k: [round(x, 5) for x in v] for k, v in dev.items()},
            "c_compress_layer_spread_between_rounds": round(spread, 3), "margin": round(margin, 3),
            "c_ragged_over_compress_layer_time": round(m_r / m_l, 3), "c_ragged_within_margin": bool(m_r <= m_l * (1 + margin)),
            "d_mixed_n_slots": sizes, "d_many_s": round(d_many, 4), "d_loop_s": round(d_loop, 4), "d_loop_over_many_time": round(d_loop / d_many, 2),
            "d_trace": trace_mixed,
        }
    finally:
        shutil.rmtree(d, ignore_errors=True)
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/set_roots_many_rate.py on one MI355X (%s; one box's figures; medians of alternated rounds after a warm-up):\n%s\n" %
                    (" ".join(sys.argv[1:]) or "defaults", line))
    if not record["c_ragged_within_margin"]:
        sys.exit("(c) the ragged levels' %.5f s are not within %.3f of k_compress_layer's %.5f s" % (m_r, record["margin"], m_l))


if __name__ == "__main__":
    main()
