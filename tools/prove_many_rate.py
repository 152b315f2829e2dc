"""Rate of proving many hosted slots of many datasets, each with its own entropy (cp2_proof_inputs_generate_many / _export_many),
against one cp2_proof_input_generate per slot and against the single-dataset batch.

Shape: configs[3] -- 4096 slots x 2^12 cells x 2048 B, 100 samples, maxDepth 32.  The full 4096-slot dataset is built once (its slot
roots are the "manifest"); then 4096 one-slot datasets (slot k of that dataset each, cp2_dataset_set_roots with the manifest's roots),
and 4096 distinct entropies.  For keep-trees modes 1 (every node) and 2 (compact), in one process, alternated, after a warm-up:
  many        cp2_proof_inputs_generate_many over the 4096 (one-slot dataset k, slot k, entropy k) requests
  loop        cp2_proof_input_generate per request
  batch       cp2_proof_inputs_generate_batch on the 4096-slot dataset, one entropy
and the same with JSON: cp2_proof_inputs_export_many / a loop of generate + cp2_proof_input_json / cp2_dataset_export_proof_inputs.
Prints one JSON line (median seconds per variant).

    python tools/prove_many_rate.py [--slots 4096] [--repeats 2] [--threads 16]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=1 << 12)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--modes", default="1,2")
    a = ap.parse_args()
    pkg = g.load_package()
    ctx = pkg.Context(0)
    L = ctx.L
    n = a.slots
    cfg = pkg.make_config(maxDepth=32, maxLog2NSlots=12, cellSize=2048, blockSize=65536, nSlots=n, nCells=a.cells, nSamples=100, seed=2024)
    rng = np.random.default_rng(1)
    ents = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ents[:, 31] &= 0x1f                                          # below r: what a caller would draw
    slots = np.arange(n, dtype=np.uint64)
    one_entropy = np.ascontiguousarray(ents[0])
    record = {"workload": "configs[3] shape: %d one-slot datasets (slot k each, roots from the full build) x 2^%d cells x 2048 B, "
                          "100 samples, maxDepth 32; one entropy per request" % (n, a.cells.bit_length() - 1),
              "repeats": a.repeats, "threads": a.threads}
    for mode in [int(m) for m in a.modes.split(",")]:
        ctx.set_keep_trees(mode)
        full = ctx.dataset(cfg)
        roots = full.local_roots()
        t0 = time.perf_counter()
        ones = []
        for k in range(n):
            d = ctx.dataset(cfg, k, 1)
            d.set_roots(roots)
            ones.append(d)
        build_s = time.perf_counter() - t0
        ctx.set_keep_trees(-1)
        hs = (ctypes.c_void_p * n)(*[d.h for d in ones])
        out = (ctypes.c_void_p * n)()
        paths_none = None
        total = ctypes.c_uint64()

        def free_all():
            for i in range(n):
                if out[i]:
                    L.cp2_proof_input_free(out[i])
                    out[i] = None

        def many():
            assert L.cp2_proof_inputs_generate_many(ctx.h, hs, slots.ctypes.data, ents.ctypes.data, n, out) == 0, L.cp2_last_error(ctx.h)
            free_all()

        def loop(json_too=False, count=n):
            h = ctypes.c_void_p()
            text, ln = ctypes.c_void_p(), ctypes.c_size_t()
            for k in range(count):
                assert L.cp2_proof_input_generate(ones[k].h, k, ents[k].ctypes.data, ctypes.byref(h)) == 0
                if json_too:
                    assert L.cp2_proof_input_json(h, ctypes.byref(text), ctypes.byref(ln)) == 0
                    L.cp2_free_buffer(text)
                L.cp2_proof_input_free(h)

        def batch():
            assert L.cp2_proof_inputs_generate_batch(full.h, slots.ctypes.data, n, one_entropy.ctypes.data, out) == 0
            free_all()

        def many_json():
            assert L.cp2_proof_inputs_export_many(ctx.h, hs, slots.ctypes.data, ents.ctypes.data, n, paths_none, a.threads, 0,
                                                  ctypes.byref(total)) == 0, L.cp2_last_error(ctx.h)

        def batch_json():
            assert L.cp2_dataset_export_proof_inputs(full.h, slots.ctypes.data, n, one_entropy.ctypes.data, None, a.threads, 0,
                                                     ctypes.byref(total)) == 0

        variants = {"many": many, "loop": loop, "batch": batch, "many_json": many_json, "loop_json": lambda: loop(True), "batch_json": batch_json}
        # warm-up: every variant once (the loops on 64 requests)
        for name, f in variants.items():
            f() if not name.startswith("loop") else loop(name == "loop_json", 64)
        # the many call's texts equal the per-call ones (a sample of requests)
        pis = ctx.proof_inputs_many([(ones[k], k, ents[k]) for k in range(0, n, max(1, n // 16))])
        for pi, k in zip(pis, range(0, n, max(1, n // 16))):
            assert pi.json() == ones[k].proof_input(k, ents[k]).json()
        del pis
        times = {k: [] for k in variants}
        for _ in range(a.repeats):
            for name, f in variants.items():
                ctx.sync()
                t = time.perf_counter()
                f()
                ctx.sync()
                times[name].append(time.perf_counter() - t)
        med = {k: statistics.median(v) for k, v in times.items()}
        record["mode%d" % mode] = {
            "seconds": {k: round(v, 4) for k, v in med.items()},
            "loop_over_many": round(med["loop"] / med["many"], 2), "many_over_batch": round(med["many"] / med["batch"], 2),
            "loop_json_over_many_json": round(med["loop_json"] / med["many_json"], 2),
            "many_json_over_batch_json": round(med["many_json"] / med["batch_json"], 2),
            "proofs_per_s_many": round(n / med["many"], 1), "json_bytes": total.value, "one_slot_builds_s": round(build_s, 2)}
        for d in ones:
            d.free()
        full.free()
        del ones, full
    print(json.dumps(record))


if __name__ == "__main__":
    main()
