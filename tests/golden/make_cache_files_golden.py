"""Writes the golden cache files of tests/golden/cache_files/ (needs the GPU): a tree cache ("CP2TREE3") of three fake-source slots and
the kept form ("CP2KEPT1") of a cached dataset build with the mode pinned to compact (2) and to roots only (0).  The fake source has no
stamps, so the bytes depend on the configuration alone.  Usage: make_cache_files_golden.py [directory]

The files in the repository were written by the commit BEFORE the cache-file module (csrc/cache_file.hpp) existed; the tests compare
what the library writes now with them, byte for byte."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g

# a small geometry with two blocks per slot (two cells per block): every file stays under 16 KiB
CONFIG = dict(maxDepth=8, maxLog2NSlots=2, cellSize=32, blockSize=64, nSlots=3, nCells=4, nSamples=3, seed=7)


def write(ctx, pkg, directory):
    """the three files, written by the library as it is now; returns {file name: slot roots as hex}"""
    c = CONFIG
    roots = {}
    t = ctx.slot_trees_fake(c["seed"], 0, c["nSlots"], c["cellSize"], c["blockSize"], c["nCells"])
    t.save(os.path.join(directory, "tree_3slots.cp2"))
    roots["tree_3slots.cp2"] = t.roots().tobytes().hex()
    t.free()
    try:
        for mode in (2, 0):
            name = "kept_mode%d.cp2" % mode
            path = os.path.join(directory, name)
            if os.path.exists(path):
                os.remove(path)
            ctx.set_keep_trees(mode)
            ds = ctx.dataset(pkg.make_config(**c), cache=path)
            assert ds.tree_mode == mode
            roots[name] = ds.local_roots().tobytes().hex()
            ds.free()
    finally:
        ctx.set_keep_trees(-1)
    return roots


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "cache_files")
    os.makedirs(out, exist_ok=True)
    pkg = g.load_package()
    ctx = pkg.Context(0)
    roots = write(ctx, pkg, out)
    with open(os.path.join(out, "config.json"), "w") as f:
        json.dump({"config": CONFIG, "slot_roots": roots}, f, indent=1, sort_keys=True)
        f.write("\n")
    for name in sorted(roots):
        print(name, os.path.getsize(os.path.join(out, name)), "bytes")
