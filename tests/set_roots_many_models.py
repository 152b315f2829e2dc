"""Plain references for cp2_datasets_set_roots_many: the layer sizes and tree-major offsets of a dataset tree, the cut of the requests
into chunks, the per-level prefix tables k_compress_layer_ragged reads and the lane -> (tree, node) search through them.

It restates csrc/set_roots_plan.hpp and what csrc/kernels.hpp says of launch_compress_layers_ragged; none of it shares code with the
product.  tests/test_set_roots_many_cpu.py holds the sizes against the oracle's Merkle tree and the plan against brute force, and compares
the product's plan with this one; tests/test_gpu_set_roots_many_unit.py feeds these tables to the launcher."""
import collections

import numpy as np


def layer_sizes(n):
    """rows of every layer of a tree over n >= 1 leaves, bottom first: the bottom layer is compressed once even for a singleton"""
    sizes, m = [n], n
    while True:
        m = (m + 1) // 2
        sizes.append(m)
        if m == 1:
            return sizes


def levels(n):
    return len(layer_sizes(n)) - 1


def total(n):
    return sum(layer_sizes(n))


def layer_off(n, k):
    return sum(layer_sizes(n)[:k])


Chunk = collections.namedtuple("Chunk", "first count rows")


def chunks(n_slots, bound):
    """consecutive requests while their trees' bytes stay within bound; a larger request is alone"""
    out = []
    for i, n in enumerate(n_slots):
        rows = total(n)
        if not out or (out[-1][2] + rows) * 32 > bound:
            out.append([i, 0, 0])
        out[-1][1] += 1
        out[-1][2] += rows
    return [Chunk(*c) for c in out]


Plan = collections.namedtuple("Plan", "tree_tab prefix tree_of level_off level_cnt level_work rows")


def plan(n_slots):
    """the tables of one chunk: tree_tab [(first row, n)], and per level the trees that have a layer k + 1 with the running sum of those
    layers' sizes"""
    tab, at = [], 0
    for n in n_slots:
        tab.append((at, n))
        at += total(n)
    prefix, tree_of, off, cnt, work = [], [], [], [], []
    for k in range(max([levels(n) for n in n_slots], default=0)):
        off.append(len(prefix))
        s = 0
        for r, n in enumerate(n_slots):
            if levels(n) > k:
                s += layer_sizes(n)[k + 1]
                prefix.append(s)
                tree_of.append(r)
        cnt.append(len(prefix) - off[-1])
        work.append(s)
    return Plan(tab, prefix, tree_of, off, cnt, work, at)


def trips(cnt):
    s = 0
    while (1 << s) < cnt:
        s += 1
    return s


def find(prefix, t):
    """the kernel's search: the entry of lane t, in trips(len(prefix)) steps whatever t is"""
    lo, cnt = 0, len(prefix)
    for s in reversed(range(trips(cnt))):
        mid = lo + (1 << s)
        if mid < cnt and prefix[mid - 1] <= t:
            lo = mid
    return lo


def lane(p, k, t):
    """(tree, node of layer k + 1) of lane t of level k"""
    pre = p.prefix[p.level_off[k]:p.level_off[k] + p.level_cnt[k]]
    e = find(pre, t)
    return p.tree_of[p.level_off[k] + e], t - (pre[e - 1] if e else 0)


def describe(n_slots, bound):
    return "bound %d\nn %s\n" % (bound, " ".join(str(n) for n in n_slots))


def expected(n_slots, bound):
    """what tests/host_check/set_roots_plan_check.cpp prints for the call"""
    out = []
    for c in chunks(n_slots, bound):
        p = plan(n_slots[c.first:c.first + c.count])
        out.append("chunk %d %d rows %d levels %d" % (c.first, c.count, c.rows, len(p.level_off)))
        out.append("trees " + " ".join("%d:%d" % t for t in p.tree_tab))
        for k in range(len(p.level_off)):
            a, b = p.level_off[k], p.level_off[k] + p.level_cnt[k]
            out.append("level %d off %d cnt %d work %d trips %d entries %s" % (
                k, a, p.level_cnt[k], p.level_work[k], trips(p.level_cnt[k]), " ".join("%d:%d" % e for e in zip(p.tree_of[a:b], p.prefix[a:b]))))
    return "\n".join(out) + "\n"


def ragged_tables(p):
    """the plan as the arrays the launcher takes"""
    return (np.asarray(p.tree_tab, dtype=np.uint64).reshape(-1), np.asarray(p.prefix, dtype=np.uint64), np.asarray(p.tree_of, dtype=np.uint32),
            np.asarray(p.level_off, dtype=np.uint64), np.asarray(p.level_cnt, dtype=np.uint64), np.asarray(p.level_work, dtype=np.uint64))
