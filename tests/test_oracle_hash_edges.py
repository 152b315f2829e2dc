"""CPU suite: pins the reference of the GPU staging sweep (tests/test_gpu_kernel_edges.py).  That sweep takes every expected digest
from the C oracle's hash_cells; here the C oracle is held against the Python big-int restatement at the sizes where the byte
stream's framing changes: every size up to 256, then every residue of the size mod 124 (lcm of the 4-byte dword and the 31-byte
chunk) at which the data end, the 0x01 terminator or the sponge's pad sits next to a chunk or a permutation boundary."""
import numpy as np

EDGE_RESIDUES_124 = (0, 1, 29, 30, 31, 61, 62, 63, 92, 93, 123)
MAX_SIZE = 6200


def edge_sizes():
    return list(range(257)) + [s for s in range(257, MAX_SIZE + 1) if s % 124 in EDGE_RESIDUES_124]


def test_edge_size_list_is_what_the_sweep_relies_on():
    sizes = edge_sizes()
    assert sizes == sorted(set(sizes)) and sizes[:257] == list(range(257)) and sizes[-1] <= MAX_SIZE
    assert {s % 124 for s in sizes if s > 256} == set(EDGE_RESIDUES_124)
    for r in EDGE_RESIDUES_124:                                  # each residue all the way up: one size per 124 bytes
        assert len([s for s in sizes if s > 256 and s % 124 == r]) == len(range(257 + (r - 257) % 124, MAX_SIZE + 1, 124))
    assert {s % 31 for s in sizes} == set(range(31)) and {s % 4 for s in sizes if s % 31 in (0, 29, 30)} == {0, 1, 2, 3}


def test_c_hash_cells_matches_python_at_every_framing_edge(oracle):
    C, P = oracle
    rng = np.random.default_rng(0x5EED)
    bad = []
    for s in edge_sizes():
        cell = rng.integers(0, 256, size=s, dtype=np.uint8)
        if s % 3 == 0 and s:                                     # a last byte that is itself 0x01 / 0x00 / 0xFF next to the terminator
            cell[-1] = (0x01, 0x00, 0xFF)[(s // 3) % 3]
        got = C.hash_cells(cell, s) if s else C.hash_bytes(b"").reshape(1, 32)
        if C.array_to_felts(got) != [P.hash_cell(cell.tobytes(), s)]:
            bad.append(s)
    assert not bad, "C.hash_cells differs from the Python oracle at cell sizes %s" % bad


def test_c_hash_cells_is_per_cell_and_thread_count_blind(oracle):
    """The sweep hashes many cells per size, on several threads: cell i of a batch is the hash of cell i alone."""
    C, P = oracle
    rng = np.random.default_rng(0xCE11)
    for s in (1, 30, 31, 62, 123, 124, 125, 2047):
        cells = rng.integers(0, 256, size=(7, s), dtype=np.uint8)
        one = np.concatenate([C.hash_cells(cells[i], s) for i in range(7)])
        assert np.array_equal(C.hash_cells(cells, s, threads=1), one) and np.array_equal(C.hash_cells(cells, s, threads=3), one)
        assert C.array_to_felts(one[6]) == [P.hash_cell(cells[6].tobytes(), s)]
