"""Models for tests/test_gpu_fill_resume.py, numpy and plain Python only: what k_block_root_recheck leaves behind, and the documented layout
of a fill checkpoint (csrc/fill_checkpoint.hpp) read and written without the library -- the checksum included."""
import struct

import numpy as np

M64 = (1 << 64) - 1
MAGIC = b"CP2FILL1"
WORDS = ("cell_size", "block_size", "n_cells", "n_slots", "first_slot", "n_local", "source", "seed", "file_base_len", "n_blocks")
SRC_FAKE, SRC_FILE = 0, 1


# ---- k_block_root_recheck ----------------------------------------------------------------------------------------------------------------
def recheck_model(fresh, dest, layer0, n_rows):
    """(verdict uint32[n], layer0 after): lane i compares fresh[i] with layer0[dest[i]]; 1 and the row zeroed where they differ; a row at or
    past n_rows is 1 and nothing is touched.  layer0 may hold more than n_rows rows: those stay as they are."""
    out = layer0.copy()
    verdict = np.ones(len(dest), dtype=np.uint32)
    for i, r in enumerate(int(x) for x in dest):
        if r >= n_rows:
            continue
        if np.array_equal(fresh[i], layer0[r]):
            verdict[i] = 0
        else:
            out[r] = 0
    return verdict, out


# ---- the checksum of the library's files (csrc/checksum64.hpp), one update over the whole payload -----------------------------------------
def checksum64(data):
    h = [0x9e3779b97f4a7c15, 0xc2b2ae3d27d4eb4f, 0x165667b19e3779f9, 0x27d4eb2f165667c5]
    n = len(data)
    whole = n // 32 * 32
    for i in range(0, whole, 32):
        w = struct.unpack_from("<4Q", data, i)
        for k in range(4):
            x = ((h[k] ^ w[k]) * 0x100000001b3) & M64
            h[k] = ((x << 29) | (x >> 35)) & M64
    r = (h[0] ^ (h[1] * 3) ^ (h[2] * 5) ^ (h[3] * 7) ^ n) & M64
    for b in data[whole:]:
        r = ((r ^ b) * 0x100000001b3) & M64
    r ^= r >> 33
    r = (r * 0xff51afd7ed558ccd) & M64
    r ^= r >> 33
    return r


# ---- the checkpoint file ---------------------------------------------------------------------------------------------------------------------
def parse_checkpoint(raw):
    """The fields of a checkpoint as a dict: the ten header words by name, file_base (bytes), roots uint8[n_local, 32], bits (list of 0 / 1 per
    block, local-major), layer0 uint8[total, 32].  Asserts magic, sizes, padding and checksum."""
    assert raw[:8] == MAGIC
    c = dict(zip(WORDS, struct.unpack_from("<10Q", raw, 8)))
    total = c["n_local"] * c["n_blocks"]
    assert c["n_blocks"] == c["n_cells"] // (c["block_size"] // c["cell_size"])
    at = 88
    c["file_base"] = raw[at:at + c["file_base_len"]]
    pad = (c["file_base_len"] + 7) // 8 * 8
    assert raw[at + c["file_base_len"]:at + pad] == bytes(pad - c["file_base_len"])
    at += pad
    c["roots"] = np.frombuffer(raw, dtype=np.uint8, count=c["n_local"] * 32, offset=at).reshape(-1, 32).copy()
    at += c["n_local"] * 32
    words = (total + 63) // 64
    bitmap = struct.unpack_from("<%dQ" % words, raw, at)
    at += words * 8
    c["bits"] = [(bitmap[g >> 6] >> (g & 63)) & 1 for g in range(total)]
    assert all(bitmap[g >> 6] >> (g & 63) & 1 == 0 for g in range(total, words * 64))
    c["layer0"] = np.frombuffer(raw, dtype=np.uint8, count=total * 32, offset=at).reshape(-1, 32).copy()
    at += total * 32
    assert len(raw) == at + 8 and struct.unpack_from("<Q", raw, at)[0] == checksum64(raw[:at])
    return c


def write_checkpoint(c):
    """The bytes of a checkpoint with the fields of `c` (as parse_checkpoint returns them), by the documented layout, checksum valid."""
    total = c["n_local"] * c["n_blocks"]
    base = bytes(c["file_base"])
    out = bytearray(MAGIC)
    out += struct.pack("<10Q", *[len(base) if w == "file_base_len" else c[w] for w in WORDS])
    out += base + bytes((len(base) + 7) // 8 * 8 - len(base))
    out += np.ascontiguousarray(c["roots"], dtype=np.uint8).tobytes()
    bitmap = [0] * ((total + 63) // 64)
    for g, b in enumerate(c["bits"]):
        if b:
            bitmap[g >> 6] |= 1 << (g & 63)
    out += struct.pack("<%dQ" % len(bitmap), *bitmap)
    out += np.ascontiguousarray(c["layer0"], dtype=np.uint8).tobytes()
    out += struct.pack("<Q", checksum64(bytes(out)))
    return bytes(out)
