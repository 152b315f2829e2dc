"""ctypes binding of libcodex_p2.so (include/codex_p2.h) for tests and bench.py.

This is glue, not the product: the product is the HIP library and its C ABI, with the C++ host
layer (`host/`) mirroring the reference's Nim interface.  The binding never computes a hash itself and
has no CPU fallback -- if the library is missing or no gfx950 GPU is usable it raises.

The directory name contains '-', so import it through `__graft_entry__.load_package()`.
"""
import ctypes
import os
import subprocess
import sys
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION_MAJOR, ABI_VERSION_MINOR = 1, 2      # CP2_ABI_VERSION_* of the include/codex_p2.h this binding was written against (tests keep them equal)
LIB_PATH = os.environ.get("CODEX_P2_LIB") or os.path.join(_HERE, "libcodex_p2.so")   # env override: kernel-variant A/B runs
CLI_PATH = os.path.join(_HERE, "cli")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "codex_p2.h")

CP2_OK = 0
FELT = 32


def _free_children(owner):
    """Datasets and tree batches live inside their context (device buffers, streams, the scratch pool): whatever of them is
    still alive when the context / multi handle is closed is freed FIRST, so a late `free()` (or a destructor) finds nothing
    left to touch -- the C ABI's rule ("free every dataset made through a handle before the handle") kept by the binding."""
    for child in list(getattr(owner, "_children", ())):
        try:
            child.free()
        except Exception:
            pass


def _finalizing(_is_finalizing=sys.is_finalizing):
    """True at interpreter shutdown (module globals may already be None there, hence the bound default)."""
    try:
        return _is_finalizing()
    except Exception:
        return True


class CodexP2Error(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__("%s failed: status %d%s" % (where, status, (" (" + detail + ")") if detail else ""))


class Config(ctypes.Structure):
    """cp2_config (GlobalConfig + DataSetConfig of reference/nim/proof_input/src/types.nim:82-101)."""
    _fields_ = [("max_depth", ctypes.c_int32), ("max_log2_nslots", ctypes.c_int32),
                ("cell_size", ctypes.c_uint64), ("block_size", ctypes.c_uint64),
                ("n_slots", ctypes.c_uint64), ("n_cells", ctypes.c_uint64),
                ("n_samples", ctypes.c_uint64), ("seed", ctypes.c_uint64),
                ("file_base", ctypes.c_char_p)]


def build(force=False, verbose=False):
    """Compile libcodex_p2.so and the cli twin in-tree with hipcc for gfx950."""
    args = ["make", "-C", _HERE] + (["-B"] if force else [])
    subprocess.check_call(args, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def load_library():
    """dlopen the in-tree library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm wheels bundle their own libamdhip64; two HIP runtimes in one process do not work
    # ("No HIP GPUs are available" from whichever comes second).  When torch is installed, load it first
    # so that this library binds to the runtime torch already mapped (same SONAME).
    import sys
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    # The entry points below are bound by name: the boundary's version is what tells a library built from another header
    # (include/codex_p2.h, CP2_ABI_VERSION_*).  Another major, or a minor older than this binding's, is refused.
    try:
        L.cp2_abi_version.restype, L.cp2_abi_version.argtypes = ctypes.c_int, []
        v = L.cp2_abi_version()
    except AttributeError:
        v = None
    if v is None:
        if not os.environ.get("CODEX_P2_LIB"):          # (A/B tooling may name an older library on purpose)
            raise RuntimeError("%s predates the versioned boundary (no cp2_abi_version): rebuild it" % LIB_PATH)
    elif (v >> 16) != ABI_VERSION_MAJOR or (v & 0xffff) < ABI_VERSION_MINOR:
        raise RuntimeError("%s has ABI version %d.%d, this binding was written against %d.%d (include/codex_p2.h)" %
                           (LIB_PATH, v >> 16, v & 0xffff, ABI_VERSION_MAJOR, ABI_VERSION_MINOR))
    vp, sz, u64, u32, i32, cp = (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
                                 ctypes.c_char_p)
    pvp = ctypes.POINTER(ctypes.c_void_p)
    sigs = {
        "cp2_init": (i32, [i32, pvp]),
        "cp2_free": (None, [vp]),
        "cp2_set_stream": (i32, [vp, vp]),
        "cp2_reset_stream": (i32, [vp]),
        "cp2_sync": (i32, [vp]),
        "cp2_strerror": (cp, [i32]),
        "cp2_last_error": (cp, [vp]),
        "cp2_device_is_native": (i32, [vp]),
        "cp2_check_environment": (i32, [cp, sz]),
        "cp2_abi_version": (i32, []),
        "cp2_set_ingest": (i32, [vp, i32, i32, sz]),
        "cp2_set_ingest_direct": (i32, [vp, i32]),
        "cp2_set_ingest_mapped": (i32, [vp, i32]),
        "cp2_trim": (i32, [vp]),
        "cp2_set_body_budget": (i32, [vp, sz, cp]),
        "cp2_set_keep_trees": (i32, [vp, i32]),
        "cp2_dataset_keeps_trees": (i32, [vp]),
        "cp2_permute_batch": (i32, [vp, vp, vp, sz]),
        "cp2_permute_batch_dev": (i32, [vp, vp, vp, sz]),
        "cp2_compress_batch": (i32, [vp, vp, u32, vp, sz]),
        "cp2_sponge2_felts": (i32, [vp, vp, sz, vp]),
        "cp2_sponge2_felts_batch": (i32, [vp, vp, sz, sz, vp]),
        "cp2_sponge2_felts_batch_dev": (i32, [vp, vp, sz, sz, vp]),
        "cp2_felts_per_bytes": (sz, [sz]),
        "cp2_bytes_to_felts": (i32, [vp, sz, vp]),
        "cp2_hash_cells": (i32, [vp, vp, sz, sz, vp]),
        "cp2_hash_cells_dev": (i32, [vp, vp, sz, sz, vp]),
        "cp2_hash_bytes": (i32, [vp, vp, sz, vp]),
        "cp2_merkle_total": (sz, [sz]),
        "cp2_merkle_num_layers": (sz, [sz]),
        "cp2_merkle_tree": (i32, [vp, vp, sz, vp, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
        "cp2_merkle_trees_dev": (i32, [vp, vp, sz, sz, vp]),
        "cp2_merkle_root": (i32, [vp, vp, sz, vp]),
        "cp2_slot_seed": (u64, [u64, u64]),
        "cp2_gen_fake_cells": (i32, [vp, u64, u64, sz, sz, vp]),
        "cp2_gen_fake_cells_dev": (i32, [vp, u64, u64, sz, sz, vp]),
        "cp2_cell_indices": (i32, [vp, vp, vp, u64, sz, vp]),
        "cp2_slot_trees_build_fake": (i32, [vp, u64, u64, sz, sz, sz, sz, pvp]),
        "cp2_slot_trees_build_fake_units": (i32, [vp, u64, u64, u64, sz, sz, sz, sz, pvp]),
        "cp2_slot_trees_build_file_units": (i32, [vp, cp, u64, u64, sz, sz, sz, sz, pvp]),
        "cp2_slot_trees_build_dev": (i32, [vp, vp, sz, sz, sz, sz, pvp]),
        "cp2_slot_trees_build_host": (i32, [vp, vp, sz, sz, sz, sz, pvp]),
        "cp2_slot_trees_free": (None, [vp]),
        "cp2_slot_trees_save": (i32, [vp, cp]),
        "cp2_slot_trees_load": (i32, [vp, cp, pvp]),
        "cp2_slot_trees_attach_cells": (i32, [vp, vp, vp]),
        "cp2_dataset_build_cached": (i32, [vp, ctypes.POINTER(Config), u64, u64, cp, pvp]),
        "cp2_slot_trees_count": (sz, [vp]),
        "cp2_slot_trees_depth": (sz, [vp]),
        "cp2_slot_trees_roots": (i32, [vp, vp]),
        "cp2_slot_trees_roots_dev": (vp, [vp]),
        "cp2_slot_trees_paths": (i32, [vp, sz, vp, sz, sz, vp, vp]),
        "cp2_dataset_build": (i32, [vp, ctypes.POINTER(Config), u64, u64, pvp]),
        "cp2_dataset_free": (None, [vp]),
        "cp2_dataset_local_roots": (i32, [vp, vp]),
        "cp2_dataset_set_roots": (i32, [vp, vp]),
        "cp2_dataset_root": (i32, [vp, vp]),
        "cp2_dataset_local_roots_dev": (vp, [vp]),
        "cp2_dataset_copy_local_roots_dev": (i32, [vp, vp]),
        "cp2_dataset_set_roots_dev": (i32, [vp, vp]),
        "cp2_dataset_range": (i32, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "cp2_dataset_ctx": (vp, [vp]),
        "cp2_multi_init": (i32, [ctypes.POINTER(ctypes.c_int), i32, pvp]),
        "cp2_multi_free": (None, [vp]),
        "cp2_multi_count": (i32, [vp]),
        "cp2_multi_device": (i32, [vp, i32]),
        "cp2_multi_ctx": (vp, [vp, i32]),
        "cp2_multi_last_error": (cp, [vp]),
        "cp2_multi_gather_mode": (cp, [vp]),
        "cp2_multi_set_policy": (i32, [vp, i32, u64]),
        "cp2_multi_set_split": (i32, [vp, ctypes.c_int64]),
        "cp2_multi_dataset_units_per_slot": (u64, [vp]),
        "cp2_shard_range": (None, [u64, i32, i32, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "cp2_multi_plan": (i32, [ctypes.POINTER(Config), i32, u64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(u64)]),
        "cp2_multi_dataset_build": (i32, [vp, ctypes.POINTER(Config), pvp]),
        "cp2_multi_dataset_build_cached": (i32, [vp, ctypes.POINTER(Config), cp, pvp]),
        "cp2_multi_dataset_build_streamed": (i32, [vp, ctypes.POINTER(Config), vp, i32, sz, pvp]),
        "cp2_multi_dataset_free": (None, [vp]),
        "cp2_multi_dataset_shards": (i32, [vp]),
        "cp2_multi_dataset_shard": (vp, [vp, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "cp2_multi_dataset_root": (i32, [vp, vp]),
        "cp2_multi_dataset_slot_roots": (i32, [vp, vp]),
        "cp2_multi_proof_input_generate": (i32, [vp, u64, vp, pvp]),
        "cp2_multi_dataset_export_proof_inputs": (i32, [vp, vp, sz, vp, cp, i32, sz, ctypes.POINTER(u64)]),
        "cp2_multi_dataset_export_streamed": (i32, [vp, cp, i32, ctypes.POINTER(u64)]),
        "cp2_multi_dataset_streamed_json": (i32, [vp, u64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz)]),
        "cp2_proof_input_generate": (i32, [vp, u64, vp, pvp]),
        "cp2_proof_inputs_generate_batch": (i32, [vp, vp, sz, vp, pvp]),
        "cp2_proof_inputs_write_json_batch": (i32, [pvp, sz, ctypes.POINTER(cp), i32, ctypes.POINTER(u64)]),
        "cp2_dataset_export_proof_inputs": (i32, [vp, vp, sz, vp, cp, i32, sz, ctypes.POINTER(u64)]),
        "cp2_dataset_build_streamed": (i32, [vp, ctypes.POINTER(Config), u64, u64, vp, i32, sz, pvp]),
        "cp2_dataset_export_streamed": (i32, [vp, cp, i32, ctypes.POINTER(u64)]),
        "cp2_dataset_streamed_json": (i32, [vp, u64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz)]),
        "cp2_proof_input_free": (None, [vp]),
        "cp2_proof_input_roots": (i32, [vp, vp, vp, vp]),
        "cp2_proof_input_nsamples": (sz, [vp]),
        "cp2_proof_input_cell_indices": (vp, [vp]),
        "cp2_proof_input_cell_data": (vp, [vp]),
        "cp2_proof_input_merkle_paths": (vp, [vp]),
        "cp2_proof_input_slot_proof": (vp, [vp]),
        "cp2_proof_input_leaf_hashes": (vp, [vp]),
        "cp2_proof_input_create": (i32, [ctypes.POINTER(Config), u64, vp, vp, vp, vp, sz, vp, vp, vp, vp, pvp]),
        "cp2_proof_input_write_json": (i32, [vp, cp]),
        "cp2_proof_input_json": (i32, [vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz)]),
        "cp2_free_buffer": (None, [vp]),
        "cp2_write_circom_main": (i32, [ctypes.POINTER(Config), cp]),
        "cp2_proof_input_parse_json": (i32, [ctypes.POINTER(Config), vp, sz, pvp, vp, sz]),
        "cp2_proof_input_shape": (i32, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "cp2_proof_input_cell_felts": (i32, [vp, vp]),
        "cp2_proof_inputs_verify": (i32, [vp, vp, sz, vp, vp]),
        "cp2_proof_inputs_generate_many": (i32, [vp, vp, vp, vp, sz, pvp]),
        "cp2_proof_inputs_export_many": (i32, [vp, vp, vp, vp, sz, ctypes.POINTER(cp), i32, sz, ctypes.POINTER(u64)]),
        "cp2_dataset_scrub": (i32, [vp, u64, u64, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_int)]),
        "cp2_multi_dataset_scrub": (i32, [vp, u64, u64, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_int)]),
        "cp2_datasets_scrub_many": (i32, [vp, vp, sz, vp, sz, ctypes.POINTER(sz), vp, vp]),
        "cp2_datasets_build_many": (i32, [vp, vp, vp, sz, vp]),
        "cp2_datasets_set_roots_many": (i32, [vp, vp, vp, sz, vp]),
        "cp2_dataset_repair_blocks": (i32, [vp, vp, vp, sz, i32, cp, vp, ctypes.POINTER(sz)]),
        "cp2_multi_dataset_repair_blocks": (i32, [vp, vp, vp, sz, i32, cp, vp, ctypes.POINTER(sz)]),
        "cp2_block_proof_depth": (sz, [sz, sz, sz]),
        "cp2_dataset_block_proofs": (i32, [vp, vp, sz, vp, vp]),
        "cp2_blocks_verify": (i32, [vp, sz, sz, sz, vp, sz, vp, vp, vp, sz, vp, vp]),
        "cp2_block_multiproof_rows": (sz, [sz, sz, sz, vp, sz]),
        "cp2_block_multiproof_layout": (i32, [sz, sz, sz, vp, sz, vp]),
        "cp2_dataset_block_multiproofs": (i32, [vp, vp, sz, vp, vp, vp, sz, vp]),
        "cp2_blocks_verify_multi": (i32, [vp, sz, sz, sz, vp, sz, vp, sz, vp, vp, vp, sz, vp, vp]),
        "cp2_fill_add_multi": (i32, [vp, vp, sz, vp, vp, vp, sz, vp, ctypes.POINTER(sz)]),
        "cp2_fill_multiproof_want": (i32, [vp, vp, sz, vp, vp, sz, ctypes.POINTER(sz), vp]),
        "cp2_dataset_block_tree_rows": (i32, [vp, vp, sz, vp]),
        "cp2_fill_block_tree_rows": (i32, [vp, vp, sz, vp, vp]),
        "cp2_fill_add_multi_anchored": (i32, [vp, vp, sz, vp, vp, vp, sz, vp, ctypes.POINTER(sz)]),
        "cp2_dataset_repair_blocks_proved": (i32, [vp, vp, vp, vp, sz, i32, cp, vp, ctypes.POINTER(sz)]),
        "cp2_datasets_read_blocks": (i32, [vp, vp, sz, vp, sz, i32, vp, vp, vp, vp, vp, ctypes.POINTER(sz)]),
        "cp2_dataset_read_blocks": (i32, [vp, vp, sz, i32, vp, vp, vp, vp, ctypes.POINTER(sz)]),
        "cp2_fill_begin": (i32, [vp, ctypes.POINTER(Config), u64, u64, vp, pvp]),
        "cp2_fill_add": (i32, [vp, vp, vp, vp, sz, vp, ctypes.POINTER(sz)]),
        "cp2_fill_missing": (i32, [vp, vp, sz, ctypes.POINTER(u64)]),
        "cp2_fill_finish": (i32, [vp, cp, pvp]),
        "cp2_fill_free": (None, [vp]),
        "cp2_fill_save": (i32, [vp, cp]),
        "cp2_fill_resume": (i32, [vp, ctypes.POINTER(Config), u64, u64, vp, cp, i32, pvp, ctypes.POINTER(u64)]),
        "cp2_fill_keep_nodes": (i32, [vp]),
        "cp2_fill_block_proofs": (i32, [vp, vp, sz, vp, vp, vp]),
        "cp2_fill_anchors": (i32, [vp, vp, sz, vp]),
        "cp2_fill_add_anchored": (i32, [vp, vp, vp, vp, vp, sz, vp, ctypes.POINTER(sz)]),
        "cp2_fills_add_many": (i32, [vp, vp, sz, vp, vp, vp, vp, sz, vp, vp]),
        "cp2_fills_finish_many": (i32, [vp, vp, sz, vp, vp]),
        "cp2_fills_resume_many": (i32, [vp, vp, vp, vp, vp, sz, i32, vp, vp]),
        "cp2_datasets_repair_blocks_many": (i32, [vp, vp, sz, vp, vp, vp, vp, sz, i32, vp, vp, ctypes.POINTER(sz)]),
        "cp2_fill_adopt": (i32, [vp, u64, u64, i32, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "cp2_fill_save_nodes": (i32, [vp, cp]),
        "cp2_fill_resume_nodes": (i32, [vp, ctypes.POINTER(Config), u64, u64, vp, cp, i32, pvp, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                        ctypes.POINTER(u64), ctypes.POINTER(u64)]),
    }
    for name, (res, args) in sigs.items():
        if v is None and name == "cp2_abi_version":
            continue           # (an older library named on purpose through CODEX_P2_LIB: A/B tooling)
        f = getattr(L, name)   # AttributeError if the header and the library ever disagree
        f.restype, f.argtypes = res, args
    L._cp2_signatures = sigs
    _lib = L
    return L


def check_environment():
    """cp2_check_environment: None when every CODEX_P2_* variable holds what it takes, else the message naming the first that does not."""
    L = load_library()
    buf = ctypes.create_string_buffer(512)
    return None if L.cp2_check_environment(buf, len(buf)) == CP2_OK else buf.value.decode()


def exported_symbols():
    """Names declared in include/codex_p2.h (parsed from the header text)."""
    import re
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cp2_[a-z0-9_]+)\s*\(", text)))


def _u8(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint8))


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def felt_bytes(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint8).copy()


def felts_to_array(xs):
    out = np.zeros((len(xs), 32), dtype=np.uint8)
    for i, x in enumerate(xs):
        out[i] = felt_bytes(x)
    return out


def array_to_felts(a):
    a = _u8(a).reshape(-1, 32)
    return [int.from_bytes(a[i].tobytes(), "little") for i in range(a.shape[0])]


class Context:
    """One cp2_ctx.  Host-array methods mirror the host-pointer ABI; *_dev methods take raw device pointers."""

    def __init__(self, device=0):
        self.L = load_library()
        h = ctypes.c_void_p()
        st = self.L.cp2_init(device, ctypes.byref(h))
        if st != CP2_OK:
            raise CodexP2Error(st, "cp2_init", self.L.cp2_strerror(st).decode())
        self.h = h
        self._children = weakref.WeakSet()

    def close(self):
        if self.h:
            _free_children(self)
            self.L.cp2_free(self.h)
            self.h = None

    def __del__(self):
        # at interpreter shutdown the HIP runtime (and this module's globals) may already be gone: leak instead
        try:
            if _finalizing():
                return
            self.close()
        except Exception:
            pass

    def _ck(self, st, where):
        if st != CP2_OK:
            raise CodexP2Error(st, where, self.L.cp2_last_error(self.h).decode() or self.L.cp2_strerror(st).decode())

    # -- plumbing
    def set_stream(self, stream_ptr):
        self._ck(self.L.cp2_set_stream(self.h, ctypes.c_void_p(stream_ptr)), "cp2_set_stream")

    def reset_stream(self):
        self._ck(self.L.cp2_reset_stream(self.h), "cp2_reset_stream")

    def sync(self):
        self._ck(self.L.cp2_sync(self.h), "cp2_sync")

    def set_ingest(self, fill_threads=0, ring_depth=0, chunk_bytes=0):
        self._ck(self.L.cp2_set_ingest(self.h, fill_threads, ring_depth, chunk_bytes), "cp2_set_ingest")

    def set_ingest_direct(self, on):
        """O_DIRECT reads of slot files (1 / 0; -1 = environment CP2_INGEST_DIRECT)."""
        self._ck(self.L.cp2_set_ingest_direct(self.h, on), "cp2_set_ingest_direct")

    def set_ingest_mapped(self, on):
        """page-cache-resident chunks of slot files uploaded straight from a mapping, no CPU copy (1 / 0; -1 = environment CP2_INGEST_MAPPED, default off)"""
        self._ck(self.L.cp2_set_ingest_mapped(self.h, on), "cp2_set_ingest_mapped")

    def trim(self):
        """Give the context's cached device / pinned scratch back to the system (cp2_trim)."""
        self._ck(self.L.cp2_trim(self.h), "cp2_trim")

    def set_keep_trees(self, mode=-1):
        """cp2_dataset_build keeps every node of the slot trees resident (1), the block roots and up (2: compact), only the
        roots (0), or the most that fits (-1)"""
        self._ck(self.L.cp2_set_keep_trees(self.h, mode), "cp2_set_keep_trees")

    def set_body_budget(self, max_resident_bytes=0, spill_dir=None):
        self._ck(self.L.cp2_set_body_budget(self.h, max_resident_bytes, spill_dir.encode() if spill_dir else None), "cp2_set_body_budget")

    def blocks_verify(self, cell_size, block_size, n_cells, slot_roots, root_block, data, paths, want_roots=True):
        """cp2_blocks_verify: candidate blocks (n x block_size bytes) with their Merkle paths (uint8[n, depth, 32]) checked against the
        stated slot roots; root_block = (index into slot_roots, block of the slot) pairs.  Returns (status: uint32[n] of BLOCK_*,
        block_roots: uint8[n, 32] or None)."""
        r = _u8(slot_roots).reshape(-1, 32)
        rb = np.ascontiguousarray(np.asarray(root_block, dtype=np.uint64).reshape(-1, 2))
        n = rb.shape[0]
        d, p = _candidates("block verify", data, n, block_size, paths, block_proof_depth(cell_size, block_size, n_cells))
        status = np.empty(n, dtype=np.uint32)
        roots = np.empty((n, 32), dtype=np.uint8) if want_roots else None
        self._ck(self.L.cp2_blocks_verify(self.h, cell_size, block_size, n_cells, _p(r) if r.size else None, r.shape[0], _p(rb) if n else None,
                                          _p(d) if n else None, _p(p) if n else None, n, _p(status) if n else None,
                                          _p(roots) if want_roots and n else None), "cp2_blocks_verify")
        return status, roots

    def blocks_verify_multi(self, cell_size, block_size, n_cells, slot_roots, groups, blocks, data, nodes, want_roots=True):
        """cp2_blocks_verify_multi: candidate blocks (n x block_size bytes) in groups, each group with its multiproof, checked against the
        stated slot roots; groups = (index into slot_roots, count) pairs, blocks = the n block indices group after group, strictly
        ascending inside a group, nodes = the groups' rows packed (uint8[n_rows, 32]).  Returns (status: uint32[n_groups] of BLOCK_*, one
        per GROUP, block_roots: uint8[n, 32] or None)."""
        r = _u8(slot_roots).reshape(-1, 32)
        g, b = _groups(groups, blocks)
        n, ng = b.shape[0], g.shape[0]
        d = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
        if d.nbytes != n * block_size:
            raise ValueError("block verify multi: %d request(s) need %d bytes of candidates, got %d" % (n, n * block_size, d.nbytes))
        rows = _u8(nodes).reshape(-1, 32)
        status = np.empty(ng, dtype=np.uint32)
        roots = np.empty((n, 32), dtype=np.uint8) if want_roots else None
        self._ck(self.L.cp2_blocks_verify_multi(self.h, cell_size, block_size, n_cells, _p(r) if r.size else None, r.shape[0], _p(g) if ng else None, ng,
                                                _p(b) if n else None, _p(d) if n else None, _p(rows) if rows.size else None, rows.shape[0],
                                                _p(status) if ng else None, _p(roots) if want_roots and n else None), "cp2_blocks_verify_multi")
        return status, roots

    # -- a1
    def permute_batch(self, states, out=None):
        s = _u8(states).reshape(-1, 96)
        if out is None:
            out = np.empty_like(s)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size == s.size
        self._ck(self.L.cp2_permute_batch(self.h, _p(s), _p(out), s.shape[0]), "cp2_permute_batch")
        return out

    def permute_batch_dev(self, d_in, d_out, n):
        self._ck(self.L.cp2_permute_batch_dev(self.h, ctypes.c_void_p(d_in), ctypes.c_void_p(d_out), n), "cp2_permute_batch_dev")

    # -- a6
    def compress_batch(self, xy, key):
        a = _u8(xy).reshape(-1, 64)
        out = np.empty((a.shape[0], 32), dtype=np.uint8)
        self._ck(self.L.cp2_compress_batch(self.h, _p(a), key, _p(out), a.shape[0]), "cp2_compress_batch")
        return out

    # -- a3
    def sponge2_felts(self, felts):
        f = _u8(felts).reshape(-1, 32)
        out = np.empty(32, dtype=np.uint8)
        self._ck(self.L.cp2_sponge2_felts(self.h, _p(f) if f.size else None, f.shape[0], _p(out)), "cp2_sponge2_felts")
        return out

    def sponge2_felts_batch(self, felts, nf):
        f = _u8(felts).reshape(-1, 32)
        nitems = f.shape[0] // nf if nf else 0
        out = np.empty((nitems, 32), dtype=np.uint8)
        self._ck(self.L.cp2_sponge2_felts_batch(self.h, _p(f), nf, nitems, _p(out)), "cp2_sponge2_felts_batch")
        return out

    def sponge2_felts_batch_dev(self, d_felts, nf, nitems, d_out):
        self._ck(self.L.cp2_sponge2_felts_batch_dev(self.h, ctypes.c_void_p(d_felts), nf, nitems, ctypes.c_void_p(d_out)), "cp2_sponge2_felts_batch_dev")

    # -- a4
    def bytes_to_felts(self, data):
        d = _u8(np.frombuffer(bytes(data), dtype=np.uint8))
        n = self.L.cp2_felts_per_bytes(d.size)
        out = np.empty((n, 32), dtype=np.uint8)
        self._ck(self.L.cp2_bytes_to_felts(_p(d) if d.size else None, d.size, _p(out)), "cp2_bytes_to_felts")
        return out

    # -- a5
    def hash_cells(self, cells, cell_size):
        c = _u8(cells).reshape(-1)
        n = c.size // cell_size if cell_size else 0
        out = np.empty((n, 32), dtype=np.uint8)
        self._ck(self.L.cp2_hash_cells(self.h, _p(c), cell_size, n, _p(out)), "cp2_hash_cells")
        return out

    def hash_cells_dev(self, d_cells, cell_size, n_cells, d_out):
        self._ck(self.L.cp2_hash_cells_dev(self.h, ctypes.c_void_p(d_cells), cell_size, n_cells, ctypes.c_void_p(d_out)), "cp2_hash_cells_dev")

    def hash_bytes(self, data):
        d = _u8(np.frombuffer(bytes(data), dtype=np.uint8))
        out = np.empty(32, dtype=np.uint8)
        self._ck(self.L.cp2_hash_bytes(self.h, _p(d) if d.size else None, d.size, _p(out)), "cp2_hash_bytes")
        return out

    # -- a7
    def merkle_tree(self, leaves):
        lv = _u8(leaves).reshape(-1, 32)
        n = lv.shape[0]
        total = self.L.cp2_merkle_total(n)
        out = np.empty((total, 32), dtype=np.uint8)
        sizes = (ctypes.c_size_t * 80)()
        nl = ctypes.c_size_t()
        self._ck(self.L.cp2_merkle_tree(self.h, _p(lv) if n else None, n, _p(out), sizes, ctypes.byref(nl)), "cp2_merkle_tree")
        layers, off = [], 0
        for i in range(nl.value):
            layers.append(out[off:off + sizes[i]])
            off += sizes[i]
        return layers

    def merkle_trees_dev(self, d_leaves, n, nseg, d_layers):
        self._ck(self.L.cp2_merkle_trees_dev(self.h, ctypes.c_void_p(d_leaves), n, nseg, ctypes.c_void_p(d_layers)), "cp2_merkle_trees_dev")

    def merkle_root(self, leaves):
        lv = _u8(leaves).reshape(-1, 32)
        out = np.empty(32, dtype=np.uint8)
        self._ck(self.L.cp2_merkle_root(self.h, _p(lv) if lv.size else None, lv.shape[0], _p(out)), "cp2_merkle_root")
        return out

    # -- a10
    def slot_seed(self, seed, slot_idx):
        return self.L.cp2_slot_seed(seed, slot_idx)

    def gen_fake_cells(self, seed, first, n, cell_size):
        out = np.empty((n, cell_size), dtype=np.uint8)
        self._ck(self.L.cp2_gen_fake_cells(self.h, seed, first, n, cell_size, _p(out)), "cp2_gen_fake_cells")
        return out

    def gen_fake_cells_dev(self, seed, first, n, cell_size, d_out):
        self._ck(self.L.cp2_gen_fake_cells_dev(self.h, seed, first, n, cell_size, ctypes.c_void_p(d_out)), "cp2_gen_fake_cells_dev")

    # -- a12
    def cell_indices(self, entropy, slot_root, n_cells, n_samples):
        e, r = _u8(entropy), _u8(slot_root)
        out = np.empty(n_samples, dtype=np.uint64)
        self._ck(self.L.cp2_cell_indices(self.h, _p(e), _p(r), n_cells, n_samples, _p(out)), "cp2_cell_indices")
        return out

    # -- slot trees
    def slot_trees_fake(self, dataset_seed, first_slot, n_slots, cell_size, block_size, n_cells):
        h = ctypes.c_void_p()
        self._ck(self.L.cp2_slot_trees_build_fake(self.h, dataset_seed, first_slot, n_slots, cell_size, block_size, n_cells,
                                                  ctypes.byref(h)), "cp2_slot_trees_build_fake")
        return SlotTrees(self, h)

    def slot_trees_fake_units(self, dataset_seed, units_per_slot, first_unit, n_units, cell_size, block_size, cells_per_unit):
        h = ctypes.c_void_p()
        self._ck(self.L.cp2_slot_trees_build_fake_units(self.h, dataset_seed, units_per_slot, first_unit, n_units, cell_size, block_size,
                                                        cells_per_unit, ctypes.byref(h)), "cp2_slot_trees_build_fake_units")
        return SlotTrees(self, h)

    def slot_trees_file_units(self, file_base, units_per_slot, first_unit, n_units, cell_size, block_size, cells_per_unit):
        h = ctypes.c_void_p()
        self._ck(self.L.cp2_slot_trees_build_file_units(self.h, file_base.encode(), units_per_slot, first_unit, n_units, cell_size, block_size,
                                                        cells_per_unit, ctypes.byref(h)), "cp2_slot_trees_build_file_units")
        return SlotTrees(self, h)

    def slot_trees_dev(self, d_cells, n_slots, cell_size, block_size, n_cells):
        h = ctypes.c_void_p()
        self._ck(self.L.cp2_slot_trees_build_dev(self.h, ctypes.c_void_p(d_cells), n_slots, cell_size, block_size, n_cells,
                                                 ctypes.byref(h)), "cp2_slot_trees_build_dev")
        return SlotTrees(self, h)

    def slot_trees_host(self, cells, n_slots, cell_size, block_size, n_cells):
        c = _u8(cells).reshape(-1)
        h = ctypes.c_void_p()
        self._ck(self.L.cp2_slot_trees_build_host(self.h, _p(c), n_slots, cell_size, block_size, n_cells, ctypes.byref(h)),
                 "cp2_slot_trees_build_host")
        t = SlotTrees(self, h)
        t._keep = c   # the library keeps the host pointer for sampled-cell retrieval
        return t

    def slot_trees_load(self, path):
        h = ctypes.c_void_p()
        self._ck(self.L.cp2_slot_trees_load(self.h, path.encode(), ctypes.byref(h)), "cp2_slot_trees_load")
        return SlotTrees(self, h)

    # -- dataset / proof input
    def fill(self, cfg, slot_roots, first_slot=0, n_local=None):
        """cp2_fill_begin: a session that fills local slots [first_slot, + n_local) from proved network blocks (FillSession)"""
        return FillSession(self, cfg, slot_roots, first_slot, cfg.n_slots - first_slot if n_local is None else n_local)

    def fill_resume(self, cfg, slot_roots, path, first_slot=0, n_local=None, trust_files=False):
        """cp2_fill_resume: the session saved at `path` (FillSession.save), every block it calls present re-checked on the device against what
        the source holds now unless trust_files; the session's `n_dropped` says how many blocks the disk no longer backs"""
        return FillSession.resume(self, cfg, slot_roots, path, first_slot, cfg.n_slots - first_slot if n_local is None else n_local, trust_files)

    def fill_resume_nodes(self, cfg, slot_roots, path, first_slot=0, n_local=None, trust_files=False):
        """cp2_fill_resume_nodes: the keeping session saved at `path` (FillSession.save_nodes, or FillSession.save), resumed as fill_resume
        resumes it, keeping nodes, with every saved node restored that the device re-derives from the stated roots; the session's
        `n_dropped`, `n_restored`, `n_unproved` and `n_rejected` say what became of the blocks and the saved rows"""
        return FillSession.resume_nodes(self, cfg, slot_roots, path, first_slot, cfg.n_slots - first_slot if n_local is None else n_local, trust_files)

    def dataset(self, cfg, first_slot=0, n_local=None, cache=None):
        return Dataset(self, cfg, first_slot, cfg.n_slots if n_local is None else n_local, cache)

    def verify_proof_inputs(self, proof_inputs):
        """cp2_proof_inputs_verify: what SampleAndProve accepts.  Returns (status uint32[n]: 0 or CP2_VERIFY_* bits,
        sample_ok uint8[n, nSamples]: 1 where that sample's cell and path give slotRoot)."""
        n = len(proof_inputs)
        ns = int(self.L.cp2_proof_input_nsamples(proof_inputs[0].h)) if n else 0
        hs = (ctypes.c_void_p * max(n, 1))(*[p.h for p in proof_inputs])
        status = np.zeros(n, dtype=np.uint32)
        ok = np.zeros((n, ns), dtype=np.uint8)
        self._ck(self.L.cp2_proof_inputs_verify(self.h, hs, n, _p(status), _p(ok)), "cp2_proof_inputs_verify")
        return status, ok

    @staticmethod
    def _many_arrays(requests):
        """(dataset handles, slot indices, entropies n x 32) of a sequence of (Dataset, slot, entropy) requests"""
        n = len(requests)
        hs = (ctypes.c_void_p * max(n, 1))(*[r[0].h for r in requests])
        slots = np.ascontiguousarray(np.asarray([r[1] for r in requests], dtype=np.uint64).reshape(n))
        ent = np.zeros((max(n, 1), 32), dtype=np.uint8)
        for i, r in enumerate(requests):
            e = r[2]
            ent[i] = felt_bytes(e) if isinstance(e, int) else np.frombuffer(bytes(e), dtype=np.uint8) if isinstance(e, (bytes, bytearray)) else _u8(e)
        return hs, slots, ent

    def proof_inputs_many(self, requests):
        """cp2_proof_inputs_generate_many: one proof input per (Dataset, slot, entropy) request, across datasets of one circuit
        (entropy: an int or 32 bytes)."""
        hs, slots, ent = self._many_arrays(requests)
        n = len(requests)
        out = (ctypes.c_void_p * max(n, 1))()
        self._ck(self.L.cp2_proof_inputs_generate_many(self.h, hs, _p(slots), _p(ent), n, out), "cp2_proof_inputs_generate_many")
        pis = []
        for i, r in enumerate(requests):
            pi = ProofInput(self, ctypes.c_void_p(out[i]), r[0].cfg)
            pi.slot_idx = int(r[1])
            pis.append(pi)
        return pis

    def scrub_many(self, datasets, cap=1 << 20):
        """cp2_datasets_scrub_many: every local slot of each Dataset of this context in one pass.  Returns (granularity: int32[n] of
        SCRUB_*, bad: uint64[k, 3] of (request, slot, index), the lowest k = min(cap, n_bad), counts: uint64[n] mismatches per request,
        complete whatever cap is, n_bad)."""
        n, cap = len(datasets), int(cap)
        hs = (ctypes.c_void_p * max(n, 1))(*[d.h for d in datasets])
        bad = np.empty((cap, 3), dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.uint64)
        gran = np.zeros(max(n, 1), dtype=np.int32)
        nb = ctypes.c_size_t()
        self._ck(self.L.cp2_datasets_scrub_many(self.h, hs, n, _p(bad) if cap else None, cap, ctypes.byref(nb), _p(counts), _p(gran)),
                 "cp2_datasets_scrub_many")
        return gran[:n].copy(), bad[:min(cap, nb.value)].copy(), counts[:n].copy(), nb.value

    def build_many(self, requests):
        """cp2_datasets_build_many: one Dataset per (cfg, first_slot, n_local) request, all built in one pass; each is what
        Context.dataset(cfg, first_slot, n_local) returns under the same kept mode.  All of them, or an error and none."""
        requests = list(requests)
        n = len(requests)
        cfgs = (Config * max(n, 1))()
        ranges = np.zeros((max(n, 1), 2), dtype=np.uint64)
        for i, (cfg, first_slot, n_local) in enumerate(requests):
            cfgs[i] = cfg                          # (a copy of the struct; the request keeps the base name it points to alive)
            ranges[i] = (first_slot, n_local)
        out = (ctypes.c_void_p * max(n, 1))()
        self._ck(self.L.cp2_datasets_build_many(self.h, cfgs, _p(ranges), n, out), "cp2_datasets_build_many")
        return [Dataset.adopt(self, r[0], ctypes.c_void_p(out[i]), int(r[1]), int(r[2])) for i, r in enumerate(requests)]

    def set_roots_many(self, datasets, roots=None):
        """cp2_datasets_set_roots_many: the dataset tree of every Dataset of this context in one pass; each is left as
        Dataset.set_roots(roots[i]) leaves it.  roots: None, or one entry per dataset (None, or n_slots x 32 bytes).  Returns own:
        uint8[n], 1 where the dataset's own rows of its roots equal the roots it built.  All of them, or an error and none."""
        datasets = list(datasets)
        n = len(datasets)
        hs = (ctypes.c_void_p * max(n, 1))(*[d.h for d in datasets])
        ptrs, keep = None, []
        if roots is not None:
            roots = list(roots)
            assert len(roots) == n
            ptrs = (ctypes.c_void_p * max(n, 1))()
            for i, r in enumerate(roots):
                if r is not None:
                    a = np.ascontiguousarray(_u8(r).reshape(-1, 32))
                    assert a.shape[0] == datasets[i].cfg.n_slots
                    keep.append(a)
                    ptrs[i] = a.ctypes.data
        own = np.zeros(max(n, 1), dtype=np.uint8)
        self._ck(self.L.cp2_datasets_set_roots_many(self.h, hs, ptrs, n, _p(own)), "cp2_datasets_set_roots_many")
        return own[:n].copy()

    def read_blocks(self, datasets, requests, check_only=False, want_data=True, want_paths=True, data=None):
        """cp2_datasets_read_blocks: the blocks named by requests (uint64[n, 3]: index into datasets, slot, block) read from the slot files,
        checked on the device against the block roots the datasets keep and returned with their proofs.  data: an array of n x blockSize
        bytes to read into (caller-pinned memory is read in place), else one is made unless want_data is False (which needs check_only).
        Returns (data: uint8[n, blockSize] or None, block_roots: uint8[n, 32], paths: uint8[sum of depths, 32] or None, path_off:
        uint64[n + 1] or None, status: uint32[n] of READ_*, n_ok); DAMAGED rows of data are zeros."""
        rq = np.ascontiguousarray(np.asarray(requests, dtype=np.uint64).reshape(-1, 3))
        n, nd = rq.shape[0], len(datasets)
        hs = (ctypes.c_void_p * max(nd, 1))(*[d.h for d in datasets])
        bs = int(datasets[0].cfg.block_size) if nd else 0
        if data is None and want_data:
            data = np.empty((n, bs), dtype=np.uint8)
        roots = np.empty((n, 32), dtype=np.uint8)
        paths = off = None
        if want_paths:
            depth = [d.block_proof_depth for d in datasets]
            total = sum(depth[int(k)] for k in rq[:, 0] if int(k) < nd)
            paths = np.empty((total, 32), dtype=np.uint8)
            off = np.zeros(n + 1, dtype=np.uint64)
        status = np.empty(n, dtype=np.uint32)
        ok = ctypes.c_size_t()
        dp = None if data is None else ctypes.c_void_p(data.ctypes.data if isinstance(data, np.ndarray) else int(data))
        self._ck(self.L.cp2_datasets_read_blocks(self.h, hs, nd, _p(rq), n, READ_CHECK_ONLY if check_only else 0, dp, _p(roots),
                                                 _p(paths) if want_paths else None, _p(off) if want_paths else None, _p(status), ctypes.byref(ok)),
                 "cp2_datasets_read_blocks")
        return data, roots, paths, off, status, ok.value

    def repair_blocks_many(self, datasets, requests, data, paths=None, path_off=None, check_only=False, cache_paths=None):
        """cp2_datasets_repair_blocks_many: candidate blocks (n x blockSize bytes) for requests (uint64[n, 3]: index into datasets, slot,
        block) judged on the device in one pass and the matching ones written back, the slot files spread over the ingestion threads.
        paths (uint8[rows, 32]) and path_off (uint64[n + 1]) are what read_blocks returns: request i's path is rows path_off[i] to
        path_off[i + 1]; an empty one judges against the kept block root, a whole one walks to the dataset's own slot root (the only form a
        roots-only dataset takes); both None: every path is empty.  cache_paths: None, or one entry (None or a path) per dataset.  `data`
        as for Dataset.repair_blocks.  Returns (status: uint32[n] of REPAIR_*, n_written)."""
        rq = np.ascontiguousarray(np.asarray(requests, dtype=np.uint64).reshape(-1, 3))
        n, nd = rq.shape[0], len(datasets)
        hs = (ctypes.c_void_p * max(nd, 1))(*[d.h for d in datasets])
        bs = int(datasets[0].cfg.block_size) if nd else 0
        d = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)   # (no copy of a contiguous array)
        if d.nbytes != n * bs:
            raise ValueError("repair many: %d request(s) need %d bytes of candidates, got %d" % (n, n * bs, d.nbytes))
        if (paths is None) != (path_off is None):
            raise ValueError("repair many: paths and path_off go together")
        pp = po = None
        if paths is not None:
            po = np.ascontiguousarray(np.asarray(path_off, dtype=np.uint64).reshape(-1))
            pp = np.ascontiguousarray(_u8(paths).reshape(-1, 32))
            if po.shape[0] != n + 1 or (n and int(po.max()) > pp.shape[0]):
                raise ValueError("repair many: path_off needs n + 1 = %d entries inside the %d row(s) of paths" % (n + 1, pp.shape[0]))
            if pp.shape[0] == 0:
                pp = np.zeros((1, 32), dtype=np.uint8)   # (an address to hand over: no row of it is read)
        cps = None
        if cache_paths is not None:
            cache_paths = list(cache_paths)
            assert len(cache_paths) == nd
            cps = (ctypes.c_char_p * max(nd, 1))(*[c.encode() if c else None for c in cache_paths])
        status = np.empty(n, dtype=np.uint32)
        written = ctypes.c_size_t()
        self._ck(self.L.cp2_datasets_repair_blocks_many(self.h, hs, nd, _p(rq) if n else None, _p(d) if n else None, _p(pp) if pp is not None else None,
                                                        _p(po) if po is not None else None, n, REPAIR_CHECK_ONLY if check_only else 0, cps,
                                                        _p(status) if n else None, ctypes.byref(written)), "cp2_datasets_repair_blocks_many")
        return status, written.value

    def export_proof_inputs_many(self, requests, paths=None, threads=1, batch=0):
        """cp2_proof_inputs_export_many: generate + serialise (+ write paths[i] where it is not None) as a pipeline; returns the
        total text bytes."""
        hs, slots, ent = self._many_arrays(requests)
        n = len(requests)
        cpaths = None
        if paths is not None:
            cpaths = (ctypes.c_char_p * max(n, 1))(*[p.encode() if p else None for p in paths])
        total = ctypes.c_uint64()
        self._ck(self.L.cp2_proof_inputs_export_many(self.h, hs, _p(slots), _p(ent), n, cpaths, threads, batch, ctypes.byref(total)),
                 "cp2_proof_inputs_export_many")
        return total.value

    def dataset_streamed(self, cfg, entropy, first_slot=0, n_local=None, threads=1, group_slots=0):
        """cp2_dataset_build_streamed: trees + (overlapped) the proof-input bodies of every local slot for `entropy`."""
        return Dataset(self, cfg, first_slot, cfg.n_slots if n_local is None else n_local, None,
                       streamed=(entropy, threads, group_slots))


def make_config(maxDepth=32, maxLog2NSlots=8, cellSize=2048, blockSize=65536, nSlots=11, nCells=256, nSamples=5,
                seed=12345, file=None):
    """Defaults are the reference CLI's (reference/nim/proof_input/src/cli.nim:47-76)."""
    c = Config()
    c.max_depth, c.max_log2_nslots = maxDepth, maxLog2NSlots
    c.cell_size, c.block_size = cellSize, blockSize
    c.n_slots, c.n_cells, c.n_samples, c.seed = nSlots, nCells, nSamples, seed
    c.file_base = file.encode() if file else None
    return c


class SlotTrees:
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h
        ctx._children.add(self)

    def free(self):
        if self.h:
            self.ctx.L.cp2_slot_trees_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if _finalizing():
                return
            self.free()
        except Exception:
            pass

    @property
    def count(self):
        return self.ctx.L.cp2_slot_trees_count(self.h)

    @property
    def depth(self):
        return self.ctx.L.cp2_slot_trees_depth(self.h)

    def save(self, path):
        self.ctx._ck(self.ctx.L.cp2_slot_trees_save(self.h, path.encode()), "cp2_slot_trees_save")

    def roots(self):
        out = np.empty((self.count, 32), dtype=np.uint8)
        self.ctx._ck(self.ctx.L.cp2_slot_trees_roots(self.h, _p(out)), "cp2_slot_trees_roots")
        return out

    def roots_dev(self):
        return self.ctx.L.cp2_slot_trees_roots_dev(self.h)

    def paths(self, slot, cell_idx, max_depth):
        idx = np.ascontiguousarray(np.asarray(cell_idx, dtype=np.uint64))
        out = np.empty((idx.size, max_depth, 32), dtype=np.uint8)
        leaves = np.empty((idx.size, 32), dtype=np.uint8)
        self.ctx._ck(self.ctx.L.cp2_slot_trees_paths(self.h, slot, _p(idx), idx.size, max_depth, _p(out), _p(leaves)),
                     "cp2_slot_trees_paths")
        return out, leaves


SCRUB_SLOT, SCRUB_BLOCK, SCRUB_CELL = 0, 1, 2     # CP2_SCRUB_* (include/codex_p2.h): what a scrub's indices count


def _scrub(fn, h, first_slot, n_slots, cap, ck, where):
    """(granularity, bad: uint64[k, 2] of (slot, index), n_bad) of cp2_dataset_scrub / cp2_multi_dataset_scrub"""
    cap = int(cap)
    bad = np.empty((cap, 2), dtype=np.uint64)
    n, g = ctypes.c_size_t(), ctypes.c_int()
    ck(fn(h, first_slot, n_slots, _p(bad) if cap else None, cap, ctypes.byref(n), ctypes.byref(g)), where)
    return g.value, bad[:min(cap, n.value)].copy(), n.value


# CP2_REPAIR_* (include/codex_p2.h): the flag that makes a repair check only, and the per-request verdicts
REPAIR_CHECK_ONLY = 1
REPAIR_MATCH, REPAIR_MISMATCH, REPAIR_UNWRITTEN = 0, 1, 2


def _repair(fn, h, block_size, slot_block, data, check_only, cache_path, ck, where):
    """(status: uint32[n], n_written) of cp2_dataset_repair_blocks / cp2_multi_dataset_repair_blocks.  `data` may be any buffer of
    n x block_size bytes that numpy can view without a copy (bytes, a numpy array, a pinned torch tensor's .numpy())."""
    sb = np.ascontiguousarray(np.asarray(slot_block, dtype=np.uint64).reshape(-1, 2))
    n = sb.shape[0]
    d = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)   # (no copy of a contiguous array)
    if d.nbytes != n * block_size:
        raise ValueError("repair: %d request(s) need %d bytes of candidates, got %d" % (n, n * block_size, d.nbytes))
    status = np.empty(n, dtype=np.uint32)
    written = ctypes.c_size_t()
    ck(fn(h, _p(sb) if n else None, _p(d) if n else None, n, REPAIR_CHECK_ONLY if check_only else 0,
          cache_path.encode() if cache_path else None, _p(status) if n else None, ctypes.byref(written)), where)
    return status, written.value


READ_CHECK_ONLY = 1                               # CP2_READ_* (include/codex_p2.h): the flag and the verdicts of the verified read-back
READ_OK, READ_DAMAGED = 0, 1
BLOCK_MATCH, BLOCK_MISMATCH = 0, 1                # CP2_BLOCK_* (include/codex_p2.h): the verdicts of cp2_blocks_verify


def block_proof_depth(cell_size, block_size, n_cells):
    """cp2_block_proof_depth: siblings in the proof of one network block (0: a geometry the tree builders refuse); host only"""
    return load_library().cp2_block_proof_depth(cell_size, block_size, n_cells)


def _groups(groups, blocks):
    """the (slot or root index, count) pairs and the block list of a multiproof call as contiguous uint64 arrays"""
    g = np.ascontiguousarray(np.asarray(groups, dtype=np.uint64).reshape(-1, 2))
    b = np.ascontiguousarray(np.asarray(blocks, dtype=np.uint64).reshape(-1))
    if int(g[:, 1].sum()) != b.shape[0]:
        raise ValueError("multiproof: the groups count %d block(s), blocks holds %d" % (int(g[:, 1].sum()), b.shape[0]))
    return g, b


def block_multiproof_rows(cell_size, block_size, n_cells, blocks):
    """cp2_block_multiproof_rows: rows in the multiproof of `blocks` (strictly ascending) of one slot; host only.  ValueError for a refused
    geometry or list."""
    b = np.ascontiguousarray(np.asarray(blocks, dtype=np.uint64).reshape(-1))
    rows = load_library().cp2_block_multiproof_rows(cell_size, block_size, n_cells, _p(b) if b.size else None, b.shape[0])
    if rows == ctypes.c_size_t(-1).value:
        raise ValueError("block multiproof: a geometry the tree builders refuse, or blocks that are not strictly ascending below nBlocks")
    return rows


def block_multiproof_layout(cell_size, block_size, n_cells, blocks):
    """cp2_block_multiproof_layout: the (level, index) of every row of that multiproof, in order, as a list of pairs; host only"""
    b = np.ascontiguousarray(np.asarray(blocks, dtype=np.uint64).reshape(-1))
    li = np.zeros((block_multiproof_rows(cell_size, block_size, n_cells, b), 2), dtype=np.uint64)
    if load_library().cp2_block_multiproof_layout(cell_size, block_size, n_cells, _p(b), b.shape[0], _p(li) if li.size else None) != 0:
        raise ValueError("block multiproof: refused")
    return [(int(l), int(i)) for l, i in li]


def _candidates(what, data, n, block_size, paths, depth):
    """the candidate bytes without a copy (see _repair) and the paths as uint8[n, depth, 32]"""
    d = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
    if d.nbytes != n * block_size:
        raise ValueError("%s: %d request(s) need %d bytes of candidates, got %d" % (what, n, n * block_size, d.nbytes))
    p = _u8(paths)
    if p.size != n * depth * 32:
        raise ValueError("%s: %d request(s) need %d bytes of paths (depth %d), got %d" % (what, n, n * depth * 32, depth, p.size))
    return d, p


class Dataset:
    def __init__(self, ctx, cfg, first_slot, n_local, cache=None, streamed=None):
        self.ctx, self.cfg = ctx, cfg
        h = ctypes.c_void_p()
        if streamed is not None:
            entropy, threads, group = streamed
            e = _u8(entropy if not isinstance(entropy, int) else felt_bytes(entropy))
            ctx._ck(ctx.L.cp2_dataset_build_streamed(ctx.h, ctypes.byref(cfg), first_slot, n_local, _p(e), threads, group,
                                                     ctypes.byref(h)), "cp2_dataset_build_streamed")
        elif cache:
            ctx._ck(ctx.L.cp2_dataset_build_cached(ctx.h, ctypes.byref(cfg), first_slot, n_local, cache.encode(), ctypes.byref(h)),
                    "cp2_dataset_build_cached")
        else:
            ctx._ck(ctx.L.cp2_dataset_build(ctx.h, ctypes.byref(cfg), first_slot, n_local, ctypes.byref(h)), "cp2_dataset_build")
        self._own(h, first_slot, n_local)

    def _own(self, h, first_slot, n_local):
        self.h, self.first_slot, self.n_local = h, first_slot, n_local
        self.ctx._children.add(self)

    @classmethod
    def adopt(cls, ctx, cfg, h, first_slot, n_local):
        """a Dataset around a cp2_dataset handle made elsewhere (cp2_fill_finish); it owns the handle like a built one"""
        ds = cls.__new__(cls)
        ds.ctx, ds.cfg = ctx, cfg
        ds._own(h, first_slot, n_local)
        return ds

    def free(self):
        if self.h:
            self.ctx.L.cp2_dataset_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if _finalizing():
                return
            self.free()
        except Exception:
            pass

    def local_roots(self):
        out = np.empty((self.n_local, 32), dtype=np.uint8)
        self.ctx._ck(self.ctx.L.cp2_dataset_local_roots(self.h, _p(out)), "cp2_dataset_local_roots")
        return out

    def set_roots(self, all_roots=None):
        if all_roots is None:
            self.ctx._ck(self.ctx.L.cp2_dataset_set_roots(self.h, None), "cp2_dataset_set_roots")
        else:
            r = _u8(all_roots).reshape(-1, 32)
            assert r.shape[0] == self.cfg.n_slots
            self.ctx._ck(self.ctx.L.cp2_dataset_set_roots(self.h, _p(r)), "cp2_dataset_set_roots")

    @property
    def tree_mode(self):
        """1 every node resident, 2 compact (block roots and up), 0 roots only"""
        return self.ctx.L.cp2_dataset_keeps_trees(self.h)

    @property
    def keeps_trees(self):
        return self.tree_mode == 1

    def local_roots_dev(self):
        """device pointer to the n_local x 32 bytes of local slot roots"""
        return self.ctx.L.cp2_dataset_local_roots_dev(self.h)

    def copy_local_roots_dev(self, d_out):
        """enqueue a device-to-device copy of the local roots into the caller's buffer (context's stream; ctx.sync() after)"""
        self.ctx._ck(self.ctx.L.cp2_dataset_copy_local_roots_dev(self.h, ctypes.c_void_p(d_out)), "cp2_dataset_copy_local_roots_dev")

    def set_roots_dev(self, d_all_roots):
        """all n_slots roots from device memory (the gathered buffer): no host copy on the way in"""
        self.ctx._ck(self.ctx.L.cp2_dataset_set_roots_dev(self.h, ctypes.c_void_p(d_all_roots)), "cp2_dataset_set_roots_dev")

    def root(self):
        out = np.empty(32, dtype=np.uint8)
        self.ctx._ck(self.ctx.L.cp2_dataset_root(self.h, _p(out)), "cp2_dataset_root")
        return out

    def proof_input(self, slot_idx, entropy):
        e = _u8(entropy if not isinstance(entropy, int) else felt_bytes(entropy))
        h = ctypes.c_void_p()
        self.ctx._ck(self.ctx.L.cp2_proof_input_generate(self.h, slot_idx, _p(e), ctypes.byref(h)), "cp2_proof_input_generate")
        pi = ProofInput(self.ctx, h, self.cfg)
        pi.slot_idx = slot_idx
        return pi


    def export_proof_inputs(self, slot_indices, entropy, directory=None, threads=1, batch=0):
        """Pipelined generate + serialise (+ write "<directory>/input_<slot>.json"); returns the total text bytes."""
        e = _u8(entropy if not isinstance(entropy, int) else felt_bytes(entropy))
        idx = np.ascontiguousarray(np.asarray(slot_indices, dtype=np.uint64))
        total = ctypes.c_uint64()
        self.ctx._ck(self.ctx.L.cp2_dataset_export_proof_inputs(self.h, _p(idx), idx.size, _p(e), directory.encode() if directory else None,
                                                                threads, batch, ctypes.byref(total)), "cp2_dataset_export_proof_inputs")
        return total.value

    def export_streamed(self, directory=None, threads=1):
        """Finish the proof inputs prepared by Context.dataset_streamed; returns the total text bytes."""
        total = ctypes.c_uint64()
        self.ctx._ck(self.ctx.L.cp2_dataset_export_streamed(self.h, directory.encode() if directory else None, threads,
                                                            ctypes.byref(total)), "cp2_dataset_export_streamed")
        return total.value

    def streamed_json(self, slot_idx):
        text, ln = ctypes.c_void_p(), ctypes.c_size_t()
        self.ctx._ck(self.ctx.L.cp2_dataset_streamed_json(self.h, slot_idx, ctypes.byref(text), ctypes.byref(ln)), "cp2_dataset_streamed_json")
        s = ctypes.string_at(text, ln.value).decode()
        self.ctx.L.cp2_free_buffer(text)
        return s

    def scrub(self, first_slot=None, n_slots=0, cap=1 << 20):
        """cp2_dataset_scrub: re-read slots first_slot .. + n_slots (0: every local slot) from the source and compare them with what the
        dataset keeps.  Returns (granularity SCRUB_*, bad: uint64[k, 2] of (slot, index), the lowest k = min(cap, n_bad), n_bad)."""
        first = self.first_slot if first_slot is None else first_slot
        return _scrub(self.ctx.L.cp2_dataset_scrub, self.h, first, n_slots, cap, self.ctx._ck, "cp2_dataset_scrub")

    def repair_blocks(self, slot_block, data, check_only=False, cache_path=None):
        """cp2_dataset_repair_blocks: candidate blocks (n x blockSize bytes) for (slot, block) pairs checked on the device against the
        kept block roots; the matching ones written back into the slot files (unless check_only) and, with cache_path, the cache's
        stamps of those files kept valid.  Returns (status: uint32[n] of REPAIR_*, n_written)."""
        return _repair(self.ctx.L.cp2_dataset_repair_blocks, self.h, self.cfg.block_size, slot_block, data, check_only, cache_path, self.ctx._ck,
                       "cp2_dataset_repair_blocks")

    @property
    def block_proof_depth(self):
        return block_proof_depth(self.cfg.cell_size, self.cfg.block_size, self.cfg.n_cells)

    def block_proofs(self, slot_block):
        """cp2_dataset_block_proofs: (block_roots: uint8[n, 32], paths: uint8[n, depth, 32]) of (slot, block) pairs, from what the dataset
        keeps (every node or the compact layers; a roots-only dataset refuses)."""
        sb = np.ascontiguousarray(np.asarray(slot_block, dtype=np.uint64).reshape(-1, 2))
        n, depth = sb.shape[0], self.block_proof_depth
        roots = np.empty((n, 32), dtype=np.uint8)
        paths = np.empty((n, depth, 32), dtype=np.uint8)
        self.ctx._ck(self.ctx.L.cp2_dataset_block_proofs(self.h, _p(sb) if n else None, n, _p(roots) if n else None, _p(paths) if n else None),
                     "cp2_dataset_block_proofs")
        return roots, paths

    def block_multiproofs(self, groups, blocks, want_roots=True):
        """cp2_dataset_block_multiproofs: (block_roots: uint8[n, 32] or None, nodes: uint8[n_rows, 32]) of groups of blocks -- groups =
        (dataset slot, count) pairs, blocks strictly ascending inside a group -- from what the dataset keeps; the rows of the groups are
        packed in group order (block_multiproof_layout names them)."""
        g, b = _groups(groups, blocks)
        n, ng = b.shape[0], g.shape[0]
        roots = np.empty((n, 32), dtype=np.uint8) if want_roots else None
        nodes, n_rows = np.empty((0, 32), dtype=np.uint8), ctypes.c_size_t(0)

        def call():
            return self.ctx.L.cp2_dataset_block_multiproofs(self.h, _p(g) if ng else None, ng, _p(b) if n else None, _p(roots) if want_roots and n else None,
                                                            _p(nodes) if nodes.size else None, nodes.shape[0], ctypes.byref(n_rows))
        st = call()                                    # without room: the call states the rows it needs and writes nothing
        if st != 0 and n_rows.value:
            nodes = np.empty((n_rows.value, 32), dtype=np.uint8)
            st = call()
        self.ctx._ck(st, "cp2_dataset_block_multiproofs")
        return roots, nodes

    def block_tree_rows(self, places):
        """cp2_dataset_block_tree_rows: uint8[n, 32], the tree rows at (dataset slot, level, index) places -- level depth is the slot root --
        from what the dataset keeps: the rows a fill session's multiproof_want names."""
        pl = np.ascontiguousarray(np.asarray(places, dtype=np.uint64).reshape(-1, 3))
        n = pl.shape[0]
        rows = np.empty((n, 32), dtype=np.uint8)
        self.ctx._ck(self.ctx.L.cp2_dataset_block_tree_rows(self.h, _p(pl) if n else None, n, _p(rows) if n else None), "cp2_dataset_block_tree_rows")
        return rows

    def read_blocks(self, slot_block, check_only=False, want_data=True, want_paths=True, data=None):
        """cp2_dataset_read_blocks: Context.read_blocks over this dataset alone, (slot, block) pairs.  Returns (data: uint8[n, blockSize] or
        None, block_roots: uint8[n, 32], paths: uint8[n, depth, 32] or None, status: uint32[n] of READ_*, n_ok)."""
        sb = np.ascontiguousarray(np.asarray(slot_block, dtype=np.uint64).reshape(-1, 2))
        n, depth = sb.shape[0], self.block_proof_depth
        if data is None and want_data:
            data = np.empty((n, int(self.cfg.block_size)), dtype=np.uint8)
        roots = np.empty((n, 32), dtype=np.uint8)
        paths = np.empty((n, depth, 32), dtype=np.uint8) if want_paths else None
        status = np.empty(n, dtype=np.uint32)
        ok = ctypes.c_size_t()
        dp = None if data is None else ctypes.c_void_p(data.ctypes.data if isinstance(data, np.ndarray) else int(data))
        self.ctx._ck(self.ctx.L.cp2_dataset_read_blocks(self.h, _p(sb), n, READ_CHECK_ONLY if check_only else 0, dp, _p(roots),
                                                        _p(paths) if want_paths else None, _p(status), ctypes.byref(ok)),
                     "cp2_dataset_read_blocks")
        return data, roots, paths, status, ok.value

    def repair_blocks_proved(self, slot_block, data, paths, check_only=False, cache_path=None):
        """cp2_dataset_repair_blocks_proved: repair_blocks with the Merkle path (uint8[n, depth, 32]) of every candidate, checked against the
        dataset's slot roots: works in every residency mode.  Returns (status: uint32[n] of REPAIR_*, n_written)."""
        sb = np.ascontiguousarray(np.asarray(slot_block, dtype=np.uint64).reshape(-1, 2))
        n = sb.shape[0]
        d, p = _candidates("repair", data, n, self.cfg.block_size, paths, self.block_proof_depth)
        status = np.empty(n, dtype=np.uint32)
        written = ctypes.c_size_t()
        self.ctx._ck(self.ctx.L.cp2_dataset_repair_blocks_proved(self.h, _p(sb) if n else None, _p(d) if n else None, _p(p) if n else None, n,
                                                                 REPAIR_CHECK_ONLY if check_only else 0, cache_path.encode() if cache_path else None,
                                                                 _p(status) if n else None, ctypes.byref(written)),
                     "cp2_dataset_repair_blocks_proved")
        return status, written.value

    def proof_inputs(self, slot_indices, entropy):
        """Batched generateProofInput for many slots of this dataset (one sampling / gather / fetch)."""
        e = _u8(entropy if not isinstance(entropy, int) else felt_bytes(entropy))
        idx = np.ascontiguousarray(np.asarray(slot_indices, dtype=np.uint64))
        hs = (ctypes.c_void_p * idx.size)()
        self.ctx._ck(self.ctx.L.cp2_proof_inputs_generate_batch(self.h, _p(idx), idx.size, _p(e), hs), "cp2_proof_inputs_generate_batch")
        return [ProofInput(self.ctx, ctypes.c_void_p(h), self.cfg) for h in hs]


FILL_NEW, FILL_MISMATCH, FILL_DUPLICATE, FILL_UNWRITTEN = 0, 1, 2, 3   # CP2_FILL_* (include/codex_p2.h): the per-request results of cp2_fill_add
RESUME_TRUST_FILES = 1                                                 # CP2_RESUME_TRUST_FILES: cp2_fill_resume reads no slot byte
FILL_PROOF_OK, FILL_PROOF_ABSENT, FILL_PROOF_PARTIAL = 0, 1, 2         # CP2_FILL_PROOF_*: the per-request results of cp2_fill_block_proofs
FILL_ROW_KNOWN, FILL_ROW_UNKNOWN = 0, 1                                # CP2_FILL_ROW_*: the per-place results of cp2_fill_block_tree_rows
ADOPT_NO_READ = 1                                                      # CP2_ADOPT_NO_READ: cp2_fill_adopt judges what earlier calls read


class FillSession:
    """One cp2_fill: slots filled from proved network blocks in any order, then handed over as a compact Dataset.  Owns the handle; a
    failing add (CP2_ERR_IO: a slot file could not be written) raises with the statuses in the error's `fill_status`."""

    def __init__(self, ctx, cfg, slot_roots, first_slot, n_local):
        self.ctx, self.cfg, self.first_slot, self.n_local = ctx, cfg, first_slot, n_local
        r = _u8(slot_roots).reshape(-1, 32)
        if r.shape[0] != n_local:
            raise ValueError("fill: %d local slot(s) need %d roots, got %d" % (n_local, n_local, r.shape[0]))
        h = ctypes.c_void_p()
        ctx._ck(ctx.L.cp2_fill_begin(ctx.h, ctypes.byref(cfg), first_slot, n_local, _p(r) if r.size else None, ctypes.byref(h)), "cp2_fill_begin")
        self.h = h
        self.n_dropped = 0
        ctx._children.add(self)

    @classmethod
    def resume(cls, ctx, cfg, slot_roots, path, first_slot, n_local, trust_files=False):
        """cp2_fill_resume: a session around the checkpoint at `path`; n_dropped = the blocks the re-check took back"""
        r = _u8(slot_roots).reshape(-1, 32)
        if r.shape[0] != n_local:
            raise ValueError("fill: %d local slot(s) need %d roots, got %d" % (n_local, n_local, r.shape[0]))
        f = cls.__new__(cls)
        f.ctx, f.cfg, f.first_slot, f.n_local, f.h = ctx, cfg, first_slot, n_local, None
        h, dropped = ctypes.c_void_p(), ctypes.c_uint64()
        ctx._ck(ctx.L.cp2_fill_resume(ctx.h, ctypes.byref(cfg), first_slot, n_local, _p(r) if r.size else None, os.fsencode(path),
                                      RESUME_TRUST_FILES if trust_files else 0, ctypes.byref(h), ctypes.byref(dropped)), "cp2_fill_resume")
        f.h, f.n_dropped = h, dropped.value
        ctx._children.add(f)
        return f

    @classmethod
    def resume_nodes(cls, ctx, cfg, slot_roots, path, first_slot, n_local, trust_files=False):
        """cp2_fill_resume_nodes: a keeping session around the checkpoint at `path` (CP2FILL2 or CP2FILL1); n_dropped = the blocks the
        re-check took back, n_restored / n_unproved / n_rejected = what became of the saved rows presence does not give"""
        r = _u8(slot_roots).reshape(-1, 32)
        if r.shape[0] != n_local:
            raise ValueError("fill: %d local slot(s) need %d roots, got %d" % (n_local, n_local, r.shape[0]))
        f = cls.__new__(cls)
        f.ctx, f.cfg, f.first_slot, f.n_local, f.h = ctx, cfg, first_slot, n_local, None
        h, dropped, restored, unproved, rejected = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        ctx._ck(ctx.L.cp2_fill_resume_nodes(ctx.h, ctypes.byref(cfg), first_slot, n_local, _p(r) if r.size else None, os.fsencode(path),
                                            RESUME_TRUST_FILES if trust_files else 0, ctypes.byref(h), ctypes.byref(dropped), ctypes.byref(restored),
                                            ctypes.byref(unproved), ctypes.byref(rejected)), "cp2_fill_resume_nodes")
        f.h, f.n_dropped, f.n_restored, f.n_unproved, f.n_rejected = h, dropped.value, restored.value, unproved.value, rejected.value
        ctx._children.add(f)
        return f

    def save(self, path):
        """cp2_fill_save: a checkpoint of this unfinished session at `path` (written beside it and renamed)"""
        self.ctx._ck(self.ctx.L.cp2_fill_save(self.h, os.fsencode(path)), "cp2_fill_save")

    def save_nodes(self, path):
        """cp2_fill_save_nodes: a checkpoint of this unfinished keeping session at `path` with its known nodes (format CP2FILL2)"""
        self.ctx._ck(self.ctx.L.cp2_fill_save_nodes(self.h, os.fsencode(path)), "cp2_fill_save_nodes")

    def free(self):
        if self.h:
            self.ctx.L.cp2_fill_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if _finalizing():
                return
            self.free()
        except Exception:
            pass

    @property
    def block_proof_depth(self):
        return block_proof_depth(self.cfg.cell_size, self.cfg.block_size, self.cfg.n_cells)

    def add(self, slot_block, data, paths, status=None):
        """cp2_fill_add: blocks (n x blockSize bytes, any buffer numpy views without a copy) with their paths (uint8[n, depth, 32]) for
        (slot, block) pairs.  Returns (status: uint32[n] of FILL_*, n_new); `status` may be a caller's uint32[n] array to fill."""
        sb = np.ascontiguousarray(np.asarray(slot_block, dtype=np.uint64).reshape(-1, 2))
        n = sb.shape[0]
        d, p = _candidates("fill", data, n, self.cfg.block_size, paths, self.block_proof_depth)
        if status is None:
            status = np.empty(n, dtype=np.uint32)
        assert status.dtype == np.uint32 and status.flags["C_CONTIGUOUS"] and status.size == n
        new = ctypes.c_size_t()
        st = self.ctx.L.cp2_fill_add(self.h, _p(sb) if n else None, _p(d) if n else None, _p(p) if n else None, n, _p(status) if n else None,
                                     ctypes.byref(new))
        try:
            self.ctx._ck(st, "cp2_fill_add")
        except CodexP2Error as e:
            e.fill_status, e.n_new = status, new.value
            raise
        return status, new.value

    def add_multi(self, groups, blocks, data, nodes):
        """cp2_fill_add_multi: groups of blocks, each with its multiproof: groups = (dataset slot, count) pairs, blocks = the block indices
        group after group, strictly ascending inside a group, data = n x blockSize bytes in that order, nodes = the groups' rows packed
        (uint8[n_rows, 32]).  A group proves or fails as a whole.  Returns (status: uint32[n] of FILL_*, one per request, n_new)."""
        g, b = _groups(groups, blocks)
        n, ng = b.shape[0], g.shape[0]
        d = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
        if d.nbytes != n * self.cfg.block_size:
            raise ValueError("fill multi: %d request(s) need %d bytes of candidates, got %d" % (n, n * self.cfg.block_size, d.nbytes))
        rows = _u8(nodes).reshape(-1, 32)
        status = np.empty(n, dtype=np.uint32)
        new = ctypes.c_size_t()
        st = self.ctx.L.cp2_fill_add_multi(self.h, _p(g) if ng else None, ng, _p(b) if n else None, _p(d) if n else None,
                                           _p(rows) if rows.size else None, rows.shape[0], _p(status) if n else None, ctypes.byref(new))
        try:
            self.ctx._ck(st, "cp2_fill_add_multi")
        except CodexP2Error as e:
            e.fill_status, e.n_new = status, new.value
            raise
        return status, new.value

    def multiproof_want(self, groups, blocks):
        """cp2_fill_multiproof_want: (level_index: uint64[n_rows, 2], group_rows: uint64[n_groups]), the rows groups of blocks still need
        from a peer, laid out against what the session knows now: (level, index) pairs packed in group order; host only."""
        g, b = _groups(groups, blocks)
        n, ng = b.shape[0], g.shape[0]
        per = np.zeros(ng, dtype=np.uint64)
        n_rows = ctypes.c_size_t(0)
        L = self.ctx.L
        self.ctx._ck(L.cp2_fill_multiproof_want(self.h, _p(g) if ng else None, ng, _p(b) if n else None, None, 0, ctypes.byref(n_rows),
                                                _p(per) if ng else None), "cp2_fill_multiproof_want")
        li = np.zeros((n_rows.value, 2), dtype=np.uint64)
        if n_rows.value:
            self.ctx._ck(L.cp2_fill_multiproof_want(self.h, _p(g), ng, _p(b), _p(li), li.shape[0], ctypes.byref(n_rows), None), "cp2_fill_multiproof_want")
        return li, per

    def block_tree_rows(self, places, statuses_only=False):
        """cp2_fill_block_tree_rows: (status: uint32[n] of FILL_ROW_*, rows: uint8[n, 32]) of (dataset slot, level, index) places from the
        session's own buffer; an unknown row is zeros.  statuses_only: just the statuses, from the host bitmap, no device work."""
        pl = np.ascontiguousarray(np.asarray(places, dtype=np.uint64).reshape(-1, 3))
        n = pl.shape[0]
        status = np.empty(n, dtype=np.uint32)
        rows = None if statuses_only else np.empty((n, 32), dtype=np.uint8)
        self.ctx._ck(self.ctx.L.cp2_fill_block_tree_rows(self.h, _p(pl) if n else None, n, _p(status) if n else None,
                                                         _p(rows) if n and not statuses_only else None), "cp2_fill_block_tree_rows")
        return status if statuses_only else (status, rows)

    def add_multi_anchored(self, groups, blocks, data, nodes):
        """cp2_fill_add_multi_anchored: add_multi for a session that keeps nodes, with nodes = the rows of the groups' want lists
        (multiproof_want) packed in group order: what the session holds is neither sent nor hashed again.  Returns (status: uint32[n] of
        FILL_*, one per request, n_new)."""
        g, b = _groups(groups, blocks)
        n, ng = b.shape[0], g.shape[0]
        d = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
        if d.nbytes != n * self.cfg.block_size:
            raise ValueError("fill multi anchored: %d request(s) need %d bytes of candidates, got %d" % (n, n * self.cfg.block_size, d.nbytes))
        rows = _u8(nodes).reshape(-1, 32) if nodes is not None else np.empty((0, 32), dtype=np.uint8)   # (nothing wanted: nothing sent)
        status = np.empty(n, dtype=np.uint32)
        new = ctypes.c_size_t()
        st = self.ctx.L.cp2_fill_add_multi_anchored(self.h, _p(g) if ng else None, ng, _p(b) if n else None, _p(d) if n else None,
                                                    _p(rows) if rows.size else None, rows.shape[0], _p(status) if n else None, ctypes.byref(new))
        try:
            self.ctx._ck(st, "cp2_fill_add_multi_anchored")
        except CodexP2Error as e:
            e.fill_status, e.n_new = status, new.value
            raise
        return status, new.value

    def keep_nodes(self):
        """cp2_fill_keep_nodes: from here on every proved path leaves all its nodes in the session's buffer, and block_proofs serves"""
        self.ctx._ck(self.ctx.L.cp2_fill_keep_nodes(self.h), "cp2_fill_keep_nodes")

    def block_proofs(self, slot_block, statuses_only=False):
        """cp2_fill_block_proofs: (status: uint32[n] of FILL_PROOF_*, block_roots: uint8[n, 32], paths: uint8[n, depth, 32]) of (slot, block)
        pairs from the session's own buffer; the rows of a request that is not served are zeros.  statuses_only: just the statuses, from the
        host bitmaps, no device work."""
        sb = np.ascontiguousarray(np.asarray(slot_block, dtype=np.uint64).reshape(-1, 2))
        n, depth = sb.shape[0], self.block_proof_depth
        status = np.empty(n, dtype=np.uint32)
        roots = None if statuses_only else np.empty((n, 32), dtype=np.uint8)
        paths = None if statuses_only else np.empty((n, depth, 32), dtype=np.uint8)
        self.ctx._ck(self.ctx.L.cp2_fill_block_proofs(self.h, _p(sb) if n else None, n, _p(status) if n else None,
                                                      _p(roots) if n and not statuses_only else None,
                                                      _p(paths) if n and not statuses_only else None), "cp2_fill_block_proofs")
        return status if statuses_only else (status, roots, paths)

    def anchors(self, slot_block):
        """cp2_fill_anchors: uint32[n], per (slot, block) pair the lowest level at which the session knows the node above the block (0: its
        block root ... depth: only the stated slot root); host only.  A session that keeps no nodes answers depth throughout."""
        sb = np.ascontiguousarray(np.asarray(slot_block, dtype=np.uint64).reshape(-1, 2))
        n = sb.shape[0]
        levels = np.empty(n, dtype=np.uint32)
        self.ctx._ck(self.ctx.L.cp2_fill_anchors(self.h, _p(sb) if n else None, n, _p(levels) if n else None), "cp2_fill_anchors")
        return levels

    def add_anchored(self, slot_block, data, levels, paths, status=None):
        """cp2_fill_add_anchored: add() for blocks that bring only their levels[i] lowest siblings; `paths` holds them packed in request
        order (sum(levels) x 32 bytes; None when every level is 0).  Returns (status: uint32[n] of FILL_*, n_new)."""
        sb = np.ascontiguousarray(np.asarray(slot_block, dtype=np.uint64).reshape(-1, 2))
        n = sb.shape[0]
        d = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)   # (no copy: see _candidates)
        if d.nbytes != n * self.cfg.block_size:
            raise ValueError("fill: %d request(s) need %d bytes of candidates, got %d" % (n, n * self.cfg.block_size, d.nbytes))
        lv = np.ascontiguousarray(np.asarray(levels, dtype=np.uint32).reshape(-1))
        if lv.size != n:
            raise ValueError("fill: %d level(s) expected, got %d" % (n, lv.size))
        total = int(lv.astype(np.uint64).sum())
        p = _u8(paths) if paths is not None else np.empty(0, dtype=np.uint8)
        if p.size != total * 32:
            raise ValueError("fill: the levels ask for %d sibling(s) of 32 bytes, got %d bytes" % (total, p.size))
        if status is None:
            status = np.empty(n, dtype=np.uint32)
        assert status.dtype == np.uint32 and status.flags["C_CONTIGUOUS"] and status.size == n
        new = ctypes.c_size_t()
        st = self.ctx.L.cp2_fill_add_anchored(self.h, _p(sb) if n else None, _p(d) if n else None, _p(lv) if n else None, _p(p) if p.size else None,
                                              n, _p(status) if n else None, ctypes.byref(new))
        try:
            self.ctx._ck(st, "cp2_fill_add_anchored")
        except CodexP2Error as e:
            e.fill_status, e.n_new = status, new.value
            raise
        return status, new.value

    def adopt(self, first_slot=None, n_slots=0, no_read=False):
        """cp2_fill_adopt: the absent blocks the slot files of slots first_slot .. + n_slots (0: every local slot) cover are read, hashed and
        kept where the tree above them reaches a node the session knows, the stated slot root included; no_read judges what earlier calls
        read.  Returns (n_read, n_adopted); a file that cannot be synced raises with both in the error's `n_read` / `n_adopted`."""
        first = self.first_slot if first_slot is None else first_slot
        read, adopted = ctypes.c_uint64(), ctypes.c_uint64()
        st = self.ctx.L.cp2_fill_adopt(self.h, first, n_slots, ADOPT_NO_READ if no_read else 0, ctypes.byref(read), ctypes.byref(adopted))
        try:
            self.ctx._ck(st, "cp2_fill_adopt")
        except CodexP2Error as e:
            e.n_read, e.n_adopted = read.value, adopted.value
            raise
        return read.value, adopted.value

    def missing(self, cap=1 << 20):
        """cp2_fill_missing: (missing: uint64[k, 2] of (slot, block), ascending, the lowest k = min(cap, n_missing), n_missing); cap = 0 counts"""
        cap = int(cap)
        out = np.empty((cap, 2), dtype=np.uint64)
        n = ctypes.c_uint64()
        self.ctx._ck(self.ctx.L.cp2_fill_missing(self.h, _p(out) if cap else None, cap, ctypes.byref(n)), "cp2_fill_missing")
        return out[:min(cap, n.value)].copy(), n.value

    def finish(self, cache_path=None):
        """cp2_fill_finish: the compact Dataset of the filled slots (it takes the session's device buffer; the session then only frees)"""
        h = ctypes.c_void_p()
        self.ctx._ck(self.ctx.L.cp2_fill_finish(self.h, cache_path.encode() if cache_path else None, ctypes.byref(h)), "cp2_fill_finish")
        return Dataset.adopt(self.ctx, self.cfg, h, self.first_slot, self.n_local)


def fills_add_many(ctx, sessions, req, data, paths, levels=None):
    """cp2_fills_add_many: proved blocks added to many FillSessions of `ctx` in one pass.  req: uint64[n, 3] of (index into sessions,
    dataset slot, block); data: n x blockSize bytes; levels: uint32[n], or None when every request brings its session's whole path; paths:
    the siblings packed in request order (None when every level is 0).  Per session the meaning of FillSession.add / add_anchored on the
    requests that name it.  Returns (status: uint32[n] of FILL_*, n_new: list of len(sessions)); a file that cannot be written raises with
    both in the error's `fill_status` / `n_new`."""
    sessions = list(sessions)
    rq = np.ascontiguousarray(np.asarray(req, dtype=np.uint64).reshape(-1, 3))
    n, k = rq.shape[0], len(sessions)
    d = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)   # (no copy: see _candidates)
    lv = None if levels is None else np.ascontiguousarray(np.asarray(levels, dtype=np.uint32).reshape(-1))
    if lv is not None and lv.size != n:
        raise ValueError("fills: %d level(s) expected, got %d" % (n, lv.size))
    p = _u8(paths) if paths is not None else np.empty(0, dtype=np.uint8)
    hs = (ctypes.c_void_p * max(k, 1))(*[None if s is None else s.h for s in sessions])
    status = np.empty(n, dtype=np.uint32)
    new = (ctypes.c_size_t * max(k, 1))()
    st = ctx.L.cp2_fills_add_many(ctx.h, hs, k, _p(rq) if n else None, _p(d) if d.size else None, _p(lv) if lv is not None and n else None,
                                  _p(p) if p.size else None, n, _p(status) if n else None, new)
    try:
        ctx._ck(st, "cp2_fills_add_many")
    except CodexP2Error as e:
        e.fill_status, e.n_new = status, list(new)[:k]
        raise
    return status, list(new)[:k]


def fills_finish_many(ctx, sessions, cache_paths=None):
    """cp2_fills_finish_many: many complete FillSessions of `ctx` finished in one pass.  cache_paths: None, or one entry per session, each
    a path or None.  Per session the meaning of FillSession.finish(cache_path).  Returns the compact Datasets in the order of `sessions` and
    marks every session wrapper `finished`; all of them, or an error, no Dataset and every session as it was."""
    sessions = list(sessions)
    k = len(sessions)
    if cache_paths is not None and len(cache_paths) != k:
        raise ValueError("fills: %d cache path(s) expected, got %d" % (k, len(cache_paths)))
    hs = (ctypes.c_void_p * max(k, 1))(*[None if s is None else s.h for s in sessions])
    paths = None if cache_paths is None else (ctypes.c_char_p * max(k, 1))(*[None if p is None else os.fsencode(p) for p in cache_paths])
    out = (ctypes.c_void_p * max(k, 1))()
    ctx._ck(ctx.L.cp2_fills_finish_many(ctx.h, hs, k, paths, out), "cp2_fills_finish_many")
    for s in sessions:
        s.finished = True
    return [Dataset.adopt(ctx, s.cfg, ctypes.c_void_p(out[i]), s.first_slot, s.n_local) for i, s in enumerate(sessions)]


def fills_resume_many(ctx, cfgs, slot_roots, paths, ranges=None, trust_files=False):
    """cp2_fills_resume_many: many FillSessions of `ctx` resumed from their CP2FILL1 checkpoints in one pass.  cfgs, slot_roots and paths
    hold one entry per session; ranges: None (every session covers all slots of its cfg) or one (first_slot, n_local) per session.  Per
    session the meaning of Context.fill_resume; all of them, or an error and no session.  Returns (the FillSessions in the order of the
    entries, each with its `n_dropped`; n_dropped as a uint64 array)."""
    cfgs, paths, slot_roots = list(cfgs), list(paths), list(slot_roots)
    k = len(cfgs)
    if len(slot_roots) != k or len(paths) != k or (ranges is not None and len(ranges) != k):
        raise ValueError("fills: %d entries need as many slot_roots, paths and ranges" % k)
    # (thousands of entries: what is done per entry here is kept to a pointer and a size)
    if ranges is None:
        rg = np.array([(0, 0 if c is None else c.n_slots) for c in cfgs], dtype=np.uint64).reshape(-1, 2)
    else:
        rg = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
    n_local = rg[:, 1].tolist()
    roots = [r if r is None or (type(r) is np.ndarray and r.dtype == np.uint8 and r.flags.c_contiguous) else _u8(r) for r in slot_roots]
    for i, r in enumerate(roots):
        if r is not None and r.size != 32 * n_local[i]:
            raise ValueError("fills: entry %d: %d local slot(s) need %d roots, got %d" % (i, n_local[i], n_local[i], r.size // 32))
    cs = (ctypes.c_void_p * max(k, 1))(*[None if c is None else ctypes.addressof(c) for c in cfgs])
    rs = (ctypes.c_void_p * max(k, 1))(*[None if r is None or not r.size else r.__array_interface__["data"][0] for r in roots])
    ps = (ctypes.c_char_p * max(k, 1))(*[None if p is None else os.fsencode(p) for p in paths])
    out = (ctypes.c_void_p * max(k, 1))()
    dropped = np.zeros(k, dtype=np.uint64)
    st = ctx.L.cp2_fills_resume_many(ctx.h, cs, _p(rg) if k else None, rs, ps, k, RESUME_TRUST_FILES if trust_files else 0, out,
                                     _p(dropped) if k else None)
    ctx._ck(st, "cp2_fills_resume_many")
    sessions, first, handles, drops, new = [], rg[:, 0].tolist(), list(out), dropped.tolist(), FillSession.__new__
    for i in range(k):
        f = new(FillSession)
        f.__dict__.update(ctx=ctx, cfg=cfgs[i], first_slot=first[i], n_local=n_local[i], h=ctypes.c_void_p(handles[i]), n_dropped=drops[i])
        ctx._children.add(f)
        sessions.append(f)
    return sessions, dropped


GATHER_AUTO, GATHER_RCCL, GATHER_HOST, GATHER_COPY = 0, 1, 2, 3


def shard_range(n_items, rank, world):
    """cp2_shard_range: (first, count) of the contiguous range rank `rank` of `world` holds."""
    L = load_library()
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    L.cp2_shard_range(n_items, rank, world, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def multi_plan(cfg, n_devices, min_cells_per_device=0, units_per_slot=0):
    """cp2_multi_plan: (number of shards, units per slot) cp2_multi_dataset_build would use -- host-only arithmetic."""
    L = load_library()
    w, u = ctypes.c_int(), ctypes.c_uint64()
    st = L.cp2_multi_plan(ctypes.byref(cfg), n_devices, min_cells_per_device, units_per_slot, ctypes.byref(w), ctypes.byref(u))
    if st != CP2_OK:
        raise CodexP2Error(st, "cp2_multi_plan", L.cp2_strerror(st).decode())
    return w.value, u.value


class _BorrowedContext(Context):
    """A cp2_ctx owned by a cp2_multi (never freed from here)."""

    def __init__(self, L, h):
        self.L, self.h = L, h
        self._children = weakref.WeakSet()

    def close(self):
        _free_children(self)
        self.h = None


class Multi:
    """cp2_multi: one handle over several devices of the node (in-process sharding, include/codex_p2.h section e)."""

    def __init__(self, devices=None):
        self.L = load_library()
        h = ctypes.c_void_p()
        if devices:
            arr = (ctypes.c_int * len(devices))(*devices)
            st = self.L.cp2_multi_init(arr, len(devices), ctypes.byref(h))
        else:
            st = self.L.cp2_multi_init(None, 0, ctypes.byref(h))
        if st != CP2_OK:
            raise CodexP2Error(st, "cp2_multi_init", self.L.cp2_strerror(st).decode())
        self.h = h
        self._children = weakref.WeakSet()
        self._borrowed = {}

    def close(self):
        if self.h:
            _free_children(self)
            for c in self._borrowed.values():
                c.close()
            self._borrowed = {}
            self.L.cp2_multi_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if _finalizing():
                return
            self.close()
        except Exception:
            pass

    def _ck(self, st, where):
        if st != CP2_OK:
            raise CodexP2Error(st, where, self.L.cp2_multi_last_error(self.h).decode() or self.L.cp2_strerror(st).decode())

    @property
    def count(self):
        return self.L.cp2_multi_count(self.h)

    def devices(self):
        return [self.L.cp2_multi_device(self.h, i) for i in range(self.count)]

    def ctx(self, i=0):
        if i not in self._borrowed:
            h = self.L.cp2_multi_ctx(self.h, i)
            if not h:
                raise CodexP2Error(-2, "cp2_multi_ctx")
            self._borrowed[i] = _BorrowedContext(self.L, ctypes.c_void_p(h))   # one object per context: it tracks what was made through it
        return self._borrowed[i]

    def gather_mode(self):
        return self.L.cp2_multi_gather_mode(self.h).decode()

    def set_policy(self, gather=GATHER_AUTO, min_cells_per_device=0):
        self._ck(self.L.cp2_multi_set_policy(self.h, gather, min_cells_per_device), "cp2_multi_set_policy")

    def set_split(self, units_per_slot=0):
        """units every slot is cut into by Multi.dataset: 0 = choose, 1 = whole slots only, 2^k = exactly that"""
        self._ck(self.L.cp2_multi_set_split(self.h, units_per_slot), "cp2_multi_set_split")

    def dataset(self, cfg, cache=None):
        return MultiDataset(self, cfg, cache=cache)

    def dataset_streamed(self, cfg, entropy, threads=1, group_slots=0):
        return MultiDataset(self, cfg, streamed=(entropy, threads, group_slots))


class MultiDataset:
    def __init__(self, multi, cfg, cache=None, streamed=None):
        self.multi, self.cfg = multi, cfg
        L = multi.L
        h = ctypes.c_void_p()
        if streamed is not None:
            entropy, threads, group = streamed
            e = _u8(entropy if not isinstance(entropy, int) else felt_bytes(entropy))
            multi._ck(L.cp2_multi_dataset_build_streamed(multi.h, ctypes.byref(cfg), _p(e), threads, group, ctypes.byref(h)),
                      "cp2_multi_dataset_build_streamed")
        elif cache:
            multi._ck(L.cp2_multi_dataset_build_cached(multi.h, ctypes.byref(cfg), cache.encode(), ctypes.byref(h)), "cp2_multi_dataset_build_cached")
        else:
            multi._ck(L.cp2_multi_dataset_build(multi.h, ctypes.byref(cfg), ctypes.byref(h)), "cp2_multi_dataset_build")
        self.h = h
        multi._children.add(self)

    def free(self):
        if self.h:
            self.multi.L.cp2_multi_dataset_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if _finalizing():
                return
            self.free()
        except Exception:
            pass

    @property
    def units_per_slot(self):
        return self.multi.L.cp2_multi_dataset_units_per_slot(self.h)

    def shards(self):
        """[(device, first, count)] of every shard: slots, or units when units_per_slot > 1"""
        L, out = self.multi.L, []
        for i in range(L.cp2_multi_dataset_shards(self.h)):
            d, a, b = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
            L.cp2_multi_dataset_shard(self.h, i, ctypes.byref(d), ctypes.byref(a), ctypes.byref(b))
            out.append((d.value, a.value, b.value))
        return out

    def root(self):
        out = np.empty(32, dtype=np.uint8)
        self.multi._ck(self.multi.L.cp2_multi_dataset_root(self.h, _p(out)), "cp2_multi_dataset_root")
        return out

    def shard_root(self, i):
        """the dataset root as shard i's device computed it (every device builds the tree itself)"""
        L = self.multi.L
        ds = L.cp2_multi_dataset_shard(self.h, i, None, None, None)
        out = np.empty(32, dtype=np.uint8)
        self.multi._ck(L.cp2_dataset_root(ctypes.c_void_p(ds), _p(out)), "cp2_dataset_root")
        return out

    def slot_roots(self):
        out = np.empty((self.cfg.n_slots, 32), dtype=np.uint8)
        self.multi._ck(self.multi.L.cp2_multi_dataset_slot_roots(self.h, _p(out)), "cp2_multi_dataset_slot_roots")
        return out

    def proof_input(self, slot_idx, entropy):
        e = _u8(entropy if not isinstance(entropy, int) else felt_bytes(entropy))
        h = ctypes.c_void_p()
        self.multi._ck(self.multi.L.cp2_multi_proof_input_generate(self.h, slot_idx, _p(e), ctypes.byref(h)), "cp2_multi_proof_input_generate")
        pi = ProofInput(self.multi, h, self.cfg)
        pi.slot_idx = slot_idx
        return pi

    def export_proof_inputs(self, slot_indices, entropy, directory=None, threads=1, batch=0):
        e = _u8(entropy if not isinstance(entropy, int) else felt_bytes(entropy))
        idx = np.ascontiguousarray(np.asarray(slot_indices, dtype=np.uint64))
        total = ctypes.c_uint64()
        self.multi._ck(self.multi.L.cp2_multi_dataset_export_proof_inputs(self.h, _p(idx), idx.size, _p(e), directory.encode() if directory else None,
                                                                          threads, batch, ctypes.byref(total)), "cp2_multi_dataset_export_proof_inputs")
        return total.value

    def export_streamed(self, directory=None, threads=1):
        total = ctypes.c_uint64()
        self.multi._ck(self.multi.L.cp2_multi_dataset_export_streamed(self.h, directory.encode() if directory else None, threads,
                                                                      ctypes.byref(total)), "cp2_multi_dataset_export_streamed")
        return total.value

    def scrub(self, first_slot=None, n_slots=0, cap=1 << 20):
        """cp2_multi_dataset_scrub: Dataset.scrub over every shard (cut by units: cell indices of the slot)."""
        first = 0 if first_slot is None else first_slot
        return _scrub(self.multi.L.cp2_multi_dataset_scrub, self.h, first, n_slots, cap, self.multi._ck, "cp2_multi_dataset_scrub")

    def repair_blocks(self, slot_block, data, check_only=False, cache_path=None):
        """cp2_multi_dataset_repair_blocks: Dataset.repair_blocks over every shard (slots of the whole dataset)."""
        return _repair(self.multi.L.cp2_multi_dataset_repair_blocks, self.h, self.cfg.block_size, slot_block, data, check_only, cache_path,
                       self.multi._ck, "cp2_multi_dataset_repair_blocks")

    def streamed_json(self, slot_idx):
        text, ln = ctypes.c_void_p(), ctypes.c_size_t()
        self.multi._ck(self.multi.L.cp2_multi_dataset_streamed_json(self.h, slot_idx, ctypes.byref(text), ctypes.byref(ln)), "cp2_multi_dataset_streamed_json")
        s = ctypes.string_at(text, ln.value).decode()
        self.multi.L.cp2_free_buffer(text)
        return s


def write_json_batch(ctx, proof_inputs, paths=None, threads=1):
    """Serialise (and write, when paths are given) many proof inputs on host threads; returns total text bytes."""
    n = len(proof_inputs)
    hs = (ctypes.c_void_p * n)(*[p.h for p in proof_inputs])
    ps = None
    if paths is not None:
        ps = (ctypes.c_char_p * n)(*[(q.encode() if q else None) for q in paths])
    total = ctypes.c_uint64()
    ctx._ck(ctx.L.cp2_proof_inputs_write_json_batch(hs, n, ps, threads, ctypes.byref(total)), "cp2_proof_inputs_write_json_batch")
    return total.value


VERIFY_DATASET_ROOT, VERIFY_SAMPLE, VERIFY_SHAPE = 1, 2, 4     # CP2_VERIFY_* (include/codex_p2.h)


def parse_proof_input(cfg, text):
    """cp2_proof_input_parse_json: input.json text -> ProofInput (no context needed).  cfg gives maxDepth, maxLog2NSlots, cellSize,
    blockSize and nSamples (0: as many rows as the text has).  A text the parser refuses raises CodexP2Error naming the key / row."""
    L = load_library()
    raw = text.encode() if isinstance(text, str) else bytes(text)
    buf = ctypes.create_string_buffer(raw, len(raw))
    msg = ctypes.create_string_buffer(512)
    h = ctypes.c_void_p()
    st = L.cp2_proof_input_parse_json(ctypes.byref(cfg), buf, len(raw), ctypes.byref(h), msg, len(msg))
    if st != CP2_OK:
        raise CodexP2Error(st, "cp2_proof_input_parse_json", msg.value.decode(errors="replace"))
    c = Config()
    ctypes.pointer(c)[0] = cfg
    n_cells, n_slots, slot_idx = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    L.cp2_proof_input_shape(h, ctypes.byref(n_cells), ctypes.byref(n_slots), ctypes.byref(slot_idx))
    c.n_cells, c.n_slots, c.n_samples = n_cells.value, n_slots.value, L.cp2_proof_input_nsamples(h)
    pi = ProofInput(None, h, c)
    pi.slot_idx = slot_idx.value
    return pi


class ProofInput:
    """A cp2_proof_input.  Its accessors need no context (the library comes from load_library()); `ctx` is the context that made
    it, or None for a parsed one."""

    def __init__(self, ctx, h, cfg):
        self.ctx, self.h, self.cfg = ctx, h, cfg
        self.L = ctx.L if ctx is not None else load_library()

    def _ck(self, st, where):
        if st != CP2_OK:
            raise CodexP2Error(st, where, self.L.cp2_strerror(st).decode())

    def free(self):
        if self.h:
            self.L.cp2_proof_input_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if _finalizing():
                return
            self.free()
        except Exception:
            pass

    def _arr(self, ptr, shape, dtype=np.uint8):
        """A copy of the array at ptr, or None where the object has none (a parsed object's cell indices and leaf hashes, and
        its cell bytes when some row encodes no bytes)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if n == 0:
            return np.zeros(shape, dtype=dtype)
        if not ptr:
            return None
        buf = (ctypes.c_uint8 * n).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype).reshape(shape).copy()

    def roots(self):
        d, s, e = (np.empty(32, dtype=np.uint8) for _ in range(3))
        self._ck(self.L.cp2_proof_input_roots(self.h, _p(d), _p(s), _p(e)), "cp2_proof_input_roots")
        return d, s, e

    def cell_indices(self):
        n = self.L.cp2_proof_input_nsamples(self.h)
        return self._arr(self.L.cp2_proof_input_cell_indices(self.h), (n,), np.uint64)

    def cell_data(self):
        n = self.L.cp2_proof_input_nsamples(self.h)
        return self._arr(self.L.cp2_proof_input_cell_data(self.h), (n, self.cfg.cell_size))

    def merkle_paths(self):
        n = self.L.cp2_proof_input_nsamples(self.h)
        return self._arr(self.L.cp2_proof_input_merkle_paths(self.h), (n, self.cfg.max_depth, 32))

    def slot_proof(self):
        return self._arr(self.L.cp2_proof_input_slot_proof(self.h), (self.cfg.max_log2_nslots, 32))

    def nsamples(self):
        return int(self.L.cp2_proof_input_nsamples(self.h))

    def shape(self):
        """(nCellsPerSlot, nSlotsPerDataSet, slotIndex) as the object holds them."""
        v = [ctypes.c_uint64() for _ in range(3)]
        self._ck(self.L.cp2_proof_input_shape(self.h, *[ctypes.byref(x) for x in v]), "cp2_proof_input_shape")
        return tuple(x.value for x in v)

    def cell_felts(self):
        """The sampled cells as the circuit reads them: uint8[nSamples, cp2_felts_per_bytes(cellSize), 32]."""
        n = self.nsamples()
        out = np.zeros((n, self.L.cp2_felts_per_bytes(self.cfg.cell_size), 32), dtype=np.uint8)
        self._ck(self.L.cp2_proof_input_cell_felts(self.h, _p(out)), "cp2_proof_input_cell_felts")
        return out

    def leaf_hashes(self):
        n = self.L.cp2_proof_input_nsamples(self.h)
        return self._arr(self.L.cp2_proof_input_leaf_hashes(self.h), (n, 32))

    def recreate(self):
        """A copy made through cp2_proof_input_create from this object's accessor arrays (what the Nim shim's
        exportProofInputBN254 does with a SlotProofInput value)."""
        d, s, e = self.roots()
        sp, idx, cells, paths, leaves = (np.ascontiguousarray(a) for a in
                                         (self.slot_proof(), self.cell_indices(), self.cell_data(), self.merkle_paths(), self.leaf_hashes()))
        slot_idx = getattr(self, "slot_idx", 0)
        h = ctypes.c_void_p()
        self._ck(self.L.cp2_proof_input_create(ctypes.byref(self.cfg), slot_idx, _p(d), _p(e), _p(s), _p(sp), idx.size,
                                                       _p(idx), _p(cells), _p(paths), _p(leaves), ctypes.byref(h)), "cp2_proof_input_create")
        q = ProofInput(self.ctx, h, self.cfg)
        q.slot_idx = slot_idx
        return q

    def json(self):
        text, ln = ctypes.c_void_p(), ctypes.c_size_t()
        self._ck(self.L.cp2_proof_input_json(self.h, ctypes.byref(text), ctypes.byref(ln)), "cp2_proof_input_json")
        s = ctypes.string_at(text, ln.value).decode()
        self.L.cp2_free_buffer(text)
        return s

    def write_json(self, path):
        self._ck(self.L.cp2_proof_input_write_json(self.h, path.encode()), "cp2_proof_input_write_json")


def write_circom_main(cfg, path):
    L = load_library()
    st = L.cp2_write_circom_main(ctypes.byref(cfg), path.encode())
    if st != CP2_OK:
        raise CodexP2Error(st, "cp2_write_circom_main", L.cp2_strerror(st).decode())
