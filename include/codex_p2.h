/* codex_p2.h -- C ABI of libcodex_p2.so: the MI355X (gfx950) Poseidon2-BN254 proof-input engine.
 *
 * This is the drop-in boundary for the hot path of codex-storage/codex-storage-proofs-circuits'
 * `reference/nim/proof_input` tool (BN254 / Poseidon2 only).  The reference has no FFI for this path:
 * its seam is the set of nim-poseidon2 / constantine calls made from `reference/nim/proof_input/src`
 * (SURVEY.md section 8b).  Each entry point below names the reference call it replaces
 * (paths relative to the reference repository root).  INTEGRATION.md shows the Nim `importc` shim.
 *
 * Conventions
 *   - A field element (Fr of BN254) crosses the ABI as 32 bytes, little-endian, canonical integer in
 *     [0, r).  Inputs >= r are accepted and taken mod r.  Never Montgomery limbs.
 *   - Every function returns CP2_OK (0) or a negative cp2_status; nothing aborts across the ABI
 *     (the reference's `assert`s map to CP2_ERR_INVALID; the Nim shim turns non-zero into raiseAssert).
 *   - Plain functions take HOST pointers and are synchronous: inputs are copied to the GPU, the HIP
 *     kernels run, outputs are copied back before return.
 *   - `_dev` functions take HIP DEVICE pointers (16-byte aligned), enqueue on the context's stream and
 *     return without synchronising; use cp2_sync().
 *   - One context per host thread; contexts are independent.  There is no CPU fallback: without a
 *     usable gfx950 device cp2_init fails with CP2_ERR_NO_DEVICE.
 */
#ifndef CODEX_P2_H
#define CODEX_P2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CP2_FELT_BYTES 32

/* ---- version of this boundary --------------------------------------------------------------
 * Callers bind the entry points BY NAME at load time (the Nim `dynlib` binding nim/codex_p2.nim, the ctypes binding, dlopen), so
 * nothing but this number tells a caller built against one header from a library built from another.
 *   MAJOR  changes when an existing entry point, struct or status code changes meaning or layout, or one is removed: a caller built
 *          for another major MUST refuse the library (every binding in this repository does, naming both numbers).  The library's
 *          SONAME carries it: libcodex_p2.so.<MAJOR>.
 *   MINOR  grows with every release that only ADDS entry points; a caller needs library minor >= the minor it was written against.
 * cp2_abi_version() returns what the LIBRARY was built from: (MAJOR << 16) | MINOR.  It touches no device and needs no context.
 * History: 1.0 = the 105 entry points of round 5 + this function + cp2_set_ingest's two rings (round 6).
 *          1.1 = + cp2_proof_input_parse_json, _shape, _cell_felts and cp2_proof_inputs_verify (verification).
 *          1.2 = + cp2_proof_inputs_generate_many and cp2_proof_inputs_export_many (proof inputs across datasets).
 *          next: + cp2_dataset_scrub, cp2_multi_dataset_scrub and cp2_datasets_scrub_many (scrub), cp2_dataset_repair_blocks and
 *                cp2_multi_dataset_repair_blocks (repair), cp2_block_proof_depth, cp2_dataset_block_proofs, cp2_blocks_verify and
 *                cp2_dataset_repair_blocks_proved (block proofs), cp2_fill_begin, cp2_fill_add, cp2_fill_missing, cp2_fill_finish and
 *                cp2_fill_free (fill sessions), cp2_fill_save and cp2_fill_resume (fill checkpoints), cp2_fill_keep_nodes and
 *                cp2_fill_block_proofs (fill sessions that serve), cp2_fill_anchors and cp2_fill_add_anchored (anchored fill adds),
 *                cp2_fill_adopt (adopting blocks from disk), cp2_fill_save_nodes and cp2_fill_resume_nodes (checkpoints with nodes),
 *                cp2_datasets_read_blocks and cp2_dataset_read_blocks (verified read-back of listed blocks),
 *                cp2_datasets_build_many (many datasets built in one pass), cp2_datasets_set_roots_many (their dataset trees in one pass),
 *                cp2_fills_add_many (proved blocks added to many fill sessions in one pass), cp2_fills_finish_many (many fill
 *                sessions finished in one pass), cp2_fills_resume_many (many fill sessions resumed in one pass),
 *                cp2_datasets_repair_blocks_many (many datasets repaired in one pass), cp2_block_multiproof_rows,
 *                cp2_block_multiproof_layout, cp2_dataset_block_multiproofs, cp2_blocks_verify_multi and cp2_fill_add_multi
 *                (block multiproofs), cp2_fill_multiproof_want, cp2_dataset_block_tree_rows, cp2_fill_block_tree_rows and
 *                cp2_fill_add_multi_anchored (multiproofs against what a fill session knows).
 *                MINOR stays 2 until the release that carries them: the bump to 1.3 goes in its own commit with that release.         */
#define CP2_ABI_VERSION_MAJOR 1
#define CP2_ABI_VERSION_MINOR 2
#define CP2_ABI_VERSION ((CP2_ABI_VERSION_MAJOR << 16) | CP2_ABI_VERSION_MINOR)
int cp2_abi_version(void);

typedef enum cp2_status {
  CP2_OK = 0,
  CP2_ERR_INVALID = -1,    /* bad argument (the reference would fail an assert)            */
  CP2_ERR_NO_DEVICE = -2,  /* no usable HIP device / wrong architecture                    */
  CP2_ERR_HIP = -3,        /* a HIP runtime call failed; see cp2_last_error                */
  CP2_ERR_ALLOC = -4,      /* host or device allocation failed                             */
  CP2_ERR_IO = -5,         /* file could not be read / written                             */
  CP2_ERR_ALIGN = -6       /* a _dev pointer is not 16-byte aligned                        */
} cp2_status;

typedef struct cp2_ctx cp2_ctx;

/* ---- context ------------------------------------------------------------------------------ */
int cp2_init(int device, cp2_ctx** out);
void cp2_free(cp2_ctx* ctx);
/* Use a caller-owned HIP stream (hipStream_t) for all work of this context.  The handle is used as is:
 * NULL is HIP's legacy default stream (what torch.cuda.current_stream().cuda_stream returns by default).
 * cp2_reset_stream goes back to the context's own non-blocking stream. */
int cp2_set_stream(cp2_ctx* ctx, void* hip_stream);
int cp2_reset_stream(cp2_ctx* ctx);
int cp2_sync(cp2_ctx* ctx);
const char* cp2_strerror(int status);
const char* cp2_last_error(const cp2_ctx* ctx);
/* 1 when the library's kernels were built for the device of `ctx` (gfx950). */
int cp2_device_is_native(const cp2_ctx* ctx);
/* The environment variables the library reads are parsed STRICTLY: each holds exactly what it takes, or cp2_init / cp2_multi_init
 * fail with CP2_ERR_INVALID -- a mistyped knob is never read as "automatic".  cp2_check_environment (host only: no device is
 * touched, so it also answers on a box without a GPU) returns CP2_OK, or CP2_ERR_INVALID with the first offending variable, its
 * value and what it takes in `msg` (may be NULL).  The variables:
 *   CODEX_P2_GPUS        "all" | a device count | a comma-separated list of device indices      (cp2_multi_init)
 *   CODEX_P2_GATHER      "auto" | "rccl" | "copy" | "host"                                       (cp2_multi_set_policy)
 *   CODEX_P2_MIN_CELLS   a decimal number                                                        (cp2_multi_set_policy)
 *   CODEX_P2_SPLIT       0, 1 or a power of two                                                  (cp2_multi_set_split)
 *   CODEX_P2_KEEP_TREES  "auto" | "1" | "2" | "0"                                                (cp2_set_keep_trees)
 *   CODEX_P2_EXCHANGE_TIMEOUT_S  seconds the exchange of slot roots may take (default 120; 0 = no limit)
 *   CODEX_P2_STAGE_MB    MiB of device staging per chunk of generated cells (default 2048; cp2_init); a compact / roots-only build
 *                        holds half of it in tree nodes per batch
 *   CODEX_P2_MEM_LIMIT_MB        (tests) a cap, in MiB per device, on the device memory this process may hold through the library:
 *                        the automatic residency choice sees min(free, cap left) and an allocation beyond the cap fails like a real
 *                        out-of-memory, so all residency modes and the fallback between them can be reached on an empty 288 GB device
 * Test hooks the shipped library also reads (they exist so that branches a healthy MI355X never takes can be reached by the suite;
 * none of them can change a result, only which path produces it or turn a run into an error):
 *   CODEX_P2_TEST_LDS_LIMIT      a decimal number of bytes: the LDS per workgroup cp2_init's launch-shape decision sees (65536 makes
 *                        the hash launches of the streamed builds hold every workgroup slot instead of leaving room; parsed strictly)
 *   CODEX_P2_TEST_OPTIMISTIC     "1": the automatic residency choice starts at "every node" without looking at the device, so that
 *                        the step-down chain is what finds the mode that fits (anything else: ignored)
 *   CODEX_P2_TEST_EXCHANGE_FAULT "hang_init" | "hang_collective" | "corrupt": the multi-device exchange of slot roots stalls at
 *                        that point or delivers wrong rows (cp2_multi_*; anything else: ignored)
 * and the A/B knobs of the measurement tools, read leniently (anything but the value named means "off"): CP2_STREAM_SERIAL=1,
 * CP2_STREAM_RAMP=0, CP2_HASH_BLOCK=64, CP2_INGEST_COPY_STREAM=1 (the ingestion pipe's uploads on a stream of their own, as until
 * round 6, instead of on the chunk's own hashing stream), CP2_TRACE (any value: stage timings on stderr). */
int cp2_check_environment(char* msg, size_t msg_len);
/* Tuning of the host -> GPU ingestion pipe used by cp2_slot_trees_build_host, cp2_hash_cells (large inputs) and the
 * SlotFile data source (the reference reads one cell per call, reference/nim/proof_input/src/slot.nim:57-68):
 * host threads filling the pinned ring, ring depth (2..8) and bytes per chunk.  0 = keep the default
 * (environment CP2_INGEST_THREADS / CP2_INGEST_RING / CP2_INGEST_CHUNK_MB, else 8 threads, depth 3 and one full
 * residency of the hash kernel per chunk: 768 x 256 cells, 384 MiB at 2 KiB cells; the streamed builds, whose launches leave room
 * for their small kernels, take 768 MiB: three waves of workgroups at that occupancy).  `ring_depth` pinned host buffers
 * (free again as soon as their upload is done) feed ring_depth + 1 device buffers (one landing, two being hashed, slack).
 * A chunk is a range of the BATCH's cells: it holds many small slot files, or a piece of a large one.  Memory: ring_depth x chunk of
 * pinned host memory + (ring_depth + 1) x chunk of device memory while a build runs (2.25 + 3 GiB at the streamed builds' default),
 * cached by the context afterwards (cp2_trim); when the host or the device cannot give that much the chunk is halved until it fits. */
int cp2_set_ingest(cp2_ctx* ctx, int fill_threads, int ring_depth, size_t chunk_bytes);
/* SlotFile source: read the slot files with O_DIRECT (block-aligned requests straight into the pinned ring, no page-cache copy
 * and no eviction of what the cache holds): for files that are NOT cached -- a cached file reads faster through the cache.
 * on = 1 / 0; -1 = the environment variable CP2_INGEST_DIRECT (default off).  A file system that refuses O_DIRECT is read
 * buffered; results are identical either way. */
int cp2_set_ingest_direct(cp2_ctx* ctx, int on);
/* SlotFile source, opt-in: chunks of a slot file that sit in the PAGE CACHE go to the device without a CPU copy -- the file is
 * mmap'ed read-only, a chunk that starts and ends on page boundaries and whose pages are resident (mincore, sampled) is registered
 * with the runtime (the page-cache pages themselves are pinned) and uploaded straight from the mapping by the copy engine, instead
 * of being pread into the pinned ring first.  Registrations are held until the build's ingestion ends (at most 32 GiB at a time).
 * Any other chunk -- not cached, not on page boundaries, past the end of the file, or the runtime refuses to register file pages
 * (RLIMIT_MEMLOCK and the like) -- goes through the ring as before; the two mix chunk by chunk, results are identical.  On one
 * device the throughput equals the ring's (the hash kernel bounds both: DESIGN.md section 6); what it saves is host threads
 * copying and two thirds of the host memory traffic.  on = 1 / 0; -1 = the environment variable CP2_INGEST_MAPPED (default OFF).
 * Not used together with O_DIRECT. */
int cp2_set_ingest_mapped(cp2_ctx* ctx, int on);
/* Memory a long-lived context holds.  Scratch blocks (device staging, pinned landing zones) are cached per context so that
 * repeated calls stop allocating: up to 6 GiB of device memory and 4 GiB of PINNED host memory stay with the context after
 * the calls that needed them.  cp2_trim waits for the context's streams and gives all cached blocks back to the system
 * (blocks still referenced by live proof inputs return when those are freed); the next call allocates again. */
int cp2_trim(cp2_ctx* ctx);
/* Host memory of the streamed proof-input path (cp2_dataset_build_streamed): the JSON body of every local slot (about 0.7 MB
 * at nSamples = 100, cellSize = 2048) is kept until the dataset is freed.  Bodies beyond `max_resident_bytes` per dataset are
 * written to files instead and read back by cp2_dataset_export_streamed / cp2_dataset_streamed_json.  The files hold sampled
 * cell data: they live in a private directory "<spill_dir>/cp2_bodies_XXXXXX" made by mkdtemp (mode 0700), each created with
 * O_EXCL | O_NOFOLLOW and mode 0600; files and directory are removed by cp2_dataset_free.  Defaults: 4 GiB (environment
 * CP2_BODY_BUDGET_MB), spill_dir NULL = $TMPDIR or /tmp.  max_resident_bytes = 0 keeps the current budget; (size_t)-1 = never
 * spill.  A spill that fails is CP2_ERR_IO with the path in cp2_last_error. */
int cp2_set_body_budget(cp2_ctx* ctx, size_t max_resident_bytes, const char* spill_dir);
/* Device memory of cp2_dataset_build.  Three ways to hold the slot trees of a dataset, same results from each:
 *   1  every node resident (3.1 % of the data: 256 MiB per 8 GiB slot): a proof input for any entropy costs two permutations
 *      per sample plus gathers;
 *   2  COMPACT: of every slot tree only the part from the block roots up stays (8 MiB per 8 GiB slot, 1/32 of the above); the
 *      bottom of each path is recomputed from the <= nSamples touched network blocks (regenerated, or read from the slot file:
 *      100 x 64 KiB), whose rebuilt roots are checked against the stored ones (a mismatch is CP2_ERR_IO: the slot data changed):
 *      a few ms per proof input; 4096 slots of 8 GiB hold 32 GiB of device memory instead of 1 TiB;
 *   0  ROOTS ONLY: the 32-byte slot roots stay; cp2_proof_input_generate rebuilds the whole tree of the slot it proves (0.2 s per
 *      8 GiB slot; the reference rebuilds it once per SAMPLE, gen_input/bn254.nim:57).
 * For 2 and 0 the trees are built batch by batch (about 2 GiB of nodes) in the context's scratch, what is kept is copied out, the
 * rest dropped (the copy-out of one batch overlaps the hashing of the next).  mode -1 (default): the environment variable
 * CODEX_P2_KEEP_TREES ("0" / "1" / "2"; "auto" = unset), else the most that fits what the device has free (1, else 2, else 0) --
 * divided by the number of contexts a cp2_multi has placed on that device.  The figure is a snapshot: another tenant of the
 * device (a second process, a framework's caching allocator) can take the memory between the choice and the allocation.  When
 * the mode was chosen AUTOMATICALLY and the build then fails with CP2_ERR_ALLOC, everything is freed, the context's cached
 * scratch is handed back (cp2_trim) and the build is retried one mode down (1 -> 2 -> 0); CP2_TRACE says so, and
 * cp2_dataset_keeps_trees tells what a built dataset did.  A mode the caller named is never changed.  The streamed build follows
 * the same rule (the bodies of a batch of slots are made while its trees exist: every proof input of 4096 slots of 8 GiB in one
 * pass over the data).  cp2_dataset_build_cached caches what the dataset keeps: every node, or -- 1/32 of that -- the compact
 * layers, or the roots; a later run loads them and, compact, proves from the touched blocks alone.  On a roots-only dataset every
 * cp2_proof_input_generate costs one slot rebuild, and the batch / export calls one per slot: to get the proof inputs of ALL
 * slots use the streamed build. */
int cp2_set_keep_trees(cp2_ctx* ctx, int mode);

/* ---- a1: Poseidon2 t=3 permutation --------------------------------------------------------- */
/* replaces nim-poseidon2 `perm` as specified by reference/haskell/src/Poseidon2/Permutation.hs:40-45.
 * in/out: n states of 3 field elements (n x 96 bytes).  Host arrays of more than 2^20 states stream through the device in
 * chunks (upload, kernel and download overlapped); arrays the caller has pinned (hipHostMalloc, hipHostRegister) are read and
 * written in place by the copy engines, pageable ones pass through a pinned ring filled by host threads. */
int cp2_permute_batch(cp2_ctx* ctx, const uint8_t* in, uint8_t* out, size_t n);
int cp2_permute_batch_dev(cp2_ctx* ctx, const void* d_in, void* d_out, size_t n);

/* ---- a6: keyed compression ----------------------------------------------------------------- */
/* replaces `compress(x, y, key = toF(key))`, reference/nim/proof_input/src/merkle/bn254.nim:18,50,53.
 * xy: n pairs (n x 64 bytes); key in {0,1,2,3}; out: n x 32 bytes. */
int cp2_compress_batch(cp2_ctx* ctx, const uint8_t* xy, uint32_t key, uint8_t* out, size_t n);

/* ---- a3: sponge over field elements --------------------------------------------------------- */
/* replaces `Sponge.digest(seq[F], rate = 2)`, reference/nim/proof_input/src/sample/bn254.nim:23. */
int cp2_sponge2_felts(cp2_ctx* ctx, const uint8_t* felts, size_t n, uint8_t out[32]);
/* batched: nitems inputs of nf elements each -> nitems digests */
int cp2_sponge2_felts_batch(cp2_ctx* ctx, const uint8_t* felts, size_t nf, size_t nitems, uint8_t* out);
int cp2_sponge2_felts_batch_dev(cp2_ctx* ctx, const void* d_felts, size_t nf, size_t nitems, void* d_out);

/* ---- a4: bytes -> field elements (host only, no device work) --------------------------------- */
/* replaces the iterator `elements(bytes, F)`, reference/nim/proof_input/src/json/bn254.nim:11,25
 * (10* byte padding, 31-byte little-endian chunks; reference/haskell/src/Slot.hs:243-270). */
size_t cp2_felts_per_bytes(size_t len);
int cp2_bytes_to_felts(const uint8_t* data, size_t len, uint8_t* out /* cp2_felts_per_bytes(len) x 32 */);

/* ---- a5: hashCell ---------------------------------------------------------------------------- */
/* replaces `Sponge.digest(cellData, rate = 2)` over bytes, reference/nim/proof_input/src/blocks/bn254.nim:27.
 * cells: n_cells contiguous cells of cell_size bytes; out: n_cells x 32 bytes. */
int cp2_hash_cells(cp2_ctx* ctx, const uint8_t* cells, size_t cell_size, size_t n_cells, uint8_t* out);
int cp2_hash_cells_dev(cp2_ctx* ctx, const void* d_cells, size_t cell_size, size_t n_cells, void* d_out);
/* one byte string of any length (same function with n_cells = 1) */
int cp2_hash_bytes(cp2_ctx* ctx, const uint8_t* data, size_t len, uint8_t out[32]);

/* ---- a7: Merkle tree -------------------------------------------------------------------------- */
/* replaces `merkleTreeBN254(xs)`, reference/nim/proof_input/src/merkle/bn254.nim:62-63 (all layers,
 * bottom first; keys 1/0 and odd keys 3/2; a singleton still gets one compression).
 * cp2_merkle_total(n) = number of elements over all layers; layers_out holds that many x 32 bytes.
 * layer_sizes (may be NULL) receives the element count of each layer; *n_layers their number. */
size_t cp2_merkle_total(size_t n);
size_t cp2_merkle_num_layers(size_t n);
int cp2_merkle_tree(cp2_ctx* ctx, const uint8_t* leaves, size_t n, uint8_t* layers_out, size_t* layer_sizes,
                    size_t* n_layers);
/* nseg independent trees of n leaves each (d_leaves: nseg x n elements, tree after tree).
 * d_layers_out: nseg x cp2_merkle_total(n) elements, LAYER-major: layer k of all trees is contiguous
 * (it starts at element nseg * (size_0 + ... + size_{k-1})), tree s at offset s * size_k inside it.
 * d_layers_out may equal d_leaves (the leaves are then layer 0 in place). */
int cp2_merkle_trees_dev(cp2_ctx* ctx, const void* d_leaves, size_t n, size_t nseg, void* d_layers_out);
/* replaces `Merkle.digest(xs)`, reference/nim/proof_input/src/merkle/bn254.nim:20 */
int cp2_merkle_root(cp2_ctx* ctx, const uint8_t* leaves, size_t n, uint8_t out[32]);

/* ---- a10: fake slot data ---------------------------------------------------------------------- */
/* replaces `genFakeCell`, reference/nim/proof_input/src/slot.nim:23-32, for cells first..first+n-1.
 * `seed` is the slot's own seed; cp2_slot_seed = parametricSlotSeed, dataset.nim:32. */
uint64_t cp2_slot_seed(uint64_t dataset_seed, uint64_t slot_idx);
int cp2_gen_fake_cells(cp2_ctx* ctx, uint64_t seed, uint64_t first, size_t n, size_t cell_size, uint8_t* out);
int cp2_gen_fake_cells_dev(cp2_ctx* ctx, uint64_t seed, uint64_t first, size_t n, size_t cell_size, void* d_out);

/* ---- a12: sampling ---------------------------------------------------------------------------- */
/* replaces `cellIndices`, reference/nim/proof_input/src/sample/bn254.nim:16-27 (counters 1..n_samples).
 * n_cells must be a power of two and at least 2 (`extractLowBits` asserts k > 0, types/bn254.nim:48). */
int cp2_cell_indices(cp2_ctx* ctx, const uint8_t entropy[32], const uint8_t slot_root[32], uint64_t n_cells,
                     size_t n_samples, uint64_t* out);

/* ---- a8/a9/a13: slot trees (device resident) --------------------------------------------------- */
/* A batch of `n_slots` slot trees of identical geometry, as built by `buildSlotTreeFull`,
 * reference/nim/proof_input/src/gen_input/bn254.nim:21-30: per block a tree over its cell hashes
 * (bottom key 1), then per slot a tree over the block roots (bottom key 1 again). */
typedef struct cp2_slot_trees cp2_slot_trees;

/* slots first_slot..first_slot+n_slots-1 of a fake-data dataset (cells generated on the device) */
int cp2_slot_trees_build_fake(cp2_ctx* ctx, uint64_t dataset_seed, uint64_t first_slot, size_t n_slots,
                              size_t cell_size, size_t block_size, size_t n_cells, cp2_slot_trees** out);
/* The same for UNITS: every slot cut into `units_per_slot` (a power of two) pieces of `cells_per_unit` cells -- whole blocks,
 * at least two, a power of two of them -- and this batch holding units first_unit .. first_unit + n_units - 1 of the dataset
 * (unit u = cells [(u mod units_per_slot) x cells_per_unit, + cells_per_unit) of slot u / units_per_slot).  The root of a unit is
 * the node of its slot's tree above those cells, so several devices can share ONE slot (section e, "by units"; SURVEY.md 8e:
 * "within one very large slot the same scheme applies one level down").  cp2_slot_trees_roots / _paths address units as
 * slots of cells_per_unit cells.  cp2_slot_trees_save / _load carry unit batches too (the file records units_per_slot). */
int cp2_slot_trees_build_fake_units(cp2_ctx* ctx, uint64_t dataset_seed, uint64_t units_per_slot, uint64_t first_unit, size_t n_units,
                                    size_t cell_size, size_t block_size, size_t cells_per_unit, cp2_slot_trees** out);
/* units of slot files "<file_base><slot>.dat" (dataset.nim:34): unit u is read at byte offset (u mod units_per_slot) x
 * cells_per_unit x cell_size of the file of slot u / units_per_slot */
int cp2_slot_trees_build_file_units(cp2_ctx* ctx, const char* file_base, uint64_t units_per_slot, uint64_t first_unit, size_t n_units,
                                    size_t cell_size, size_t block_size, size_t cells_per_unit, cp2_slot_trees** out);
/* n_slots slots whose cells are already in device memory, slot-major (n_slots x n_cells x cell_size bytes).
 * A `_dev`-style call: the hashing is ENQUEUED on the context's stream and the call returns without synchronising
 * (the cells must stay valid until then).  cp2_sync, cp2_slot_trees_roots and cp2_slot_trees_paths synchronise;
 * a launch failure is reported by whichever of them runs first (cp2_last_error). */
int cp2_slot_trees_build_dev(cp2_ctx* ctx, const void* d_cells, size_t n_slots, size_t cell_size, size_t block_size,
                             size_t n_cells, cp2_slot_trees** out);
/* same from host memory (streamed through a pinned staging buffer) */
int cp2_slot_trees_build_host(cp2_ctx* ctx, const uint8_t* cells, size_t n_slots, size_t cell_size,
                              size_t block_size, size_t n_cells, cp2_slot_trees** out);
void cp2_slot_trees_free(cp2_slot_trees* t);
/* Persisted trees (the reference recomputes every tree on every run and once more per
 * sample, gen_input/bn254.nim:42,57).  The file holds the geometry, the data-source description and every
 * node; loading it skips all cell hashing.  Trees built from caller memory (build_dev / build_host) load
 * without a cell source: paths work, sampled-cell retrieval needs cp2_slot_trees_attach_cells first. */
int cp2_slot_trees_save(cp2_slot_trees* t, const char* path);
int cp2_slot_trees_load(cp2_ctx* ctx, const char* path, cp2_slot_trees** out);
int cp2_slot_trees_attach_cells(cp2_slot_trees* t, const uint8_t* host_cells, const void* dev_cells);
size_t cp2_slot_trees_count(const cp2_slot_trees* t);
size_t cp2_slot_trees_depth(const cp2_slot_trees* t);   /* log2(cellsPerBlock) + log2(nBlocks) */
/* roots of all slots in the batch (n_slots x 32 bytes): `treeRoot(bigTree)`, merkle.nim:14-17 */
int cp2_slot_trees_roots(cp2_slot_trees* t, uint8_t* out);
/* device pointer to the same roots (n_slots x 32 bytes, canonical), valid until free */
const void* cp2_slot_trees_roots_dev(const cp2_slot_trees* t);
/* merged bottom+top Merkle paths (merkleProof + mergeMerkleProofs, merkle.nim:21-42,86-100) of
 * n cells of slot `slot` (index inside the batch), padded with zeros to max_depth (types.nim:27-37).
 * out: n x max_depth x 32 bytes; leaf_hashes (may be NULL): n x 32 bytes. */
int cp2_slot_trees_paths(cp2_slot_trees* t, size_t slot, const uint64_t* cell_idx, size_t n, size_t max_depth,
                         uint8_t* out, uint8_t* leaf_hashes);

/* ---- a14/a15: proof input ----------------------------------------------------------------------- */
/* mirrors GlobalConfig + DataSetConfig, reference/nim/proof_input/src/types.nim:82-101 */
typedef struct cp2_config {
  int32_t max_depth;        /* GlobalConfig.maxDepth                                 */
  int32_t max_log2_nslots;  /* GlobalConfig.maxLog2NSlots                            */
  uint64_t cell_size;       /* GlobalConfig.cellSize                                 */
  uint64_t block_size;      /* GlobalConfig.blockSize                                */
  uint64_t n_slots;         /* DataSetConfig.nSlots                                  */
  uint64_t n_cells;         /* DataSetConfig.nCells (power of two)                   */
  uint64_t n_samples;       /* DataSetConfig.nSamples                                */
  uint64_t seed;            /* DataSource FakeData seed (used when file_base == NULL) */
  const char* file_base;    /* DataSource SlotFile base name: slot k = "<base><k>.dat" (dataset.nim:34).  Cell i of a slot is
                             * bytes [i x cell_size, (i + 1) x cell_size) of its file; what lies past the end of the file reads as
                             * zeros (slot.nim:61-66).  A file that cannot be opened is CP2_ERR_IO with "cannot open <file>" in
                             * cp2_last_error; a read of it that fails (EIO, EISDIR, ...: anything but the end of the file; an
                             * interrupted read is retried) is CP2_ERR_IO with "cannot read <file>: <reason>", never zeros, and no
                             * tree, proof input or input.json comes back from that call.  Cells over 16384 bytes are refused:
                             * CP2_ERR_INVALID (slot.nim:60-61).  The same holds for cp2_slot_trees_build_file_units. */
} cp2_config;

/* A dataset whose slot trees are built: slot roots + dataset tree (gen_input/bn254.nim:41-51). */
typedef struct cp2_dataset cp2_dataset;
/* Builds the trees of slots [first_slot, first_slot + n_local) on this GPU.  For a single GPU pass
 * first_slot = 0, n_local = cfg->n_slots.  */
int cp2_dataset_build(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, cp2_dataset** out);
/* cp2_dataset_build with what it keeps of the slot trees (cp2_set_keep_trees: every node, the compact layers, or the roots) cached
 * in `cache_path`: read when present, intact and matching the configuration -- and, for the SlotFile source, slot files of
 * unchanged size and mtime --, else built and written (to a temporary name, then renamed) */
int cp2_dataset_build_cached(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local,
                             const char* cache_path, cp2_dataset** out);
void cp2_dataset_free(cp2_dataset* ds);
/* roots of the local slots (n_local x 32 bytes) */
int cp2_dataset_local_roots(cp2_dataset* ds, uint8_t* out);
/* Supply the roots of ALL n_slots slots (after the multi-GPU gather; single GPU: pass NULL to use the
 * local ones) and build the dataset-level tree on the GPU. */
int cp2_dataset_set_roots(cp2_dataset* ds, const uint8_t* all_roots);
/* The same exchange without host copies of the roots (the gather of SURVEY.md 8e is device to device: RCCL, a torch tensor):
 * cp2_dataset_local_roots_dev = device pointer to the n_local x 32 bytes of local roots (valid until the dataset is freed);
 * cp2_dataset_copy_local_roots_dev ENQUEUES a device-to-device copy of them into the caller's buffer on the context's stream
 * (cp2_sync before another stream reads it); cp2_dataset_set_roots_dev takes ALL n_slots roots in device memory (16-byte
 * aligned, any device of the node), builds the dataset tree from them and synchronises. */
const void* cp2_dataset_local_roots_dev(const cp2_dataset* ds);
int cp2_dataset_copy_local_roots_dev(cp2_dataset* ds, void* d_out);
int cp2_dataset_set_roots_dev(cp2_dataset* ds, const void* d_all_roots);
int cp2_dataset_root(cp2_dataset* ds, uint8_t out[32]);
int cp2_dataset_keeps_trees(const cp2_dataset* ds);
/* the slot range and the context a dataset was built with */
int cp2_dataset_range(const cp2_dataset* ds, uint64_t* first_slot, uint64_t* n_local);
cp2_ctx* cp2_dataset_ctx(const cp2_dataset* ds);

/* SlotProofInput, reference/nim/proof_input/src/types.nim:52-60 */
typedef struct cp2_proof_input cp2_proof_input;
/* replaces `generateProofInputBN254`, reference/nim/proof_input/src/gen_input/bn254.nim:35-79, for a
 * slot that is local to `ds`. */
int cp2_proof_input_generate(cp2_dataset* ds, uint64_t slot_idx, const uint8_t entropy[32], cp2_proof_input** out);
/* The same for n slots of `ds` at once (config 4: thousands of slots sharing one dataset tree): one
 * sampling launch, one path gather and one cell fetch for all of them.  out[0..n) receive the objects. */
int cp2_proof_inputs_generate_batch(cp2_dataset* ds, const uint64_t* slot_idx, size_t n, const uint8_t entropy[32],
                                    cp2_proof_input** out);
void cp2_proof_input_free(cp2_proof_input* p);
/* accessors (all field elements canonical 32-byte LE) */
int cp2_proof_input_roots(const cp2_proof_input* p, uint8_t dataset_root[32], uint8_t slot_root[32], uint8_t entropy[32]);
size_t cp2_proof_input_nsamples(const cp2_proof_input* p);
const uint64_t* cp2_proof_input_cell_indices(const cp2_proof_input* p);
const uint8_t* cp2_proof_input_cell_data(const cp2_proof_input* p);     /* nSamples x cellSize bytes      */
const uint8_t* cp2_proof_input_merkle_paths(const cp2_proof_input* p);  /* nSamples x maxDepth x 32 bytes */
const uint8_t* cp2_proof_input_slot_proof(const cp2_proof_input* p);    /* maxLog2NSlots x 32 bytes       */
/* hash of each sampled cell = `leafValue` of its merged proof (merkle.nim:86-100); nSamples x 32 bytes, or NULL for an
 * object made by cp2_proof_input_create without them */
const uint8_t* cp2_proof_input_leaf_hashes(const cp2_proof_input* p);
/* A proof input assembled from caller arrays -- what a `SlotProofInput[Hash]` value holds (types.nim:52-60) -- so that
 * `exportProofInputBN254(hashcfg, fname, prfInput)` (json/bn254.nim:77) can hand any such value to the byte-exact writer.
 * cfg supplies maxDepth, maxLog2NSlots, cellSize, nCells, nSlots; arrays as the accessors above return them; cell_indices
 * and leaf_hashes may be NULL (neither is printed).  Everything is copied; free with cp2_proof_input_free. */
int cp2_proof_input_create(const cp2_config* cfg, uint64_t slot_idx, const uint8_t dataset_root[32], const uint8_t entropy[32],
                           const uint8_t slot_root[32], const uint8_t* slot_proof, size_t n_samples, const uint64_t* cell_indices,
                           const uint8_t* cell_data, const uint8_t* merkle_paths, const uint8_t* leaf_hashes,
                           cp2_proof_input** out);
/* replaces `exportProofInputBN254`, reference/nim/proof_input/src/json/bn254.nim:57-78: byte-exact JSON */
int cp2_proof_input_write_json(const cp2_proof_input* p, const char* path);
/* the same text into a malloc'ed buffer (caller frees with cp2_free_buffer) */
int cp2_proof_input_json(const cp2_proof_input* p, char** text, size_t* len);
void cp2_free_buffer(void* p);
/* Serialise n proof inputs on `threads` host threads and write paths[i] (paths == NULL or paths[i] == NULL:
 * serialise only).  total_bytes (may be NULL) receives the summed text length. */
int cp2_proof_inputs_write_json_batch(const cp2_proof_input* const* ps, size_t n, const char* const* paths, int threads,
                                      uint64_t* total_bytes);
/* All of it for many slots as a two-stage pipeline (GPU: sampling + gathers of batch k+1; host threads: JSON of
 * batch k).  dir == NULL: serialise only; else "<dir>/input_<slot>.json" is written per slot.  batch == 0: 512. */
int cp2_dataset_export_proof_inputs(cp2_dataset* ds, const uint64_t* slot_idx, size_t n, const uint8_t entropy[32],
                                    const char* dir, int threads, size_t batch, uint64_t* total_bytes);
/* The whole of `generateProofInputBN254` + `exportProofInputBN254` for EVERY local slot with the entropy known up front
 * (reference/nim/proof_input/src/gen_input/bn254.nim:35-79, json/bn254.nim:57-78), as one overlapped pipeline: slot trees
 * are built `group_slots` at a time (0: what fills the 2 GiB staging chunk; the last groups shrink so that little formatting is
 * left un-overlapped; with the SlotFile source the slots are read in ring turns of many small files or pieces of large ones, and
 * the groups are what the layer passes and the sampling are done by), and while later slots are still hashing the
 * finished ones are sampled (sample/bn254.nim:16-27), their paths and cells gathered on the device, downloaded into pinned
 * memory and formatted (cellData + merklePaths) on `threads` host threads.  Only the lines that need all slot roots
 * (dataSetRoot, slotProof: gen_input/bn254.nim:49-51,72) are left for cp2_dataset_export_streamed.  The returned dataset
 * is a normal cp2_dataset (roots, set_roots, proof inputs for other entropies all work).
 * Host memory: the formatted bodies stay with the dataset until cp2_dataset_free, in memory up to the context's body budget
 * and in spill files beyond it (cp2_set_body_budget above). */
int cp2_dataset_build_streamed(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local,
                               const uint8_t entropy[32], int threads, size_t group_slots, cp2_dataset** out);
/* Finish what cp2_dataset_build_streamed prepared: needs the dataset tree (cp2_dataset_set_roots; implied when all slots
 * are local).  dir == NULL: format only; else "<dir>/input_<slot>.json" per local slot.  Text identical to
 * cp2_proof_input_json of the same slot and entropy. */
int cp2_dataset_export_streamed(cp2_dataset* ds, const char* dir, int threads, uint64_t* total_bytes);
/* the finished text of one prepared slot in a malloc'ed buffer (cp2_free_buffer) */
int cp2_dataset_streamed_json(cp2_dataset* ds, uint64_t slot_idx, char** text, size_t* len);
/* ---- proof inputs across datasets ----------------------------------------------------------------------------------------
 * generateProofInput (reference/nim/proof_input/src/gen_input/bn254.nim:35-79) takes a dataset, a slot and an entropy on every call
 * (generateProofInputBN254, :78).  These take n such requests at once: request i is (ds[i], slot_idx[i], entropies[32*i .. 32*i+32)).
 * A storage node holding one slot each of many datasets (cp2_dataset_build(_cached) with first_slot = k, n_local = 1, then
 * cp2_dataset_set_roots with the manifest's slot roots) proves all of them each period in one call.
 *   Same result   out[i] is the object cp2_proof_input_generate(ds[i], slot_idx[i], entropy i) returns, and its cp2_proof_input_json
 *                 text is byte-identical.  Entropies are reduced to their canonical residue as there.  A dataset may appear in many
 *                 requests, with the same or different slots and entropies.
 *   One circuit   every dataset belongs to ctx and has the same SampleAndProve template arguments (sample_cells.circom:58-148):
 *                 max_depth, max_log2_nslots, cell_size, block_size, n_samples (the rule of cp2_proof_inputs_verify).  n_cells,
 *                 n_slots, the source (seed or file_base) and what the dataset keeps of its trees may differ.
 *   Refusals      checked before any proof work on the device: CP2_ERR_INVALID, every out[i] NULL, and cp2_last_error names the
 *                 request index.  A request is refused when ds[i] is NULL; its dataset belongs to another context; its circuit
 *                 parameters differ from request 0's; its slot is not local to its dataset; its dataset has no dataset tree and not
 *                 all of its slots are local (cp2_dataset_set_roots was never called); nCells or a tree depth breaks an assert of
 *                 generateProofInput (sample/bn254.nim:19-20, types.nim:29); or the root the dataset tree holds for its slot (what
 *                 cp2_dataset_set_roots was given) differs from the slot's built root (that input.json would be rejected by the circuit).
 *   All or nothing  slot data that no longer hashes to what was built (a compact dataset's block-root check, a roots-only dataset's
 *                 rebuild check) and slot-file reads that fail are CP2_ERR_IO, naming the request, the block and the slot where they
 *                 apply, and no object comes back.  A context whose stream will not drain is refused (CP2_ERR_HIP).  n == 0: CP2_OK.
 * Datasets that keep every node or the compact layers are sampled and gathered in one pass for all requests (the compact ones in
 * chunks whose touched blocks fit the staging chunk, CODEX_P2_STAGE_MB); a roots-only dataset costs one slot rebuild per request.
 * Datasets of a cp2_multi_dataset belong to the multi-device object's own contexts. */
int cp2_proof_inputs_generate_many(cp2_ctx* ctx, cp2_dataset* const* ds, const uint64_t* slot_idx, const uint8_t* entropies /* n x 32 */,
                                   size_t n, cp2_proof_input** out);
/* The same, serialised on `threads` host threads and written to paths[i] (paths == NULL or paths[i] == NULL: serialise only), as a
 * two-stage pipeline like cp2_dataset_export_proof_inputs (device work of chunk k+1 while chunk k is formatted); batch == 0: 512
 * requests per chunk.  Every request is checked before the first chunk.  total_bytes (may be NULL) receives the summed text length. */
int cp2_proof_inputs_export_many(cp2_ctx* ctx, cp2_dataset* const* ds, const uint64_t* slot_idx, const uint8_t* entropies, size_t n,
                                 const char* const* paths, int threads, size_t batch, uint64_t* total_bytes);
/* ---- verification: what SampleAndProve accepts (circuit/codex/sample_cells.circom:58-148) ----------------------------------
 * The verifier accepts exactly the inputs for which SampleAndProve(maxDepth, maxLog2NSlots, blockTreeDepth, nFieldElemsPerCell,
 * nSamples) has a satisfying witness, reading them as the field elements the circuit sees:
 *   top      RootFromMerklePath(maxLog2NSlots) of slotRoot with path bits = slotIndex, last bits = nSlotsPerDataSet - 1,
 *            mask = CeilingLog2(nSlotsPerDataSet).mask, path = slotProof, must give dataSetRoot (sample_cells.circom:95-109);
 *   sample   counter cnt + 1: idx = lowbits(Poseidon2_hash_rate2([entropy, slotRoot, cnt + 1])) & (nCellsPerSlot - 1)
 *            (:23-48), leaf = Poseidon2_hash_rate2(cellData[cnt]), then the bottom RootFromMerklePath(blockTreeDepth) and the
 *            middle RootFromMerklePath(maxDepth - blockTreeDepth) over merklePaths[cnt], both with last bits = mask bits =
 *            Log2(nCellsPerSlot).mask (:117-123), must give slotRoot (single_cell.circom:30-73);
 *   RootFromMerklePath exactly as merkle.circom:44-114 (maskBitsCorrected[0] = 1, isLast from the top down, key = bottom + 2*odd,
 *            the root is the layer the mask selects): a path entry above the selected layer is ignored, whatever its value.
 * blockSize / cellSize must be a power of two >= 2 (the circuit has no blockTreeDepth 0): else CP2_ERR_INVALID. */
#define CP2_VERIFY_DATASET_ROOT 1u   /* slotRoot + slotProof do not give dataSetRoot (sample_cells.circom:95-109)            */
#define CP2_VERIFY_SAMPLE       2u   /* some sample's cell + path do not give slotRoot (single_cell.circom:63-71)            */
#define CP2_VERIFY_SHAPE        4u   /* a witness-generation assertion fails: nCellsPerSlot not 2^k with 1 <= k <= maxDepth
                                        (lib/log2.circom Log2_CircomWitnessCalc_Hack), nSlotsPerDataSet not in
                                        [1, 2^maxLog2NSlots] (CeilingLog2), slotIndex >= 2^maxLog2NSlots (misc.circom ToBits) */
/* input.json text (any JSON whitespace and key order; numbers as quoted decimal strings or bare integers) -> a proof input.
 * cfg supplies the circuit parameters maxDepth, maxLog2NSlots, cellSize, blockSize and nSamples (0: as many rows as the text
 * has); the text supplies the rest.  nCellsPerSlot, nSlotsPerDataSet and slotIndex are kept as read, shape failures included.
 * Refused (CP2_ERR_INVALID, the key / row / column named in msg, which may be NULL): missing, unknown or repeated keys, wrong
 * array lengths, a field element >= r, nCellsPerSlot / nSlotsPerDataSet / slotIndex >= 2^64, a sign, a non-digit, trailing text.
 * The object holds the cells as field elements: cp2_proof_input_cell_data returns the bytes when every row is the 10*-padded
 * encoding of cellSize bytes, else NULL; cell_indices and leaf_hashes are NULL; cp2_proof_input_json prints the field
 * elements it holds (a producer's text comes back byte for byte).  Free with cp2_proof_input_free. */
int cp2_proof_input_parse_json(const cp2_config* cfg, const char* text, size_t len, cp2_proof_input** out, char* msg, size_t msg_len);
/* nCellsPerSlot, nSlotsPerDataSet and slotIndex as the object holds them (a parsed object: as the text states them) */
int cp2_proof_input_shape(const cp2_proof_input* p, uint64_t* n_cells, uint64_t* n_slots, uint64_t* slot_idx);
/* the sampled cells as the circuit sees them: nSamples x cp2_felts_per_bytes(cellSize) x 32 bytes (canonical LE) */
int cp2_proof_input_cell_felts(const cp2_proof_input* p, uint8_t* out);
/* status[i] = 0 (accepted) or CP2_VERIFY_* bits; sample_ok (may be NULL): n x nSamples bytes, 1 where that sample's equation
 * holds.  All objects must share the circuit parameters (maxDepth, maxLog2NSlots, cellSize, blockSize, nSamples).
 * CP2_VERIFY_SHAPE is reported alone, with every sample_ok byte 0.  One GPU launch per chunk of inputs (device memory bounded
 * whatever n is); synchronous. */
int cp2_proof_inputs_verify(cp2_ctx* ctx, const cp2_proof_input* const* ps, size_t n, uint32_t* status, uint8_t* sample_ok);

/* ---- scrub: the stored slot data against what the dataset keeps ----------------------------------------------------------
 * cp2_dataset_build_cached trusts a slot file of unchanged size and mtime, and a compact proof input reads only the blocks its samples
 * touch: bytes that changed underneath (bit rot, a bad sector, a partial restore) surface as CP2_ERR_IO when a challenge lands on them.
 * A scrub reads the selected slots again from the dataset's source (slot files, or the fake source: regenerated, always clean), hashes
 * them in the context's build scratch as the compact / roots-only builds do (the same ingestion settings: cp2_set_ingest, O_DIRECT,
 * mapped) and compares, on the device, at the finest level the dataset keeps:
 *   CP2_SCRUB_CELL   every node kept (and every unit build of a cp2_multi_dataset): index = the cell of the slot whose hash differs;
 *   CP2_SCRUB_BLOCK  compact: index = the network block of the slot whose root differs -- the unit a storage node repairs;
 *   CP2_SCRUB_SLOT   roots only: index = 0, the slot root differs.
 *   Slots    first_slot .. first_slot + n_slots - 1, dataset slot numbers inside the local range; n_slots == 0: every local slot
 *            (first_slot is not read).  Outside the range: CP2_ERR_INVALID.
 *   Result   *n_bad = the number of mismatches; bad (cap x 2 uint64: slot, index) receives the lowest min(cap, *n_bad) of them in
 *            (slot, index) order; cap == 0 with bad == NULL only counts; *granularity = CP2_SCRUB_* (granularity may be NULL).
 *            Changed data is not an error: CP2_OK with *n_bad > 0.  A file now shorter reads as zeros past its end (slot.nim:61-66),
 *            so its changed tail blocks are reported.  A file that cannot be opened or read is CP2_ERR_IO with the builders' messages
 *            (cp2_config), and nothing is written to the outputs; neither on any other error.  A context whose stream will not drain
 *            is refused (CP2_ERR_HIP).
 *   Read-only  the kept nodes, the dataset tree, the mode and any cache file stay as they are: every proof input and input.json is
 *            byte-identical before and after a scrub.  CP2_TRACE prints one line per scrub (slots, bytes, seconds, mismatches). */
#define CP2_SCRUB_SLOT  0
#define CP2_SCRUB_BLOCK 1
#define CP2_SCRUB_CELL  2
int cp2_dataset_scrub(cp2_dataset* ds, uint64_t first_slot, uint64_t n_slots, uint64_t* bad /* cap x 2: (slot, index) */, size_t cap,
                      size_t* n_bad, int* granularity);
/* Every local slot of n datasets of one context in ONE pass -- the storage node of cp2_proof_inputs_generate_many above, which holds
 * one slot each of many datasets (first_slot = k, n_local = 1): scrubbed one by one, every dataset pays a whole pipe (rings and events
 * set up and torn down, one small hash launch, a drain), whatever its size.  Request i scrubs every local slot of ds[i]: what
 * cp2_dataset_scrub(ds[i], 0, 0, ...) does, at the finest level that dataset keeps.
 *   Same result  the triples of request i are exactly the (slot, index) pairs the single call reports for ds[i], with i in front.  bad
 *            (cap x 3 uint64: request, slot, index) receives the lowest min(cap, *n_bad) triples in (request, slot, index) order;
 *            *n_bad counts all mismatches; counts (n entries, may be NULL) receives the mismatches of each request, complete even when
 *            the report is capped (which datasets are damaged is never lost); granularity (n entries, may be NULL) the CP2_SCRUB_* level
 *            of each request.  cap == 0 with bad == NULL only counts.
 *   Datasets may differ in n_cells, n_slots, first_slot, n_local, source, base name, seed and in what they keep.  A dataset may appear
 *            twice: each request gets its own report.
 *   Refused  before any device or file work, outputs untouched, the request index in cp2_last_error (CP2_ERR_INVALID): ctx or n_bad
 *            NULL; ds NULL with n > 0; cap > 0 with bad NULL; ds[i] NULL; ds[i] not a dataset of ctx (the shards of a cp2_multi_dataset
 *            belong to that object's contexts).  n == 0: CP2_OK, *n_bad = 0.  A context whose stream will not drain: CP2_ERR_HIP.
 *   Errors   a slot file that cannot be opened or read is CP2_ERR_IO with the builders' message naming the file, and nothing is written
 *            to any output; neither on any other error.  Changed data is not an error.  Read-only, as a scrub is.
 *   How      the requests are grouped into classes of equal (cell_size, block_size, n_cells, level, source kind).  The slots of a
 *            file-sourced class are one run of items through the scrub's batch loop -- the same turns, batches and ingestion settings
 *            (cp2_set_ingest, O_DIRECT) as one dataset holding those slots -- read through a table of file names and compared through
 *            a table of the addresses of their kept layers.  The mapped ingestion mode keys its mappings by dataset unit: a listed
 *            batch does not use it and always goes through the pinned ring.  Fake-source requests are regenerated (always clean) one
 *            by one inside the call, as cp2_dataset_scrub does.  Datasets that each have a geometry of their own make every class one
 *            dataset, which is the loop over cp2_dataset_scrub: accepted.  Each class keeps at most cap triples; the classes are merged
 *            by (request, slot, index) and truncated at the end.  CP2_TRACE prints one line for the whole call (requests, classes,
 *            items, batches, bytes, seconds, GB/s, mismatches; items and bytes count the slot files read, not the fake-source requests).
 *            A batch holds half a staging chunk (CODEX_P2_STAGE_MB) of nodes, 129 slots of 64 cells at its minimum of 1 MiB: with fewer
 *            small slots than that, several batches can only be had by listing datasets more than once. */
int cp2_datasets_scrub_many(cp2_ctx* ctx, cp2_dataset* const* ds, size_t n, uint64_t* bad /* cap x 3: (request, slot, index) */, size_t cap,
                            size_t* n_bad, uint64_t* counts /* n, may be NULL */, int* granularity /* n, may be NULL */);

/* ---- build many: n datasets of one context built in ONE pass ---------------------------------------------------------------------
 * The same storage node after a restart without a cache, or after a batch of finished downloads: thousands of one-slot datasets to
 * build.  One by one through cp2_dataset_build every dataset pays a whole pipe and a drain of the device whatever its size -- 4096
 * datasets of 8 MiB: 23.3 s, against 0.87 s for the same files as the slots of one dataset (profiles/scrub_many_rate.txt).
 *   Requests request i is (cfgs[i], first_slot = ranges[2 i], n_local = ranges[2 i + 1]): what cp2_dataset_build takes.  Requests may
 *            differ in everything cp2_dataset_build accepts (geometry, n_slots, slot range, source, base name, seed); the same request
 *            may repeat, the repeats are independent datasets.
 *   Work     file-sourced requests are grouped into classes of equal (cell_size, block_size, n_cells); the slots of a class are one run
 *            of items -- a request of n_local slots is n_local consecutive items -- through the compact build's batch loop: the same
 *            turns, batches (half a staging chunk of nodes) and ingestion settings (cp2_set_ingest, O_DIRECT) as one dataset holding
 *            those slots, read through a table of file names; what each dataset keeps of a finished batch is written through a table
 *            of addresses, one launch per kept layer (the mirror image of cp2_datasets_scrub_many's compare).  The mapped ingestion mode
 *            is not used, as there.  Fake-source requests are built one by one inside the call.  What is kept (cp2_set_keep_trees /
 *            CODEX_P2_KEEP_TREES) is decided ONCE for the call: a named mode holds for every request; the automatic choice takes the
 *            most that fits for the sum of the requests, and steps down and starts over when an allocation fails after all.
 *   Result   out[i] is, in every observable, what cp2_dataset_build(ctx, &cfgs[i], first_slot, n_local, ...) returns under the same kept
 *            mode: an ordinary dataset for cp2_dataset_set_roots, proof inputs (cp2_proof_inputs_generate_many included), scrub,
 *            repair, block proofs, read-back and cp2_dataset_free, in any order and for any subset.  What the datasets keep are slices
 *            of device allocations shared by neighbouring requests (about 64 MiB each): an allocation is returned when the last
 *            dataset with a slice of it is freed.
 *   Refused  before any device or file work (CP2_ERR_INVALID, "request i: ..." in cp2_last_error where a request is at fault): ctx or
 *            out NULL; cfgs or ranges NULL with n > 0; a request cp2_dataset_build refuses (slots outside the dataset, n_local == 0,
 *            negative depths, a geometry that does not divide, slot-file cells over 16384 bytes).  n == 0: CP2_OK.  A context whose
 *            stream will not drain: CP2_ERR_HIP.
 *   Errors   a slot file that cannot be opened or read is CP2_ERR_IO with the builders' message naming the file (cp2_config).  On
 *            every return other than CP2_OK with out not NULL, all out[0 .. n) are NULL and nothing of the call stays allocated.
 *            CP2_TRACE prints one line for the whole call (requests, fake-source requests, classes, items, batches, bytes, seconds,
 *            GB/s, mode; items and bytes count the slot files read). */
int cp2_datasets_build_many(cp2_ctx* ctx, const cp2_config* cfgs /* n structs */, const uint64_t* ranges /* n x 2: first_slot, n_local */,
                            size_t n, cp2_dataset** out /* n */);

/* ---- set roots many: the dataset trees of n datasets of one context in ONE pass ------------------------------------------------------
 * Between "built" and "can prove" every dataset needs the slot roots of its manifest, so that its dataset tree and slotProof exist.  One by
 * one through cp2_dataset_set_roots every dataset pays a launch per tree level and a drain of the device: 4096 datasets of 4096 slots,
 * 5.87 s after a build of 0.82 s (profiles/build_many_rate.txt).
 *   Requests request i is (ds[i], all_roots[i]): what cp2_dataset_set_roots takes, all_roots[i] holding n_slots(ds[i]) x 32 bytes.
 *            all_roots == NULL or all_roots[i] == NULL: the local roots of ds[i] are all of them.
 *   Result   after CP2_OK dataset i is, in every observable, what cp2_dataset_set_roots(ds[i], all_roots[i]) leaves behind: cp2_dataset_root,
 *            slotProof and the head lines of every proof input and input.json, cp2_dataset_export_streamed of a streamed build,
 *            cp2_proof_inputs_generate_many.  A dataset that already had a tree gets the new one.
 *   own      own[i] (own may be NULL) is 1 when rows [first_slot, first_slot + n_local) of the roots given for request i equal the roots
 *            ds[i] built, else 0; always 1 where no roots were given.  Compared on the device in the same pass.  A difference is no error
 *            -- cp2_dataset_set_roots accepts any roots, and cp2_proof_inputs_generate_many refuses such a request later --: the node
 *            learns at set time that its slot does not match the manifest.
 *   Refused  before any device work (CP2_ERR_INVALID, "request i: ..." in cp2_last_error where a request is at fault): ctx NULL; ds NULL
 *            with n > 0; a NULL dataset; a dataset of another context; the same dataset twice; NULL roots for a dataset whose slots are
 *            not all local.  n == 0: CP2_OK.  A context whose stream will not drain: CP2_ERR_HIP.
 *   Errors   on every return other than CP2_OK no dataset of the call has changed (the trees wait in host staging until all are there) and
 *            own is not written.
 *   How      the requests go in chunks whose trees (the sum of cp2_merkle_total(n_slots) x 32 bytes) fit half the context's staging
 *            (CODEX_P2_STAGE_MB); a request larger than that runs alone.  Per chunk: one upload of the tables and the given roots, a
 *            device-to-device copy per tree that puts its leaves in place, one launch per tree level for all trees of the chunk whatever
 *            their sizes, one download.  CP2_TRACE prints one line for the whole call (requests, chunks, tree rows, levels, and the
 *            seconds of upload, levels, download and commit). */
int cp2_datasets_set_roots_many(cp2_ctx* ctx, cp2_dataset* const* ds, const uint8_t* const* all_roots /* n pointers, may be NULL */, size_t n,
                                uint8_t* own /* n, may be NULL */);

/* ---- repair: replacement blocks checked against the kept block roots, then written back ----------------------------------------
 * A scrub names the network blocks whose data no longer hashes to what the dataset keeps; the node fetches or re-decodes them (erasure
 * decoding is the caller's) and hands the candidates in here.  Each candidate is checked ALONE, on the device, against the block root the
 * dataset keeps for that block (every node kept: the block-tree root layer; compact: layer 0 of the compact layers): its cells are hashed
 * and reduced to a block root exactly as the builders do, one verdict per request.  Only candidates that match are written.
 *   Requests   slot_block (n x 2 uint64: dataset slot inside the local range, block of the slot < nBlocks), data (n x blockSize bytes,
 *              request i at i x blockSize).  Pageable or large buffers go through the context's pinned ring in chunks, upload and
 *              hashing overlapped; caller-pinned buffers (hipHostMalloc / hipHostRegister) are read in place.  A batch larger than half
 *              the context's staging (CODEX_P2_STAGE_MB) runs in several chunks.
 *   Refused    before any device or file work, CP2_ERR_INVALID with the request index (where there is one) in cp2_last_error: a NULL
 *              handle; NULL slot_block, data or status when n > 0; a slot outside the local range; a block >= nBlocks; the same (slot,
 *              block) twice; an unknown flag; a roots-only dataset (it keeps no block roots: write the slot whole, then rebuild or
 *              scrub it); a fake-source dataset without CP2_REPAIR_CHECK_ONLY (it has no files).  A refused call leaves status,
 *              *n_written, the files and the cache untouched.  n == 0: CP2_OK.  A context whose stream will not drain is refused
 *              (CP2_ERR_HIP).
 *   Result     status[i] = CP2_REPAIR_MATCH (hashes to the kept block root; written unless CP2_REPAIR_CHECK_ONLY), _MISMATCH (differs;
 *              never written) or _UNWRITTEN (matched, but its file could not be written or synced); *n_written = the blocks written
 *              and synced (n_written may be NULL).  A wrong candidate is not an error: CP2_OK.
 *   Write      each matching block with pwrite to "<base><slot>.dat" at block x blockSize, grouped by file in ascending offset order,
 *              every file fdatasync'ed once after its last write.  A missing file is created (mode 0644 before umask); a write past
 *              the end extends the file, and a hole left before it reads as zeros, which the next scrub reports.  The first file that
 *              cannot be opened, written or synced stops the writing: CP2_ERR_IO, "cannot write <file>: <reason>"; the blocks of
 *              earlier files stay written (and counted), the matched blocks of that file and of every later one are _UNWRITTEN.  A
 *              write is not atomic: a block torn by a crash shows up in the next scrub.
 *   Cache      cache_path (may be NULL): after every write and sync, the (size, mtime) stamps in whichever of <cache_path> and
 *              <cache_path>.kept describe this dataset (magic, geometry, source, first slot, base name) are set, in place (pwrite +
 *              fdatasync), for the files this call wrote -- only where the stamp equalled that file's stat before the call's first
 *              write: when the damage itself changed the mtime the cache was stale and stays stale.  The next
 *              cp2_dataset_build_cached then loads the cache instead of rebuilding.  Stamps lie outside the node checksum: a torn
 *              restamp costs a rebuild, nothing more.
 *   Unchanged  the kept nodes, the dataset tree, the mode and the bodies of a streamed build: the proof inputs and input.json files of
 *              clean slots stay byte-identical, and one that failed with CP2_ERR_IO on a damaged block is, after a matching repair,
 *              the one from before the damage.  CP2_TRACE prints one line per call (requests, matched, written, bytes, seconds,
 *              whether the cache was restamped). */
#define CP2_REPAIR_CHECK_ONLY 1      /* flag: verdicts only, nothing written */
#define CP2_REPAIR_MATCH      0      /* status: hashes to the kept block root; written unless CHECK_ONLY */
#define CP2_REPAIR_MISMATCH   1      /* status: differs from the kept block root; not written */
#define CP2_REPAIR_UNWRITTEN  2      /* status: matched, but its file could not be written or synced (call returns CP2_ERR_IO) */
int cp2_dataset_repair_blocks(cp2_dataset* ds, const uint64_t* slot_block /* n x 2: dataset slot, block of the slot */,
                              const uint8_t* data /* n x block_size */, size_t n, int flags, const char* cache_path,
                              uint32_t* status /* n */, size_t* n_written);

/* ---- block proofs: network blocks proved and checked against slot roots with Merkle paths ----------------------------------------
 * Scrub and repair rest on the block roots a dataset keeps.  A node that receives blocks of a slot it has no tree for knows only the slot
 * root (from the manifest); what a peer can send with a 64 KiB block is the block's Merkle path to that root.  The proof of block b of a
 * slot of nBlocks = nCells / (blockSize / cellSize) blocks is merkleProof(bigTree, b) (reference/nim/proof_input/src/merkle.nim:21-42):
 * leaf = the block root (the root of the block tree over the block's cell hashes), numberOfLeaves = nBlocks, path = one sibling per
 * layer of the tree over the slot's block roots, bottom first, ZERO where the sibling is out of range (an odd layer's last node, the
 * singleton).  Its length is cp2_block_proof_depth = cp2_merkle_num_layers(nBlocks) - 1: ceil(log2(nBlocks)), and 1 for nBlocks == 1.
 * It is never padded to maxDepth: this proof is not circuit input.  Checking is reconstructRoot (merkle.nim:51-74): on level i with
 * running index j and layer size m, j odd -> compress(sibling, h, key); j == m - 1 (even, last) -> compress(h, sibling, key + 2); else
 * compress(h, sibling, key); key = 1 on level 0, else 0; then j >>= 1, m = (m + 1) >> 1.  Siblings and roots are 32-byte little-endian
 * field elements, inputs >= r taken mod r.
 *
 * cp2_block_proof_depth: host only; 0 for a geometry the tree builders refuse (a zero size, a block that is not whole cells, nCells that
 * is not whole blocks, the size caps).
 *
 * cp2_dataset_block_proofs serves proofs from what a dataset keeps: every node, or the compact layers (which ARE that tree).
 *   Requests   slot_block (n x 2 uint64: dataset slot inside the local range, block of the slot < nBlocks); the same pair may repeat.
 *   Result     block_roots (n x 32 bytes, may be NULL) and paths (n x depth x 32 bytes, request i at i x depth x 32, bottom first).  One
 *              upload of the row list, one gather on the device, one download.
 *   Refused    CP2_ERR_INVALID, the request index (where there is one) in cp2_last_error, outputs untouched: a NULL handle; NULL
 *              slot_block or paths when n > 0; a slot outside the local range; a block >= nBlocks; a roots-only dataset (it keeps
 *              only its slot roots: no layers to take a path from).  n == 0: CP2_OK.  A context whose stream will not drain is refused
 *              (CP2_ERR_HIP).  The unit builds inside a cp2_multi_dataset are not served (a shard by slots is a plain cp2_dataset).
 *   Read-only  nothing of the dataset changes.
 *
 * cp2_blocks_verify checks n candidate blocks, each with its path, against slot roots the caller states: no dataset, no tree.
 *   Requests   slot_roots (n_roots x 32 bytes); root_block (n x 2 uint64: index into slot_roots, block of the slot); data (n x blockSize
 *              bytes); paths (n x depth x 32 bytes).  nBlocks need not be a power of two.  The same (root, block) twice is allowed (two
 *              peers may send the same block): each gets its own verdict.  The data path is repair's: chunks of half the context's
 *              staging (CODEX_P2_STAGE_MB), caller-pinned buffers read in place, large pageable chunks through the pinned ring; each
 *              chunk's paths are uploaded with the chunk, the slot roots once.  Every candidate's cells are hashed and reduced to its
 *              block root exactly as the builders do, then walked up its path on the device.
 *   Refused    before any device work, CP2_ERR_INVALID, outputs untouched: a NULL context; a geometry the tree builders refuse; a NULL
 *              array (block_roots excepted) when n > 0; a root index >= n_roots or a block >= nBlocks, with the request index in
 *              cp2_last_error.  n == 0: CP2_OK.  A context whose stream will not drain is refused (CP2_ERR_HIP).
 *   Result     status[i] = CP2_BLOCK_MATCH (the candidate and its path reconstruct slot_roots[root]) or CP2_BLOCK_MISMATCH; block_roots
 *              (n x 32 bytes, may be NULL) = what each candidate hashed to.  A wrong block or a wrong path is not an error: CP2_OK.
 *              CP2_TRACE prints one line per call (requests, matched, bytes, seconds, GB/s).
 *
 * cp2_dataset_repair_blocks_proved is cp2_dataset_repair_blocks with a path beside every candidate, in EVERY residency mode: the
 * verdicts come from the path check against the dataset's own slot roots (cp2_dataset_local_roots), also when block roots are kept, so
 * the call means the same for a dataset that keeps every node, the compact layers or only its roots.
 *   Requests   as cp2_dataset_repair_blocks, plus paths (n x depth x 32 bytes).
 *   Refused    as there, without the roots-only refusal and with NULL paths when n > 0 (the same (slot, block) twice stays refused: two
 *              writes to one offset; a fake-source dataset takes CP2_REPAIR_CHECK_ONLY only).
 *   Result, Write, Cache, Unchanged   as cp2_dataset_repair_blocks; status values are CP2_REPAIR_*.  A roots-only dataset's next scrub of
 *              a repaired slot is clean, and its proof inputs are those from before the damage. */
#define CP2_BLOCK_MATCH    0         /* status: the candidate and its path reconstruct the stated slot root */
#define CP2_BLOCK_MISMATCH 1         /* status: they do not */
size_t cp2_block_proof_depth(size_t cell_size, size_t block_size, size_t n_cells);
int cp2_dataset_block_proofs(cp2_dataset* ds, const uint64_t* slot_block /* n x 2: dataset slot, block of the slot */, size_t n,
                             uint8_t* block_roots /* n x 32, may be NULL */, uint8_t* paths /* n x depth x 32 */);
int cp2_blocks_verify(cp2_ctx* ctx, size_t cell_size, size_t block_size, size_t n_cells, const uint8_t* slot_roots /* n_roots x 32 */,
                      size_t n_roots, const uint64_t* root_block /* n x 2: index into slot_roots, block of the slot */,
                      const uint8_t* data /* n x block_size */, const uint8_t* paths /* n x depth x 32 */, size_t n,
                      uint32_t* status /* n */, uint8_t* block_roots /* n x 32, may be NULL */);
int cp2_dataset_repair_blocks_proved(cp2_dataset* ds, const uint64_t* slot_block /* n x 2: dataset slot, block of the slot */,
                                     const uint8_t* data /* n x block_size */, const uint8_t* paths /* n x depth x 32 */, size_t n,
                                     int flags, const char* cache_path, uint32_t* status /* n */, size_t* n_written);

/* ---- verified read-back: listed blocks read from disk, checked against the kept block roots, returned with their proofs ---------------
 * cp2_dataset_block_proofs hands out a block's root and path but none of its bytes; a node that answers a peer would read the 64 KiB
 * itself and ship them unchecked, under a good proof, whatever happened to the sector since the last scrub.  cp2_datasets_read_blocks
 * reads the listed blocks, hashes each to its block root on the device, compares it with the root the dataset keeps, and returns bytes,
 * root and path together -- for the blocks of many datasets in one pass, which is also the spot scrub a node can afford every period
 * (a few random blocks of every slot it holds).  cp2_dataset_read_blocks is the same pass with one dataset, on that dataset's context.
 *   Requests   req (n x 3 uint64: index into ds, dataset slot inside that dataset's local range, block of the slot < its nBlocks), in any
 *              order; the same triple may repeat (two peers may ask for the same block), each repeat with its own row and verdict; a
 *              dataset may be listed twice in ds.  The datasets all belong to ctx and share cell_size and block_size; they may differ
 *              in n_cells, n_slots, local range, source, base name, seed and residency (every node kept, or compact).
 *   Data       row i of data (n x blockSize) = the blockSize bytes of request i, read from "<file_base><slot>.dat" at block x blockSize
 *              under the builders' read rule: what lies past the end of the file reads as zeros (a truncated file's tail blocks come
 *              back DAMAGED, as a scrub reports them), a read that fails is an error.  Reads are buffered preads, spread over the
 *              context's ingestion threads (cp2_set_ingest), one chunk ahead of the device; O_DIRECT and the mapped mode are not used.
 *              Each block is read once, into its row, and uploaded from there: the bytes hashed are the bytes returned.  The data path
 *              is repair's: chunks of half the context's staging, a caller-pinned data read in place by the copy engines, a pageable
 *              one through the pinned ring.  After the verdicts every DAMAGED row is overwritten with zeros.  Fake-source datasets
 *              regenerate their blocks on the device and download them; they are always OK.
 *   Check only With CP2_READ_CHECK_ONLY data may be NULL: the blocks pass through two pooled pinned chunk buffers, so memory is bounded
 *              by the chunk whatever n is.  A non-NULL data with the flag is still filled.
 *   Proofs     block_roots[i] (n x 32, may be NULL) and the path of request i are what cp2_dataset_block_proofs returns for it: the
 *              KEPT nodes, authentic whatever the disk holds, so they are returned for DAMAGED requests too (the node then knows what to
 *              ask a peer for, and hands the answer to cp2_dataset_repair_blocks).  Many-dataset form: depths differ with n_cells, so
 *              paths are packed -- request i's path is rows [path_off[i], path_off[i + 1]) of paths (32 bytes a row, bottom first), as
 *              many as the cp2_block_proof_depth of its dataset; path_off has n + 1 entries.  The caller sizes paths as the sum of those
 *              depths over the requests, computed from each dataset's configuration.  paths and path_off are given together or not at
 *              all.  Single form: paths is n x depth x 32, cp2_dataset_block_proofs' layout, and may be NULL.
 *   Result     status[i] = CP2_READ_OK or CP2_READ_DAMAGED; *n_ok (may be NULL) counts the former.  DAMAGED is not an error: CP2_OK.
 *   Refused    before any device or file work, CP2_ERR_INVALID, every output untouched, the dataset or request index in
 *              cp2_last_error: a NULL ctx (handle); with n > 0 a NULL ds, req or status; NULL data without CP2_READ_CHECK_ONLY; paths
 *              without path_off or the reverse; an unknown flag; ds[k] NULL, of another context, of another cell_size or block_size than
 *              ds[0], roots-only, or with kept layers that are not those of whole slot trees (the unit builds); a dataset index >=
 *              n_ds; a slot outside the local range; a block >= nBlocks of its dataset.  n == 0: CP2_OK, *n_ok = 0.  A context whose
 *              stream will not drain is refused (CP2_ERR_HIP).
 *   Errors     a slot file that cannot be opened or read: CP2_ERR_IO, cp2_last_error "cannot open <file>" / "cannot read <file>:
 *              <reason>".  status, *n_ok, block_roots, paths and path_off are untouched; data, if given, holds zeros in every row the
 *              call had written.
 *   Read-only  kept nodes, dataset tree, residency, cache files and slot files stay as they are; every proof input is the same before
 *              and after.  CP2_TRACE prints one line per call (datasets, requests, chunks, bytes, seconds, GB/s, damaged). */
#define CP2_READ_CHECK_ONLY 1        /* flag: verdicts, roots and paths only; data may be NULL */
#define CP2_READ_OK       0          /* status: the bytes on disk hash to the kept block root; returned */
#define CP2_READ_DAMAGED  1          /* status: they do not; the request's data row is all zeros */
int cp2_datasets_read_blocks(cp2_ctx* ctx, cp2_dataset* const* ds, size_t n_ds,
                             const uint64_t* req /* n x 3: index into ds, dataset slot, block of the slot */, size_t n, int flags,
                             uint8_t* data /* n x blockSize; may be NULL with CP2_READ_CHECK_ONLY */,
                             uint8_t* block_roots /* n x 32, may be NULL */,
                             uint8_t* paths /* packed, may be NULL */, uint64_t* path_off /* n + 1 rows, may be NULL iff paths is */,
                             uint32_t* status /* n */, size_t* n_ok /* may be NULL */);
int cp2_dataset_read_blocks(cp2_dataset* ds, const uint64_t* slot_block /* n x 2: dataset slot, block of the slot */, size_t n, int flags,
                            uint8_t* data, uint8_t* block_roots, uint8_t* paths /* n x depth x 32, may be NULL */,
                            uint32_t* status /* n */, size_t* n_ok);

/* ---- repair many: replacement blocks of many datasets judged in ONE pass and written back on many threads ------------------------------
 * After cp2_datasets_scrub_many or cp2_datasets_read_blocks has named the damaged blocks of many datasets, cp2_dataset_repair_blocks and
 * cp2_dataset_repair_blocks_proved take the replacements one dataset per call: a pass set-up, a drain and serial file writes for a few
 * blocks each.  cp2_datasets_repair_blocks_many takes the interleaved candidates of all datasets of one context in one pass.
 *   Datasets   cp2_datasets_read_blocks' rule: all belong to ctx and share cell_size and block_size; they may differ in n_cells, n_slots,
 *              local range, source, base name and residency -- every node kept, compact, or roots only.  A handle may be listed twice.
 *   Requests   req (n x 3 uint64: index into ds, dataset slot inside that dataset's local range, block of the slot < its nBlocks), data
 *              (n x blockSize bytes, request i at i x blockSize; the data path is cp2_dataset_repair_blocks').  Request i's path is rows
 *              [path_off[i], path_off[i + 1]) of paths (32 bytes a row, bottom first): cp2_datasets_read_blocks' packing, so what that
 *              call returns for a DAMAGED block goes straight back in.  An EMPTY path means "judge against the kept block root"
 *              (cp2_dataset_repair_blocks' rule); a path of exactly the cp2_block_proof_depth of its dataset means "walk to this
 *              dataset's own slot root" (cp2_dataset_repair_blocks_proved's rule), the only form a roots-only dataset accepts.  paths ==
 *              NULL (then path_off == NULL too): every path is empty.  One launch judges both kinds.
 *   Meaning    for any dataset k, the requests that name it get, in request order, the statuses the matching single call gives that
 *              dataset (CP2_REPAIR_MATCH / _MISMATCH / _UNWRITTEN), and where no write fails the slot-file bytes, the cache stamps and
 *              its share of *n_written are that call's too.  Unchanged: as documented for the single calls.
 *   Refused    before any device or file work, CP2_ERR_INVALID, every output, file and cache untouched, the lowest offending dataset or
 *              request index in cp2_last_error; arguments are checked first, then datasets, then requests: a NULL ctx; an unknown flag;
 *              paths without path_off or the reverse; with n > 0 a NULL ds, req, data or status; path_off[0] != 0; ds[k] NULL, of another
 *              context, of another cell_size or block_size than ds[0]; a dataset index >= n_ds; a decreasing path_off; a path length that
 *              is neither 0 nor its dataset's depth; an empty path for a roots-only dataset or for one whose kept layers are not those of
 *              whole slot trees; a slot outside the local range; a block >= nBlocks of its dataset; a request that names a fake-source
 *              dataset without CP2_REPAIR_CHECK_ONLY; the same (slot file, block) twice, whether through one handle listed twice or two
 *              handles over the same base name (fake-source datasets: the same (handle, slot, block)).  n == 0: CP2_OK, *n_written = 0.
 *              A context whose stream will not drain is refused (CP2_ERR_HIP).
 *   Write      the matched blocks are grouped by slot file (by NAME: two handles over one base name share their files), each file's
 *              blocks written in ascending offset order and the file fdatasync'ed once; the files are spread over the context's
 *              ingestion threads (cp2_set_ingest).  UNLIKE the single calls, which stop at the first file that fails, every file is
 *              attempted on its own: a file that cannot be opened, written or synced leaves its own matched requests _UNWRITTEN, every
 *              other file is still written and counted, and the call returns CP2_ERR_IO with "cannot write <file>: <reason>" naming
 *              the failing file that comes first in (dataset index, slot) order, the dataset index being the lowest that names the
 *              file.  Where no write fails the result equals the per-dataset loop's.
 *   Cache      cache_paths (n_ds entries, may be NULL, entries may be NULL): <cache_paths[k]> and <cache_paths[k]>.kept are restamped as
 *              cache_path of the single calls is, for the files this call wrote that hold a request naming ds[k]'s handle, under the
 *              same rule: only where the stamp equalled the file's stat taken before its first write.  Two handles over one base name
 *              that repair the SAME file in one call see one write of it, where the loop's second call would find the first call's
 *              stamp stale.
 *   Trace      CP2_TRACE prints one line per call: datasets, requests, chunks, requests with paths, matched, written, files, bytes,
 *              seconds, GB/s, stamps restamped.
 *   Out of scope   cp2_multi_* datasets (their shards by slots are plain datasets and may be listed). */
int cp2_datasets_repair_blocks_many(cp2_ctx* ctx, cp2_dataset* const* ds, size_t n_ds,
                                    const uint64_t* req /* n x 3: index into ds, dataset slot, block of the slot */,
                                    const uint8_t* data /* n x blockSize */,
                                    const uint8_t* paths /* packed 32-byte rows, may be NULL */,
                                    const uint64_t* path_off /* n + 1 rows, NULL iff paths is */,
                                    size_t n, int flags,
                                    const char* const* cache_paths /* n_ds entries, may be NULL, entries may be NULL */,
                                    uint32_t* status /* n */, size_t* n_written /* may be NULL */);

/* ---- fill sessions: slots filled from proved blocks in any order into a compact dataset ----------------------------------------------
 * A node that takes on a slot holds only the manifest's slot root.  It receives the slot's network blocks from peers, in any order and
 * over many round trips, each with its path.  cp2_blocks_verify can check them, but forgets the block roots it computed, and building
 * the dataset afterwards (cp2_dataset_build) reads and hashes every byte a second time.  A compact dataset IS the tree over the block
 * roots, so a session keeps each proved root where that tree has it and turns into a dataset when the last block has arrived.
 *
 * The handle: cp2_fill names the session in a caller's source; the entry points spell it `void*` (cp2_fill is void, so `cp2_fill* f;
 * cp2_fill_begin(..., &f)` is exact), because the mechanical comparison of this header with the Nim binding knows a fixed set of
 * handle types.  One context, whole sessions: free a session before its context.
 *
 * cp2_fill_begin opens a session for local slots [first_slot, first_slot + n_local) whose roots the caller states.
 *   Checked    cfg, first_slot and n_local exactly as cp2_dataset_build checks them, nCells a power of two; CP2_ERR_INVALID otherwise, and
 *              for a NULL argument.  A context whose stream will not drain is refused (CP2_ERR_HIP).
 *   Source     cfg->file_base != NULL (SlotFile): proved blocks are written to "<file_base><slot>.dat".  file_base == NULL (fake source):
 *              nothing is written and the finished dataset has the fake source of cfg->seed -- the analogue of CP2_REPAIR_CHECK_ONLY.
 *   Memory     the compact layout of n_local slots (2 x nBlocks - 1 nodes of 32 bytes per slot), allocated once, plus the roots.  A host
 *              bitmap of n_local x nBlocks bits is the authority on which blocks are present.
 *   Roots      slot_roots: n_local x 32 bytes from the manifest; values >= r are reduced, as everywhere else.
 *
 * cp2_fill_add checks n blocks with their paths and keeps those that prove.
 *   Data path  cp2_blocks_verify's, unchanged: chunks of half the context's staging, caller-pinned buffers read in place, the pinned ring
 *              otherwise, each chunk's paths uploaded with it.  The last device step (k_block_path_commit) also stores the block root of
 *              every candidate that reconstructs its slot root into layer 0 of the session's compact buffer.
 *   Refused    before any device or file work, CP2_ERR_INVALID, the request index (where there is one) in cp2_last_error, outputs
 *              untouched: a NULL session; a NULL array when n > 0 (n_new may be NULL); a slot outside the local range; a block >=
 *              nBlocks; a session that has been finished.  n == 0: CP2_OK.
 *   Result     status[i] = CP2_FILL_NEW, _MISMATCH, _DUPLICATE or _UNWRITTEN.  The same (slot, block) may appear twice in one call or
 *              across calls (two peers may answer): the lowest proved index of the first call that proves it is NEW, every later proved
 *              one is DUPLICATE and is not written again.  A wrong block or path is not an error: CP2_OK.
 *   Write      repair's rules: the NEW blocks grouped by file in ascending offset order, missing files created, one fdatasync per file
 *              and call.  The first file that cannot be opened, written or synced stops the writing: CP2_ERR_IO, its NEW blocks and
 *              those of later files become CP2_FILL_UNWRITTEN, and so do their duplicates in the same call (never DUPLICATE for a block
 *              that is still missing).
 *   Presence   a block's bit is set only after its file has been synced (at once for the fake source), so an UNWRITTEN block stays
 *              missing and can be sent again.  *n_new = the bits this call set.  CP2_TRACE prints one line per call.
 *
 * cp2_fill_missing: host only.  The lowest min(cap, *n_missing) absent (dataset slot, block) pairs in ascending order into `missing`;
 * *n_missing = the number of all absent blocks.  cap == 0 with a NULL `missing` only counts.
 * A finished session is not refused: it answers 0.
 *
 * cp2_fill_finish turns a complete session into a dataset.
 *   Refused    CP2_ERR_INVALID while any block is absent, cp2_last_error naming the count and the first missing pair; the session stays
 *              usable.  Also for a session already finished.
 *   Work       the upper layers of all n_local trees are built from layer 0 with the builders' layer kernel, one launch per layer over all
 *              slots, and the top layer is compared on the device with the stated roots (a difference: CP2_ERR_IO naming the slot, no
 *              dataset).  No slot byte is read or hashed.
 *   Result     *out = a new cp2_dataset that owns the session's buffer (no copy): compact (cp2_dataset_keeps_trees == 2), source as begun.
 *              It is an ordinary dataset: cp2_dataset_set_roots, proof inputs, cp2_proof_inputs_generate_many, scrub, repair and block
 *              proofs work on it; free it with cp2_dataset_free.
 *   Cache      with cache_path the kept form is saved first, under the name rule of cp2_dataset_build_cached (beside a tree cache, as
 *              "<cache_path>.kept") and with the (size, mtime) stamps of the slot files as they stand: a later cp2_dataset_build_cached
 *              of the same configuration, in any process, loads it instead of rebuilding.  A save that fails returns its status, no
 *              dataset, and the session stays complete and usable.
 *   After      a successful finish the session accepts only cp2_fill_free.
 *
 * Out of scope: cp2_multi_* (a session lives in one context); fetching and erasure decoding, which stay with the caller.  Saving and
 * resuming a half-filled session, and re-checking the blocks already on disk that its checkpoint covers: the checkpoint section below. */
typedef void cp2_fill;
#define CP2_FILL_NEW        0  /* proved against the slot root, first time seen: root kept, block written            */
#define CP2_FILL_MISMATCH   1  /* block + path do not reconstruct the slot root: nothing kept, nothing written       */
#define CP2_FILL_DUPLICATE  2  /* proved, but the block is already present (earlier call, or a lower request index   */
                               /* of this call): not written again                                                   */
#define CP2_FILL_UNWRITTEN  3  /* proved and new, but its file could not be written or synced (call: CP2_ERR_IO)     */
int cp2_fill_begin(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local,
                   const uint8_t* slot_roots /* n_local x 32, from the manifest */, void** out /* cp2_fill** */);
int cp2_fill_add(void* f /* cp2_fill* */, const uint64_t* slot_block /* n x 2: dataset slot, block */, const uint8_t* data /* n x blockSize */,
                 const uint8_t* paths /* n x depth x 32 */, size_t n, uint32_t* status /* n */, size_t* n_new);
int cp2_fill_missing(const void* f /* const cp2_fill* */, uint64_t* missing /* cap x 2: (slot, block), ascending */, size_t cap,
                     uint64_t* n_missing);
int cp2_fill_finish(void* f /* cp2_fill* */, const char* cache_path /* may be NULL */, cp2_dataset** out);
void cp2_fill_free(void* f /* cp2_fill* */);

/* ---- fill checkpoints: a session saved at any point and resumed against what is on disk ----------------------------------------------
 * A session lives for as long as its blocks take to arrive.  What it has proved so far exists in its host bitmap and in layer 0 of its
 * compact buffer only: were the process to die, the blocks already in the slot files could not be proved again without their paths, and
 * the slot would have to be fetched whole.  cp2_fill_save writes both down; cp2_fill_resume, in any later process, opens a session from
 * them and trusts the disk only as far as the device has re-checked it.
 *
 * cp2_fill_save writes a checkpoint of an unfinished session to `path`.
 *   Contents   "CP2FILL1", the geometry (cell_size, block_size, n_cells, n_slots, first_slot, n_local), the source kind, the seed and the
 *              file base name, the stated slot roots (canonical), the presence bitmap, layer 0 of the compact buffer (n_local x nBlocks
 *              rows of 32 bytes; rows of absent blocks are written as zeros, so two saves of one state are byte-identical), and the
 *              checksum of the kept form over all of it (csrc/fill_checkpoint.hpp has the layout).
 *   Work       one download on the context's stream; written to "<path>.tmp.<pid>", synced, then renamed.  Nothing of the session changes.
 *   Refused    CP2_ERR_INVALID: a NULL session or path; a finished session (its durable form is the kept cache of cp2_fill_finish).
 *              CP2_ERR_HIP: a context whose stream will not drain.
 *   Failure    CP2_ERR_IO naming the file; an older checkpoint at `path` stays intact.
 *   Durable    a block's bit is set only after its slot file has been synced, so every block a checkpoint calls present was durable when
 *              the checkpoint was written.  Blocks added after the last save are simply missing again after a resume: there is no
 *              journal per add.
 *
 * cp2_fill_resume opens a session from the checkpoint at `path`.
 *   Checked    cfg, first_slot, n_local and slot_roots exactly as cp2_fill_begin checks them.  The checkpoint must be intact (magic,
 *              sizes, checksum): a missing, truncated or corrupt file is CP2_ERR_IO naming the path.  It must describe THIS session --
 *              geometry, range, source kind, the seed (fake source), the file base name (slot files), the stated roots after reduction
 *              mod r: otherwise CP2_ERR_INVALID naming the first field that differs.  In every failing case no session is created and
 *              *out = NULL.
 *   Re-check   every block the checkpoint calls present is checked against what the source holds now.  Slot files: a file that does not
 *              exist, or ends before the block does, drops that block without a read (absence is a state, not an error); the others are
 *              read from "<file_base><slot>.dat", file by file in ascending offset order, in chunks of half the context's staging, and
 *              go through cp2_dataset_repair_blocks' data path unchanged; a read that fails is CP2_ERR_IO with the builders' message and
 *              no session.  Fake source: the blocks are regenerated on the device and hashed the same way.  The last device step
 *              (k_block_root_recheck) compares each fresh block root with the row of layer 0 the checkpoint kept and zeroes the row
 *              where they differ; the host clears that block's bit.  *n_dropped (may be NULL) = the blocks dropped either way.
 *   Flags      CP2_RESUME_TRUST_FILES: the checkpoint's presence bits are taken as they are, no slot byte is read, *n_dropped = 0.  What
 *              remains is cp2_fill_finish's comparison of the top layer with the stated roots (CP2_ERR_IO naming the slot).
 *   Result     *out = a session indistinguishable from one begun fresh that has received exactly the surviving blocks: cp2_fill_missing
 *              lists the dropped blocks among the absent ones, cp2_fill_add takes them again as CP2_FILL_NEW, and the finished dataset is
 *              the one cp2_dataset_build makes.  CP2_TRACE prints one line (blocks present, re-read, dropped, bytes, seconds, GB/s).
 *
 * Out of scope: cp2_multi_*; a journal per add; adopting blocks the checkpoint does not cover. */
#define CP2_RESUME_TRUST_FILES 1   /* flag: take the checkpoint's presence bits as they are, read no slot byte */
int cp2_fill_save(const void* f /* const cp2_fill* */, const char* path);
int cp2_fill_resume(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local,
                    const uint8_t* slot_roots /* n_local x 32, from the manifest */, const char* path, int flags, void** out /* cp2_fill** */,
                    uint64_t* n_dropped /* may be NULL */);

/* ---- fill sessions that serve: block proofs from a session while it is still filling ---------------------------------------------------
 * A session becomes a dataset only when its last block has arrived, which takes minutes to hours at network speed; until then it holds
 * thousands of blocks it has proved and written, and cp2_dataset_block_proofs serves none of them.  Nothing new has to be learned to
 * serve them: a path that ends in the stated slot root proves every node on it -- the `depth` siblings the peer sent and the `depth`
 * ancestors the walk computed -- and the session's compact buffer, the whole tree over the block roots, has a row for each.  A session
 * that keeps nodes stores them there, and a present block's proof is a gather from the session's own buffer.
 *
 * cp2_fill_keep_nodes turns node keeping on, at any point of an unfinished session.  One-way; a second call is a no-op (CP2_OK).
 *   Work       the rows of layer 0 whose block is absent are zeroed, every upper layer is built once with the builders' layer kernel as
 *              cp2_fill_finish does, and a host bitmap with one bit per row of the compact layout records what is known: a block root
 *              where the block is present, a parent where both children are known (one child for the last node of an odd layer).  So a
 *              resumed session, or one that was half full before the call, serves the blocks whose whole neighbourhood it already holds.
 *   Afterwards cp2_fill_add ends in k_block_path_commit_nodes: the same walk and verdicts, and for every request that proves, the block
 *              root, the in-range siblings and the ancestors of its path are stored where the tree has them and their bits set (whether
 *              or not the block is then written: a CP2_FILL_UNWRITTEN block stays missing, its nodes are authentic).  A request that
 *              does not prove leaves nothing in the buffer.  Statuses, writes, presence and the trace line of cp2_fill_add are unchanged.
 *   Refused    CP2_ERR_INVALID: a NULL session; a finished session.  CP2_ERR_HIP: a context whose stream will not drain.
 *
 * cp2_fill_block_proofs serves proofs from the session's buffer, in cp2_dataset_block_proofs' layout.
 *   Requests   slot_block (n x 2 uint64: dataset slot inside the local range, block of the slot < nBlocks); the same pair may repeat.
 *   Result     status[i] = CP2_FILL_PROOF_OK (served), _ABSENT (the block is not present) or _PARTIAL (present, but a sibling of its path
 *              is not known yet: only blocks that arrived before keeping was turned on can be, until later adds bring their
 *              neighbourhood).  block_roots (n x 32 bytes, may be NULL) and paths (n x depth x 32 bytes, bottom first, zero for a sibling
 *              past its layer's end, may be NULL); the rows of a request that is not OK are zeros.  One upload of the row list, one gather
 *              on the device, one download; with both outputs NULL the statuses come from the host bitmaps with no device work.  A block
 *              added after keeping was turned on is served from the moment it is present.  CP2_TRACE prints one line (requests, served,
 *              absent, partial, seconds).
 *   Refused    CP2_ERR_INVALID, the request index (where there is one) in cp2_last_error, outputs untouched: a NULL session; NULL
 *              slot_block or status when n > 0; a slot outside the local range; a block >= nBlocks; a session that does not keep nodes;
 *              a finished session (its proofs come from the dataset).  n == 0: CP2_OK.
 *   Read-only  nothing of the session changes.
 *
 * Checkpoints stay as they are (layer 0 and the presence bitmap): a resumed session keeps no nodes until cp2_fill_keep_nodes is called.
 * cp2_fill_finish is unchanged: it rebuilds every layer, which overwrites the kept nodes with equal values.
 * Out of scope: cp2_multi_*; deriving nodes a second time.  Accepting a block without its whole path on the strength of kept nodes: the
 * section on anchored fill adds below.
 * The three values are written in parentheses: the per-request results of cp2_fill_add above stay the only bare CP2_FILL_* numbers. */
#define CP2_FILL_PROOF_OK      (0)  /* status: the proof is served                                                      */
#define CP2_FILL_PROOF_ABSENT  (1)  /* status: the block is not present                                                 */
#define CP2_FILL_PROOF_PARTIAL (2)  /* status: the block is present, but a sibling of its path is not known yet         */
int cp2_fill_keep_nodes(void* f /* cp2_fill* */);
int cp2_fill_block_proofs(void* f /* cp2_fill* */, const uint64_t* slot_block /* n x 2: dataset slot, block */, size_t n,
                          uint32_t* status /* n */, uint8_t* block_roots /* n x 32, may be NULL */,
                          uint8_t* paths /* n x depth x 32, may be NULL */);

/* ---- anchored fill adds: blocks whose path stops at a node the session already holds ---------------------------------------------------
 * After cp2_fill_keep_nodes every proved path leaves its siblings and ancestors in the session's buffer.  They also shorten what the next
 * peer has to send: a computed node that equals an authentic node proves everything below it, by the collision argument the whole walk
 * rests on, so a block whose ancestor at level a is known needs its a lowest siblings only.  When every add uses its lowest known
 * ancestor, a slot of nBlocks = 2^k blocks receives nBlocks - 1 siblings in all, in any arrival order, instead of depth x nBlocks, and
 * half of its blocks need none: their block root arrived as the level-0 sibling of their neighbour's path, so their bytes can come from
 * any source, a peer without a tree or an untrusted cache included.  What this saves is bytes on the wire and on the upload; a block
 * still costs its own hashing, next to which a path is nothing.  Serving needs nothing new: paths are stored bottom first, so a server
 * truncates a proof of cp2_fill_block_proofs or cp2_dataset_block_proofs by sending its first a rows.
 *
 * cp2_fill_anchors: host only, read-only.  levels[i] = the lowest level l in [0, depth] at which the session knows the node above block
 * slot_block[i] (level 0: its block root; level depth: the stated slot root, which always counts).  A session that does not keep nodes is
 * not refused: it answers depth throughout.
 * A PRESENT block of a session that keeps nodes answers 0 (its block root is known: kept by the add or the adopt that brought it, or derived
 * from presence by cp2_fill_keep_nodes); of a session that keeps none it answers depth like any other.  An absent block answers 0 when
 * its block root arrived as a neighbour's sibling, or with a CP2_FILL_UNWRITTEN add of its own.
 *   Refused    CP2_ERR_INVALID, the request index (where there is one) in cp2_last_error, outputs untouched: a NULL session; NULL
 *              slot_block or levels when n > 0; a slot outside the local range; a block >= nBlocks; a finished session.  n == 0: CP2_OK.
 *
 * cp2_fill_add_anchored is cp2_fill_add with paths of stated lengths.
 *   Requests   levels[i] <= depth siblings for request i, bottom first; `paths` holds them packed in request order, sum(levels) x 32 bytes
 *              (may be NULL when every level is 0).  Any level whose node is known may be stated, not only the lowest; level depth is
 *              cp2_fill_add's whole path.
 *   Data path  cp2_fill_add's, unchanged; a chunk's packed paths are one contiguous range and are uploaded with it.  The last device step
 *              (k_block_path_commit_anchored) walks request i up levels[i] levels and compares the result with the kept row of that node
 *              (level depth: with the stated slot root); level 0 runs no permutation, it compares the fresh block root with the kept
 *              row.  A request that proves stores its block root, its in-range siblings and the ancestors below the level where the
 *              tree has them, and their bits are set; the anchor and everything above it are never written.  A request that does not
 *              prove leaves nothing in the buffer.
 *   Refused    before any device or file work, CP2_ERR_INVALID, the request index (where there is one) in cp2_last_error, outputs
 *              untouched: everything cp2_fill_add refuses; a session that does not keep nodes; a level above depth; a level whose node
 *              was not known WHEN THE CALL STARTED (a node that another request of the same call would prove does not count); NULL
 *              levels when n > 0; NULL paths when any level is not 0.  n == 0: CP2_OK.
 *   Result     status[i] = CP2_FILL_NEW, _MISMATCH, _DUPLICATE or _UNWRITTEN with cp2_fill_add's meaning, rules of writing, roll-back and
 *              presence; a proved CP2_FILL_UNWRITTEN block stays missing and its nodes stay known.  CP2_TRACE prints cp2_fill_add's line
 *              and the siblings received against n x depth.
 *
 * cp2_fill_add, cp2_fill_keep_nodes, cp2_fill_block_proofs, checkpoints and cp2_fill_finish are unchanged.
 * Out of scope: cp2_multi_*; checkpointing the known siblings of absent blocks (a resumed session derives what presence gives it, as
 * before); adopting blocks from disk (its own section, further down); any change to what is served. */
int cp2_fill_anchors(const void* f /* const cp2_fill* */, const uint64_t* slot_block /* n x 2: dataset slot, block */, size_t n,
                     uint32_t* levels /* n */);
int cp2_fill_add_anchored(void* f /* cp2_fill* */, const uint64_t* slot_block /* n x 2: dataset slot, block */,
                          const uint8_t* data /* n x blockSize */, const uint32_t* levels /* n */,
                          const uint8_t* paths /* sum(levels) x 32, packed in request order */, size_t n, uint32_t* status /* n */,
                          size_t* n_new);

/* ---- proved blocks added to many fill sessions in one pass ------------------------------------------------------------------------------------
 * A node that takes on slots of many datasets runs one session per dataset on one context, and the blocks of all of them arrive
 * interleaved.  Every cp2_fill_add / cp2_fill_add_anchored is a pass of its own (a data-path set-up, launches that last one wave's lifetime
 * whatever their size, a drain); across thousands of one-slot sessions a batch of arrivals is thousands of calls of a few blocks each.
 * cp2_fills_add_many is ONE pass over the blocks of all of them: the last device step (k_block_path_commit_many) takes the session per
 * request from a table uploaded once per call.
 *   Sessions   fills[0 .. n_fills): sessions of `ctx` with one cell_size and block_size.  They may differ in n_cells (so in nBlocks and
 *              depth), n_slots, local range, source (slot files or fake), file base name, seed, and in whether they keep nodes.
 *   Requests   req: n x 3, (index into fills, dataset slot, block of the slot); data: n x blockSize.  Request i brings levels[i] siblings,
 *              bottom first; levels == NULL: the cp2_block_proof_depth of its own session.  `paths` holds the siblings packed in request
 *              order and may be NULL only when every level is 0.  A request whose level is its session's depth is a cp2_fill_add request
 *              and is accepted by every session; a shorter one is a cp2_fill_add_anchored request: its session must keep nodes, and the
 *              anchor must be known WHEN THE CALL STARTS.
 *   Meaning    by the calls that exist.  With R_k the subsequence, in request order, of the requests that name fills[k], the call leaves
 *              every session, every slot file and every output entry as this loop leaves them: for k in order, cp2_fill_add(fills[k],
 *              R_k ...) when levels is NULL or fills[k] keeps no nodes, cp2_fill_add_anchored(fills[k], R_k ...) otherwise, continuing
 *              after a call that returns CP2_ERR_IO.  NEW / DUPLICATE is decided per session by the lowest proved index of R_k; the
 *              writer, its roll-back, CP2_FILL_UNWRITTEN and presence after the sync are cp2_fill_add's, per session; n_new[k] (n_fills
 *              entries, may be NULL) is the number of bits set in session k.  The blocks are written from their rows of `data`, session
 *              after session: the writes are serial.
 *   I/O        a file that cannot be written stops that session's writing, as in cp2_fill_add; the other sessions' writes still
 *              happen.  CP2_ERR_IO, and cp2_last_error names the first failing file in `fills` order.
 *   Refused    all or nothing, unlike the loop: every check of every request runs before any device or file work, and a refused call
 *              changes no session, file or output.  CP2_ERR_INVALID with the fills index or the request index in cp2_last_error: a NULL
 *              ctx; with n > 0, NULL fills, req, data or status; fills[k] NULL, of another context, finished, or of another cell_size /
 *              block_size than fills[0]; the same session listed twice (two writers to one file set); a session index >= n_fills;
 *              everything cp2_fill_add or cp2_fill_add_anchored refuses for the request inside its session (a level below the depth of
 *              a session that keeps no nodes among it); NULL paths while any level is not 0.  n == 0: CP2_OK with n_new zeroed.  A
 *              context whose stream will not drain: CP2_ERR_HIP.
 *   Trace      CP2_TRACE prints one line: sessions, requests, proved, new, siblings received, bytes, seconds, GB/s, seconds writing.
 * Out of scope: cp2_multi_*; a many-session finish, save or adopt (each session's own calls, as before); spreading the file writes over
 * threads. */
int cp2_fills_add_many(cp2_ctx* ctx, void* const* fills /* cp2_fill* each */, size_t n_fills,
                       const uint64_t* req /* n x 3: index into fills, dataset slot, block of the slot */,
                       const uint8_t* data /* n x blockSize */,
                       const uint32_t* levels /* n, or NULL: every request brings its session's whole path */,
                       const uint8_t* paths /* packed in request order */, size_t n,
                       uint32_t* status /* n: CP2_FILL_* */, size_t* n_new /* n_fills entries, may be NULL */);

/* replaces `writeCircomMainComponent`, reference/nim/proof_input/src/cli.nim:186-204 */
int cp2_write_circom_main(const cp2_config* cfg, const char* path);

/* ---- adopting blocks from disk: bytes the slot files hold but the session does not count ---------------------------------------------------
 * A session learns of a block's bytes through cp2_fill_add*, from the caller's memory.  Bytes that are in "<file_base><slot>.dat" already
 * but not in the presence bitmap -- blocks added after the last cp2_fill_save and before a crash, a slot file restored from a backup or
 * copied from another node, a file whose checkpoint was lost -- are dead weight to it.  The kept nodes make them cheap to take over: a
 * computed node that equals an authentic node proves everything below it, so after cp2_fill_keep_nodes one proved path leaves depth
 * authentic siblings, the top one vouches for half the slot, and the stated slot root vouches for all of it.  An intact file is adopted
 * whole with no network traffic; a file with a few damaged blocks costs about depth siblings and one block per damaged block.
 *
 * cp2_fill_adopt(f, first_slot, n_slots, flags, n_read, n_adopted) works on slots first_slot .. + n_slots (n_slots == 0: every local slot).
 *   Candidates the ABSENT blocks of those slots that their file covers completely.  A file that does not exist, or ends before the block
 *              does, yields no candidate for that block: absence is a state, as in cp2_fill_resume.  The candidates are read file by file
 *              in ascending offset order, in chunks of half the context's staging, and reduced to fresh block roots on cp2_fill_add's data
 *              path, exactly as the re-check of cp2_fill_resume reads the present ones.  Present blocks are never read.  A read that
 *              fails is CP2_ERR_IO with the builders' message, and nothing of the session has changed.  *n_read = the blocks read.
 *              *n_read counts what THIS call read: every absent block of the selected slots that its file covers, whether or not an earlier
 *              call read and remembers it (a second reading adopt of an unchanged slot reads the same blocks again); 0 with
 *              CP2_ADOPT_NO_READ.
 *   Remembered the session keeps the fresh block roots of its candidates in a device buffer of its own (n_local x nBlocks rows, allocated
 *              by the first adopt) and a host bitmap of the rows that hold one.  A read refreshes them for the slots it covers.
 *              CP2_ADOPT_NO_READ reads no slot byte and judges what is remembered: use it after later adds have made more nodes known.
 *              It TRUSTS THE FILES UNCHANGED SINCE THEY WERE READ, as everything after a resume's re-check does.  A block that has become
 *              present in the meantime is no longer a candidate.
 *   Judgement  on the device.  Per row of the compact layout of those slots: `known` is the session's bit, the top row always known (it is
 *              the stated slot root).  A layer-0 row has a computed value where a candidate exists; a node above has one when both
 *              children are known or computed (one child for the last node of an odd layer and for the one-block slot), namely
 *              compress(vL, vR, key) with v = the kept value where known, the computed one otherwise, and the keys of the tree builders
 *              (k_adopt_layer, one launch per layer).  A known node whose computed value equals its kept value matches.  A row that is
 *              not known and has a computed value is PROVED when the first known node on its way up matches and every row between has a
 *              computed value (k_adopt_resolve): it is copied into the session's buffer and its bit is set.  A block is ADOPTED when its
 *              layer-0 row is proved, or is known and equals its candidate.  Nothing else of the buffer is written; a known row is never
 *              written, a computed value can only be proved equal to it.
 *   Presence   every file with adopted blocks is fdatasync'ed once, then its presence bits are set; *n_adopted = the bits set.  A sync
 *              that fails is CP2_ERR_IO naming the file: that file's blocks stay absent and their nodes stay known -- they are authentic,
 *              as with CP2_FILL_UNWRITTEN.  Adopting nothing is CP2_OK.  An adopted block is served by cp2_fill_block_proofs at once, and
 *              a checkpoint saved afterwards covers it.
 *   Refused    CP2_ERR_INVALID, the reason in cp2_last_error, nothing changed, outputs untouched: a NULL session; a finished session; a
 *              session that does not keep nodes; slots outside the local range; an unknown flag; a session of the fake source (it has no
 *              files).  A context whose stream will not drain: CP2_ERR_HIP.
 *   CP2_TRACE  one line per call: blocks read, candidates, adopted, rows proved, bytes, seconds, GB/s.
 *
 * cp2_fill_add*, cp2_fill_missing, cp2_fill_anchors, cp2_fill_block_proofs, checkpoints and cp2_fill_finish are unchanged.
 * Out of scope: cp2_multi_*; deriving a parent from two known children without a match; checkpointing known siblings or candidates (a
 * resumed session adopts again); pipelining the reads -- they are the re-check's reads, which are host-bound. */
#define CP2_ADOPT_NO_READ 1   /* flag: read no slot byte; judge the candidates remembered from earlier calls */
int cp2_fill_adopt(void* f /* cp2_fill* */, uint64_t first_slot, uint64_t n_slots /* 0: every local slot */, int flags,
                   uint64_t* n_read /* may be NULL */, uint64_t* n_adopted /* may be NULL */);

/* ---- fill checkpoints with nodes: the kept nodes saved, and restored only as far as the device re-derives them -----------------------------
 * cp2_fill_save writes presence and layer 0.  Everything a keeping session has beside them -- the proved siblings and ancestors its proofs,
 * anchors and adopts rest on -- lives in the upper rows of its buffer and in its known bitmap, and a cp2_fill_resume followed by
 * cp2_fill_keep_nodes knows a node only where both children are present: in a slot half filled in network order nearly every present block
 * answers CP2_FILL_PROOF_PARTIAL after a restart.  These two calls save the kept nodes and bring them back by the rule of every checkpoint
 * here: nothing a file states is believed until the device has re-derived it from the stated slot roots.
 *
 * cp2_fill_save_nodes(f, path)  everything cp2_fill_save does and refuses, for a session that keeps nodes; one that does not is
 *   CP2_ERR_INVALID.  The file is format CP2FILL2: CP2FILL1's ten words, base name, stated roots and presence bitmap where and what they
 *   are there (the magic differs); the known bitmap, ceil(rows / 64) words, bit r = row r of the compact layout, bits past the last row 0;
 *   layer 0, n_local x nBlocks rows, a row zero unless its block is present or its row known; the known rows of the layers strictly
 *   between layer 0 and the top, packed in ascending row order; the checksum.  The top rows are not stored: their bits are, their value is
 *   the stated root.  Rows that are not known are zeros or left out, so two saves of one state are byte-identical.  Written beside `path`,
 *   synced and renamed, as cp2_fill_save writes.  Nothing of the session changes; the candidates cp2_fill_adopt remembers are not saved.
 *
 * cp2_fill_resume_nodes(ctx, cfg, first_slot, n_local, slot_roots, path, flags, &f, &n_dropped, &n_restored, &n_unproved, &n_rejected)
 *   accepts CP2FILL2, and CP2FILL1, for which the result is exactly cp2_fill_resume followed by cp2_fill_keep_nodes (the three new counts
 *   0).  Checks, refusals, the drop of blocks a short file cannot back, the re-check and CP2_RESUME_TRUST_FILES are cp2_fill_resume's.
 *   A CP2FILL2 file with known bits past the last row, a packed-row count that disagrees with its known bitmap, or a size its header does
 *   not allow is CP2_ERR_IO naming the path.  cp2_fill_resume keeps refusing a CP2FILL2 file by its magic.
 *   The resumed session keeps nodes.  Its known set:
 *     D          what presence gives: cp2_fill_keep_nodes on the bitmap and layer 0 that survived the re-check.
 *     Candidates the file's known rows below the top that are not in D, with the values the file states, in a device buffer of their own:
 *                never in the session's buffer unproved.  The layer-0 rows of dropped blocks are among them.
 *     Restore    on the device, top-down, one launch per layer (k_nodes_restore_layer).  A node that is known -- in D, restored by the
 *                launch before, or a top row: the stated slot root -- whose children are all known or candidates (one child for the last
 *                node of an odd layer and for the one-block slot), at least one a candidate, is recomputed from them with the tree
 *                builders' keys.  Where the result equals its value, the candidate children are copied into the session's buffer and are
 *                RESTORED: known from here on.  Where it differs they are REJECTED.  A candidate whose parent is not known in the resumed
 *                session, or whose sibling is neither known nor a candidate, is reached by no launch: UNPROVED.
 *     Top rows   a top row's bit is taken over as saved: its value is the stated root.
 *   *n_restored, *n_rejected, *n_unproved count those rows (each may be NULL).  Neither rejected nor unproved rows are an error: they are
 *   simply not known, and the call returns CP2_OK.  With unchanged files every saved row is in D or restored.
 *   The session is indistinguishable from one that has proved exactly D and the restored rows: cp2_fill_block_proofs, cp2_fill_anchors,
 *   cp2_fill_add_anchored, cp2_fill_adopt, both saves and cp2_fill_finish.  A dropped block whose root was restored is absent with anchor
 *   level 0: cp2_fill_add_anchored takes it back as bare bytes.
 *   CP2_TRACE  cp2_fill_resume's line, cp2_fill_keep_nodes' line, then one line: format, candidates, restored, rejected, unproved, dropped.
 *
 * Out of scope: cp2_multi_*; saving the candidates cp2_fill_adopt remembers; deriving a parent from two known children. */
int cp2_fill_save_nodes(const void* f /* cp2_fill* */, const char* path);
int cp2_fill_resume_nodes(cp2_ctx* ctx, const cp2_config* cfg, uint64_t first_slot, uint64_t n_local, const uint8_t* slot_roots,
                          const char* path, int flags /* 0 or CP2_RESUME_TRUST_FILES */, void** out /* cp2_fill** */,
                          uint64_t* n_dropped /* may be NULL */, uint64_t* n_restored /* may be NULL */,
                          uint64_t* n_unproved /* may be NULL */, uint64_t* n_rejected /* may be NULL */);

/* ---- many fill sessions finished in one pass ------------------------------------------------------------------------------------------------
 * The step between the adds of many sessions (cp2_fills_add_many) and the dataset trees of what they become (cp2_datasets_set_roots_many).
 * Per session cp2_fill_finish is one launch per layer of the tree over the block roots -- a lone wave or less in a one-slot session --, an
 * upload, a comparison launch, a download and a drain.  cp2_fills_finish_many is ONE pass: level l of every session's trees is one launch
 * (k_finish_layer_many, the session per lane from a table uploaded once), and the comparison with the stated roots rides on each tree's
 * last level.  This lifts the many-session finish that the section of cp2_fills_add_many left out of scope.
 *   Sessions   fills[0 .. n_fills): sessions of `ctx`.  They may differ in everything else: n_cells (so nBlocks and depth), n_local,
 *              n_slots, cell and block size, source, and whether they keep nodes.
 *   Meaning    by the call that exists.  After CP2_OK, out[k], fills[k] and the kept file of cache_paths[k] are what
 *              cp2_fill_finish(fills[k], cache_paths[k], &out[k]) leaves, for every k: a compact dataset that owns the session's buffer (no
 *              copy), source as begun; the kept form under cp2_dataset_build_cached's name rule; a session that accepts only cp2_fill_free.
 *              cache_paths is NULL, or n_fills entries each of which may be NULL.
 *   Refused    all or nothing: every check runs before any device or file work, and a refused call changes no session, file or out
 *              entry.  CP2_ERR_INVALID with the fills index in cp2_last_error: a NULL ctx; with n_fills > 0, NULL fills or out; fills[k]
 *              NULL, of another context, or finished; fills[k] listed twice; fills[k] with a block absent (the count and the first missing
 *              pair, as cp2_fill_finish words it).  n_fills == 0: CP2_OK.  A context whose stream will not drain: CP2_ERR_HIP.
 *   Device     one upload of the session table and the level tables, one launch per level for the sessions that still have it, one
 *              download of one verdict per (session, local slot), one drain, all on the context's stream.
 *   Verdicts   a tree that does not end in its stated root: CP2_ERR_IO, cp2_last_error names the first fills[k] in order and the dataset
 *              slot in cp2_fill_finish's words.  No dataset is made and no session is finished.
 *   Cache      after the verdicts and before any hand-over, serially in `fills` order.  The first save that fails returns its status: no
 *              dataset, every session still complete and usable; kept files already written for earlier k stay (valid caches of complete
 *              sessions).  Only after all saves are the n datasets made -- all n objects before the first hand-over, so CP2_ERR_ALLOC is
 *              all or nothing too -- and the buffers handed over.
 *   Trace      CP2_TRACE prints one line: sessions, slots, rows built, launches, kept forms saved, milliseconds.
 * Out of scope: cp2_multi_*; a many-session begin, save or adopt (each session's own calls, as before); spreading the kept-file writes
 * over threads. */
int cp2_fills_finish_many(cp2_ctx* ctx, void* const* fills /* cp2_fill* each */, size_t n_fills,
                          const char* const* cache_paths /* NULL, or n_fills entries each of which may be NULL */,
                          cp2_dataset** out /* n_fills */);

/* ---- many fill sessions resumed in one pass -------------------------------------------------------------------------------------------------
 * The restart side of the many-session life cycle.  After a crash or an upgrade every session comes back through cp2_fill_resume: per
 * session a checkpoint read, two device allocations, two uploads with a drain each, and a re-check with a data-path set-up, launches and
 * drains of its own, reading block by block on one thread.  cp2_fills_resume_many is ONE pass: the checkpoints are read on the context's
 * ingestion threads, all sessions are opened and their roots and layer 0 go up through pinned staging with one drain, and every present
 * block of every session is re-read by the chunked reader of cp2_datasets_read_blocks -- each file opened once per chunk, the files
 * spread over the ingestion threads, one chunk ahead of the hashing -- and judged by one launch per chunk (k_block_root_recheck_addr,
 * the kept row of a block at an absolute address inside its own session's buffer).
 *   Sessions   entry k is (cfgs[k], first_slot = ranges[2k], n_local = ranges[2k + 1], slot_roots[k]: n_local x 32 bytes, paths[k]: a
 *              CP2FILL1 checkpoint).  Entries may differ in n_cells (so nBlocks and depth), n_slots, range, source (slot files or
 *              fake), base name and seed; they share cell_size and block_size (the data path has one shape: cp2_fills_add_many's
 *              rule).  Two entries may name the same files or the same checkpoint: resume only reads.
 *   Meaning    by the call that exists.  After CP2_OK, out[k] and n_dropped[k] are what cp2_fill_resume(ctx, cfgs[k], first_slot,
 *              n_local, slot_roots[k], paths[k], flags, &out[k], &n_dropped[k]) leaves, for every k: the same presence bitmap, the
 *              same layer 0 with the rows of dropped blocks zeroed, the same cp2_fill_missing list; a dropped block is accepted
 *              again as CP2_FILL_NEW.  Every session owns its allocations as cp2_fill_begin makes them (cp2_fill_finish hands the
 *              buffer over: nothing is shared) and keeps no nodes.  n_dropped may be NULL.
 *   Refused    all or nothing, unlike the loop: every check of every entry runs before a session exists; on any failure no session
 *              is created, every out[k] is NULL and n_dropped is untouched.  In this order, the lowest entry index first inside
 *              each step, the index in cp2_last_error ("fills: entry k: ..."): (1) CP2_ERR_INVALID: a NULL ctx; unknown flag bits;
 *              with n_fills > 0, NULL cfgs, ranges, slot_roots, paths or out; a NULL cfgs[k], slot_roots[k] or paths[k]; everything
 *              cp2_fill_begin refuses for entry k; a cell_size or block_size other than entry 0's.  (2) the checkpoints: one that is
 *              not intact (a CP2FILL2 file by its magic) is CP2_ERR_IO in cp2_fill_resume's words, naming the path; one that
 *              describes another session is CP2_ERR_INVALID naming the first field that differs.  (3) slot files that cannot be
 *              stat'ed: CP2_ERR_IO (a file that does not exist is a state: its blocks are dropped).  n_fills == 0: CP2_OK.  A
 *              context whose stream will not drain: CP2_ERR_HIP.
 *   Device     per session cp2_fill_begin's two allocations; roots and layer 0 of all sessions go up through pinned staging in pieces of
 *              at most the staging size, each piece one copy and one k_scatter_rows_addr launch, and one drain;
 *              then, without CP2_RESUME_TRUST_FILES, the re-check in chunks of half the staging size (cp2_datasets_read_blocks'
 *              chunks): two pooled pinned buffers, fake-source blocks regenerated on the device, repair's hashing, one judge launch.
 *   Failure    after the checks: a failed allocation is CP2_ERR_ALLOC and a slot-file read that fails is CP2_ERR_IO with the
 *              builders' message (never a dropped block).  Either frees every session already opened and leaves every out[k] NULL;
 *              the call returns only after the stream has drained and the reader is idle.
 *   Trace      CP2_TRACE prints one line: sessions, blocks present in the checkpoints, re-read, dropped, chunks, bytes, seconds, GB/s
 *              and the split (checkpoints, opens and uploads, re-check, host drops).
 * Out of scope: cp2_multi_*; CP2FILL2 checkpoints and a many-session cp2_fill_keep_nodes, cp2_fill_resume_nodes, cp2_fill_adopt or save
 * (each session's own calls, as before); a many-session begin; routing cp2_fill_resume or cp2_fill_adopt through this pass; O_DIRECT
 * or mapped reads. */
int cp2_fills_resume_many(cp2_ctx* ctx, const void* const* cfgs /* n_fills: const cp2_config* each */,
                          const uint64_t* ranges /* n_fills x 2: first_slot, n_local */,
                          const uint8_t* const* slot_roots /* n_fills entries, entry k: n_local[k] x 32 */,
                          const char* const* paths /* n_fills checkpoint files, CP2FILL1 */, size_t n_fills,
                          int flags /* 0 or CP2_RESUME_TRUST_FILES */, void** out /* n_fills: cp2_fill* each */,
                          uint64_t* n_dropped /* n_fills, may be NULL */);

/* ---- block multiproofs: many blocks of a slot served, checked and filled with shared Merkle nodes -------------------------------------
 * Every path-carrying call above takes one whole path per block.  Two blocks of one slot share every node above the point where their
 * paths meet: with whole paths that node is sent twice, uploaded twice and hashed twice.  A multiproof of a set B of blocks of one slot
 * sends only the nodes that cannot be computed from B and from each other, each once, and checking hashes each inner node of the
 * induced subtree once: a whole 128-block slot costs 127 compressions and no sent row, where whole paths cost 128 x 7 of each.
 *   Format     geometry as for block proofs: nBlocks = nCells / (blockSize / cellSize), depth = cp2_block_proof_depth, layer sizes m_0 =
 *              nBlocks, m_{l+1} = (m_l + 1) >> 1; a parent is compress(left, right, key), key = 1 on level 0 and 0 above, and an odd
 *              layer's last node (and the singleton) is compress(last, 0, key + 2).  For a non-empty set B of DISTINCT blocks let K_0 = B
 *              and K_{l+1} = { i >> 1 : i in K_l }.  The multiproof of B is the list of rows (l, i ^ 1) over every level l < depth and
 *              every i in K_l for which i ^ 1 is not in K_l and i ^ 1 < m_l, ordered by level ascending, then by index ascending.  Each
 *              row is a 32-byte little-endian field element, a value >= r taken mod r.  An out-of-range sibling is NOT sent (the
 *              single path carries a zero row there).  Checking computes every node of K_{l+1} from K_l and the sent rows, level by
 *              level; the proof holds when the one node of K_depth equals the stated slot root.
 *   Groups     requests come in groups: groups is n_groups x 2 uint64 (slot or root index, count), blocks holds the n = sum of the
 *              counts block indices, group after group, STRICTLY ASCENDING inside a group, and nodes holds the groups' rows packed in
 *              group order.  The same slot may appear in several groups: several proofs, perhaps from several peers, each with its
 *              own verdict.
 *   Verdict    belongs to the GROUP: one wrong block or one wrong row fails all of B, and the proof cannot say which one.  A caller who
 *              must know falls back to whole paths (cp2_blocks_verify) or anchors for that group.
 *
 * cp2_block_multiproof_rows, cp2_block_multiproof_layout: host only.  The number of rows of the multiproof of blocks[0, k), and the
 * (level, index) of every row in order (level_index: rows x 2 uint64).  SIZE_MAX / CP2_ERR_INVALID for a geometry the tree builders
 * refuse, k == 0, a block >= nBlocks or a list that is not strictly ascending.
 *
 * cp2_dataset_block_multiproofs serves multiproofs from what a dataset keeps: every node, or the compact layers.
 *   Requests   groups (dataset slot inside the local range, count) and blocks as above.
 *   Result     *n_rows = the rows of all groups, always the full count; nodes (cap x 32 bytes) receives them packed in group order,
 *              block_roots (n x 32 bytes, may be NULL) the block root of every request.  One upload of the row list, one gather on the
 *              device (cp2_dataset_block_proofs' own), one download.  With cap < *n_rows: CP2_ERR_INVALID, the needed count in
 *              cp2_last_error, and neither nodes nor block_roots is written.
 *   Refused    CP2_ERR_INVALID, the group index or the request index (where there is one) in cp2_last_error: as
 *              cp2_dataset_block_proofs, the roots-only dataset among them, and the request rules below.
 *   Read-only  nothing of the dataset changes.
 *
 * cp2_blocks_verify_multi checks n candidate blocks in groups, each group with its multiproof, against slot roots the caller states.
 *   Requests   slot_roots (n_roots x 32 bytes); groups (index into slot_roots, count); blocks; data (n x blockSize bytes, in the order
 *              of blocks); nodes (n_rows x 32 bytes).  The data path is cp2_blocks_verify's, unchanged; the sent rows, the stated roots
 *              and the job tables go up once.  Each chunk's fresh block roots are copied into a work table on the device; after the
 *              pass k_multiproof_layer runs once per level (one lane and one compression per inner node of the induced subtrees, all
 *              groups of the call in one launch), then one download of n_groups verdicts.
 *   Result     status[g] = CP2_BLOCK_MATCH (the group's candidates and rows reconstruct slot_roots[root]) or CP2_BLOCK_MISMATCH, one
 *              per GROUP; block_roots (n x 32 bytes, may be NULL) = what each candidate hashed to.  A wrong block or a wrong proof is
 *              not an error: CP2_OK.
 *   Trace      CP2_TRACE prints one line: groups, requests, matched groups, rows received against n x depth, compressions run against
 *              n x depth, bytes, seconds, GB/s.
 *
 * cp2_fill_add_multi adds groups of proved blocks to a fill session: the same pass against the session's own stated roots, then
 * k_multiproof_commit stores what the proved groups leave.
 *   Requests   groups (dataset slot inside the session's range, count), blocks, data and nodes as for cp2_blocks_verify_multi.
 *   Meaning    by the calls that exist.  When every group proves, the call leaves the same session state -- the compact buffer row for
 *              row, the known bitmap, presence and cp2_fill_missing --, the same slot files and the same per-request status as ONE
 *              cp2_fill_add of the same requests, in the same order, with each block's whole path from the true tree.  A group that
 *              fails leaves nothing in the buffer, and every one of its requests gets CP2_FILL_MISMATCH.
 *   Kept       the block roots go to layer 0 always; in a session that keeps nodes (cp2_fill_keep_nodes) the sent rows (stored
 *              canonical) and the computed rows go where the compact layout has them: the rows whole paths would leave and mark known,
 *              the union of the blocks' siblings and ancestors.
 *   Result     status (n x CP2_FILL_*, one per REQUEST) and n_new: NEW / DUPLICATE over the groups' verdicts expanded per request (a
 *              block in two proved groups of one call: the lower index is NEW, the other DUPLICATE), the writer, its roll-back,
 *              CP2_FILL_UNWRITTEN, presence after the sync and the CP2_TRACE line are cp2_fill_add's, one body.
 *
 *   Refused    all or nothing, before any device or file work, CP2_ERR_INVALID with outputs untouched; the group index or the request index,
 *              where there is one, goes into cp2_last_error.  The checks run in this order: (1) a NULL handle or context; (2) a
 *              geometry the tree builders refuse; (3) NULL arrays with n > 0 (block_roots excepted; nodes may be NULL only when n_rows
 *              == 0); (4) a group with count 0; (5) a slot outside the local range, or a root index >= n_roots; (6) a block >= nBlocks;
 *              (7) blocks not strictly ascending inside a group; (8) n_rows different from the sum of the groups' layouts (both
 *              numbers in the message); (9) for the fill, a finished session.  A call whose work table (requests, sent rows and computed nodes) would reach 2^32 - 1 rows is
 *              refused too.  n_groups == 0: CP2_OK.  A context whose stream will not drain is refused (CP2_ERR_HIP).
 * Out of scope: cp2_multi_*; a many-session form; repair with multiproofs; checkpoint formats. */
size_t cp2_block_multiproof_rows(size_t cell_size, size_t block_size, size_t n_cells, const uint64_t* blocks /* k, strictly ascending */,
                                 size_t k);
int cp2_block_multiproof_layout(size_t cell_size, size_t block_size, size_t n_cells, const uint64_t* blocks /* k, strictly ascending */,
                                size_t k, uint64_t* level_index /* rows x 2 */);
int cp2_dataset_block_multiproofs(cp2_dataset* ds, const uint64_t* groups /* n_groups x 2: dataset slot, count */, size_t n_groups,
                                  const uint64_t* blocks /* n */, uint8_t* block_roots /* n x 32, may be NULL */,
                                  uint8_t* nodes /* cap x 32 */, size_t cap, size_t* n_rows);
int cp2_blocks_verify_multi(cp2_ctx* ctx, size_t cell_size, size_t block_size, size_t n_cells, const uint8_t* slot_roots /* n_roots x 32 */,
                            size_t n_roots, const uint64_t* groups /* n_groups x 2: index into slot_roots, count */, size_t n_groups,
                            const uint64_t* blocks /* n */, const uint8_t* data /* n x block_size */,
                            const uint8_t* nodes /* n_rows x 32 */, size_t n_rows, uint32_t* status /* n_groups */,
                            uint8_t* block_roots /* n x 32, may be NULL */);
int cp2_fill_add_multi(void* f /* cp2_fill* */, const uint64_t* groups /* n_groups x 2: dataset slot, count */, size_t n_groups,
                       const uint64_t* blocks /* n */, const uint8_t* data /* n x block_size */, const uint8_t* nodes /* n_rows x 32 */,
                       size_t n_rows, uint32_t* status /* n: CP2_FILL_* */, size_t* n_new);

/* ---- multiproofs against what a fill session knows; tree rows served by place ---------------------------------------------------------
 * cp2_fill_add_multi knows only the stated slot root: a half-filled session that keeps nodes is still sent every sibling up to the root.
 * cp2_fill_add_anchored stops at kept nodes but takes one path per block: two blocks under one unknown subtree send their shared
 * siblings twice.  These calls take the minimum of both: for a set B of blocks, only the rows the session can neither compute from B nor
 * already holds, and peers -- a finished dataset, or a session that is still filling -- serve those rows by their place in the tree.
 *   Format     the geometry of block multiproofs.  known(l, i) is the session's KNOWN bit of node i of level l of the slot; (depth, 0),
 *              the stated slot root, always counts as known.  For a non-empty set B of DISTINCT blocks let A_0 = B.  For l = 0 .. depth
 *              and every i in A_l: when known(l, i), (l, i) is a TOP: the value that reaches it is compared with the kept row (at depth:
 *              the stated root); a top puts nothing into A_{l+1}, and a top of level 0 costs no compression (the fresh block root is
 *              compared).  Otherwise i >> 1 is in A_{l+1}, and when i ^ 1 < m_l the sibling is taken (a) from the call, when i ^ 1 is in
 *              A_l and unknown; (b) from the session's buffer, when known(l, i ^ 1): a KEPT INPUT, never sent, the kept row being used
 *              even when i ^ 1 is a top too; (c) otherwise it is SENT.  The WANT LIST is the sent rows (l, i ^ 1), by level ascending,
 *              then by index ascending: cp2_block_multiproof_layout's order, and its rows when only the root is known.
 *   Verdict    belongs to the GROUP: it proves when every one of its tops matches.  Every leaf lies under a top, the root being known.
 *   Kept       a proved group leaves the block roots of B that were not known, the sent rows (stored canonical) and every computed node
 *              that is not a top, each where the compact layout has it; a row that was known when the call began is never written.
 *              That is what ONE cp2_fill_add_anchored of the same requests leaves, with levels = cp2_fill_anchors' answers and paths
 *              from the true tree.  A slot of nBlocks blocks filled in any grouping receives at most nBlocks - 1 rows in all: a sent
 *              row is the sibling of an unknown node whose parent the call computes, and after the proof both children are known.
 *
 * cp2_fill_multiproof_want: host only, read-only.  groups (dataset slot, count) and blocks as for cp2_fill_add_multi.
 *   Result     *n_rows = the rows of all groups, always the full count; level_index (cap x 2 uint64: level, index) receives them packed
 *              in group order only when cap >= *n_rows; group_rows (n_groups, may be NULL) the count per group.  Every group is laid out
 *              against the session as it stands; groups of one call do not see each other.  A session that keeps no nodes is not
 *              refused: only the root is known, and the answer is cp2_block_multiproof_layout's.
 *   Refused    CP2_ERR_INVALID, outputs untouched, in this order: (1) a NULL session; (2) NULL arrays with requests; (3) a group with
 *              count 0; (4) a slot outside the range; (5) a block >= nBlocks; (6) blocks not strictly ascending; (7) a finished session.
 *
 * cp2_dataset_block_tree_rows, cp2_fill_block_tree_rows serve tree rows by place: places is n x 3 uint64 (dataset slot, level in
 * [0, depth], index < m_level); level depth is the slot root.  One upload of the address list, one gather on the device
 * (cp2_dataset_block_proofs' own), one download.  Read-only.
 *   Dataset    from every node kept or from the compact layers; a roots-only dataset is refused, as in cp2_dataset_block_proofs.
 *   Fill       also status[i] = CP2_FILL_ROW_KNOWN or CP2_FILL_ROW_UNKNOWN; an unknown row comes back as zeros.  With rows == NULL the
 *              statuses come from the host bitmap, with no device work.  A session that keeps no nodes is refused, and so is a
 *              finished one, as in cp2_fill_block_proofs.
 *   Refused    CP2_ERR_INVALID, the request index in cp2_last_error, outputs untouched: NULL arrays with n > 0, a slot outside the
 *              range, a level above depth, an index at or past its layer's size.
 *
 * cp2_fill_add_multi_anchored is cp2_fill_add_multi with nodes = the groups' want lists' rows, packed in group order.
 *   Data path  cp2_blocks_verify's, unchanged.  The work table holds the leaves, the sent rows, the kept inputs (gathered from the
 *              session's buffer by address, once, before the layers) and the computed rows; k_multiproof_layer runs as it is, level by
 *              level; k_multiproof_tops compares every top with its kept row, k_multiproof_fold ORs them into one verdict per group;
 *              k_multiproof_commit stores what the proved groups leave.  The rest is cp2_fill_add's tail.
 *   Result     status (n x CP2_FILL_*, one per REQUEST) and n_new, as cp2_fill_add_multi.  A group of present blocks: all DUPLICATE, 0
 *              rows; an absent block whose root is known: NEW from its bare bytes.
 *   Trace      CP2_TRACE prints cp2_fill_add_multi's line, and before it the number of tops and of kept inputs.
 *   Refused    all or nothing, before any device or file work: cp2_fill_add_multi's checks in their order, where (8) compares n_rows with
 *              the sum of the groups' want lists against the session AS IT STANDS NOW (both numbers in the message: a list made
 *              before another add landed is stale and shows here); then a session that keeps no nodes (it uses cp2_fill_add_multi).
 * Out of scope: cp2_multi_*; a many-session form; cp2_blocks_verify_multi against known nodes the caller supplies; repair with
 * multiproofs; checkpoint formats. */
enum { CP2_FILL_ROW_KNOWN = (0), CP2_FILL_ROW_UNKNOWN = (1) };   /* (an enum: the macros named CP2_FILL_* stay the statuses of the adds and of the proofs) */
int cp2_fill_multiproof_want(const void* f /* cp2_fill* */, const uint64_t* groups /* n_groups x 2: dataset slot, count */, size_t n_groups,
                             const uint64_t* blocks /* n */, uint64_t* level_index /* cap x 2 */, size_t cap, size_t* n_rows,
                             uint64_t* group_rows /* n_groups, may be NULL */);
int cp2_dataset_block_tree_rows(cp2_dataset* ds, const uint64_t* places /* n x 3: dataset slot, level, index */, size_t n,
                                uint8_t* rows /* n x 32 */);
int cp2_fill_block_tree_rows(void* f /* cp2_fill* */, const uint64_t* places /* n x 3: dataset slot, level, index */, size_t n,
                             uint32_t* status /* n: CP2_FILL_ROW_* */, uint8_t* rows /* n x 32, may be NULL */);
int cp2_fill_add_multi_anchored(void* f /* cp2_fill* */, const uint64_t* groups /* n_groups x 2: dataset slot, count */, size_t n_groups,
                                const uint64_t* blocks /* n */, const uint8_t* data /* n x block_size */,
                                const uint8_t* nodes /* n_rows x 32 */, size_t n_rows, uint32_t* status /* n: CP2_FILL_* */, size_t* n_new);


/* ---- e: every GPU of the node behind one handle ------------------------------------------------------ */
/* `generateProofInput` hashes every slot of the dataset before it proves one (reference/nim/proof_input/src/gen_input/
 * bn254.nim:41-42), and slots are independent until the dataset tree (:49-51).  A cp2_multi holds one context per device;
 * a dataset built through it is cut into contiguous slot ranges (cp2_shard_range: the first n mod world ranges hold one
 * slot more), each device builds its range on its own host thread with no communication, then ONE exchange -- an all-gather
 * of the 32-byte slot roots, device to device (RCCL over xGMI: in-place ncclAllGather on every context's stream) -- and
 * every device builds the identical dataset tree and serves the proof inputs of its own slots.  One process, no launcher:
 * the caller makes the same calls on a one-GPU and on an eight-GPU node.
 *   - librccl is opened at run time, and only when at least two distinct devices hold a shard.  Without it, or when a device
 *     index repeats (two contexts on one device), the roots are gathered through host memory instead (1 MiB at 32 768 slots);
 *     cp2_multi_gather_mode names what the last build did ("rccl (...)", "host (<why>)", "copy (...)", "none (one shard ...)").
 *   - The exchange is VERIFIED, whatever carried it: every device must find its own slot roots at its own rows of the list it
 *     received, and all devices must compute the same dataset root (one 32-byte-per-slot download per shard) -- a wrong
 *     rank-to-device mapping or a misplaced block is CP2_ERR_HIP ("exchange verification failed ..."), never a wrong
 *     dataSetRoot.  It is also BOUNDED: communicator creation and the collective itself are given CODEX_P2_EXCHANGE_TIMEOUT_S
 *     seconds (default 120); one that does not return is an error that says so (its buffers are abandoned, RCCL is not used again
 *     in this process).  In the automatic mode a device path that fails either way is retried once through host memory, and
 *     cp2_multi_gather_mode says that it was; a way asked for by name is never replaced.
 *   - Small datasets use fewer devices: a device gets a shard only when there is at least `min_cells_per_device` cells of
 *     hashing for it (default: one residency of the hash kernel, 768 x 256 cells -- a device with less finishes no sooner),
 *     so the reference's default run (11 slots x 512 cells, workflow/params.sh) stays on one GPU and pays one context.
 *   - Contexts are created on first use; cp2_multi_ctx(m, i) hands one out for the seam calls and the tuning knobs.
 *   - One handle per host thread (like a context): calls on one cp2_multi / cp2_multi_dataset are not to be made concurrently;
 *     the library starts and joins its per-device threads inside each call.
 *   - Datasets of FEW, LARGE slots are cut BY UNITS instead of by whole slots: when whole slots would leave the busiest device
 *     more than 6 % above its share (11 slots on 8 GPUs: 2 against 1.375; ONE 128 GiB slot on 8 GPUs), every slot is cut into
 *     S = 2^s units of nCells / S cells (cp2_slot_trees_build_*_units), the nSlots x S units are dealt out contiguously, the
 *     unit roots exchanged, and the log2 S upper layers of every slot tree plus the dataset tree built once; a proof input then
 *     takes the bottom of each path from whichever device holds the sampled cell; many proof inputs at once
 *     (cp2_multi_dataset_export_proof_inputs) take ONE batched gather per device, the devices in parallel.  Every kind of build
 *     follows this plan.  A STREAMED build cut by units is two-phase -- sampling needs the slot root, which exists only after the
 *     exchange of unit roots, so nothing of a proof input can be made while later units hash: the balanced unit build, the
 *     exchange, then every slot's input.json from the devices that hold its units, kept as text for _export_streamed /
 *     _streamed_json.  cp2_multi_set_split / CODEX_P2_SPLIT override (1 = whole slots only: the overlapped per-slot pipeline). */
typedef struct cp2_multi cp2_multi;
typedef struct cp2_multi_dataset cp2_multi_dataset;
enum { CP2_GATHER_AUTO = 0, CP2_GATHER_RCCL = 1, CP2_GATHER_HOST = 2, CP2_GATHER_COPY = 3 };
/* devices: n_dev HIP device indices (an index may repeat: several contexts on one device).  n_dev = 0: the environment
 * variable CODEX_P2_GPUS ("all" = every visible gfx950 device, "<count>" = the first <count> visible devices, or a
 * comma-separated index list), else ONE device: the first visible gfx950.  Several devices are OPT-IN -- by the variable or by
 * an explicit list -- until the exchange between two real devices has a committed record (this pipeline's GPU boxes hold one
 * device).  Every CODEX_P2_* variable is checked here (cp2_check_environment): a value that is not what
 * its variable takes is CP2_ERR_INVALID, not guessed at. */
int cp2_multi_init(const int* devices, int n_dev, cp2_multi** out);
/* frees the handle, its contexts and communicators: free every cp2_multi_dataset (and proof input) made through it first */
void cp2_multi_free(cp2_multi* m);
int cp2_multi_count(const cp2_multi* m);
int cp2_multi_device(const cp2_multi* m, int i);          /* HIP device index of entry i, -1 out of range */
cp2_ctx* cp2_multi_ctx(cp2_multi* m, int i);              /* NULL when the device is unusable            */
const char* cp2_multi_last_error(const cp2_multi* m);
const char* cp2_multi_gather_mode(const cp2_multi* m);
/* gather: CP2_GATHER_AUTO (RCCL when possible, else host), CP2_GATHER_RCCL (fail with CP2_ERR_INVALID when impossible),
 * CP2_GATHER_HOST, CP2_GATHER_COPY (the all-gather written out as device-to-device copies, hipMemcpyPeerAsync pair by pair,
 * through the RCCL path's own buffers, padded layout and compaction: no library, any mix of devices, repeated ones included);
 * cp2_multi_init reads the environment variable CODEX_P2_GATHER ("rccl" / "host" / "copy") as the initial value.  min_cells_per_device: 0 = the default above (or the environment variable CODEX_P2_MIN_CELLS, read by
 * cp2_multi_init); 1 = always spread over every device. */
int cp2_multi_set_policy(cp2_multi* m, int gather, uint64_t min_cells_per_device);
/* units per slot for cp2_multi_dataset_build: 0 = choose (above; or the environment variable CODEX_P2_SPLIT), 1 = whole slots
 * only, a power of two = exactly that many (ignored where the geometry does not allow it: units are >= 2 whole blocks). */
int cp2_multi_set_split(cp2_multi* m, int64_t units_per_slot);
/* the split rule: contiguous ranges, the first (n_items mod world) ranks hold one item more */
void cp2_shard_range(uint64_t n_items, int rank, int world, uint64_t* first, uint64_t* count);
/* The plan cp2_multi_dataset_build follows for `cfg` on `n_devices` devices (host-only arithmetic, no GPU needed): how many of
 * them get a shard and into how many units every slot is cut (1: whole slots).  min_cells_per_device / units_per_slot as for
 * cp2_multi_set_policy / cp2_multi_set_split (0 = the defaults). */
int cp2_multi_plan(const cp2_config* cfg, int n_devices, uint64_t min_cells_per_device, int64_t units_per_slot, int* n_shards,
                   uint64_t* units_per_slot_out);
/* cp2_dataset_build / _build_cached / _build_streamed for ALL cfg->n_slots slots over the devices of `m`, including the
 * exchange (verified and bounded, above) and the dataset tree on every device.  Cached: shard i of n uses "<cache_path>.shard<i>of<n>" (one shard: the path
 * itself; cut by S units per slot: "<cache_path>.units<S>.shard<i>of<n>", the unit trees of that shard).  Streamed: `threads` formatting threads in total, divided over the shards. */
int cp2_multi_dataset_build(cp2_multi* m, const cp2_config* cfg, cp2_multi_dataset** out);
int cp2_multi_dataset_build_cached(cp2_multi* m, const cp2_config* cfg, const char* cache_path, cp2_multi_dataset** out);
int cp2_multi_dataset_build_streamed(cp2_multi* m, const cp2_config* cfg, const uint8_t entropy[32], int threads, size_t group_slots,
                                     cp2_multi_dataset** out);
void cp2_multi_dataset_free(cp2_multi_dataset* mds);
int cp2_multi_dataset_shards(const cp2_multi_dataset* mds);
/* 1 when the dataset is cut by whole slots, else the number of units every slot was cut into */
uint64_t cp2_multi_dataset_units_per_slot(const cp2_multi_dataset* mds);
/* shard i: device index and its range of slots (or of units); by whole slots also its dataset (owned by mds; every
 * single-dataset call works on it), by units NULL */
cp2_dataset* cp2_multi_dataset_shard(cp2_multi_dataset* mds, int i, int* device, uint64_t* first, uint64_t* count);
int cp2_multi_dataset_root(cp2_multi_dataset* mds, uint8_t out[32]);
int cp2_multi_dataset_slot_roots(cp2_multi_dataset* mds, uint8_t* out /* n_slots x 32 */);
/* replaces `generateProofInputBN254`, gen_input/bn254.nim:35-79, on whichever device holds `slot_idx` */
int cp2_multi_proof_input_generate(cp2_multi_dataset* mds, uint64_t slot_idx, const uint8_t entropy[32], cp2_proof_input** out);
/* cp2_dataset_export_proof_inputs / _export_streamed / _streamed_json over all shards (every device works through its own
 * slots concurrently; `threads` host threads in total) */
int cp2_multi_dataset_export_proof_inputs(cp2_multi_dataset* mds, const uint64_t* slot_idx, size_t n, const uint8_t entropy[32],
                                          const char* dir, int threads, size_t batch, uint64_t* total_bytes);
int cp2_multi_dataset_export_streamed(cp2_multi_dataset* mds, const char* dir, int threads, uint64_t* total_bytes);
int cp2_multi_dataset_streamed_json(cp2_multi_dataset* mds, uint64_t slot_idx, char** text, size_t* len);
/* cp2_dataset_scrub over the shards: any range of the dataset's n_slots slots, each shard's part on its own host thread and context,
 * nothing exchanged between devices; the reports merged in slot order.  Cut by units, the comparison is on the cells of every unit
 * and the indices are cells of the SLOT (not of the unit).  Cut by slots, the granularity is the finest level every shard keeps. */
int cp2_multi_dataset_scrub(cp2_multi_dataset* mds, uint64_t first_slot, uint64_t n_slots, uint64_t* bad, size_t cap, size_t* n_bad,
                            int* granularity);

/* cp2_dataset_repair_blocks over the shards: slots of the whole dataset (0 .. n_slots - 1); each request goes to the shard that holds
 * its block (cut by units: the unit holding the block), each shard checks its candidates on its own host thread and context, and the
 * statuses come back in request order.  The matched blocks are written once all shards have checked (units of one slot share its file:
 * one sync per file), and only then is every shard's cache restamped under the names cp2_multi_dataset_build_cached gives them
 * ("<cache_path>.shardIofW", "<cache_path>.unitsS.shardIofW"; one shard: <cache_path> and <cache_path>.kept). */
int cp2_multi_dataset_repair_blocks(cp2_multi_dataset* mds, const uint64_t* slot_block, const uint8_t* data, size_t n, int flags,
                                    const char* cache_path, uint32_t* status, size_t* n_written);
#ifdef __cplusplus
}
#endif
#endif /* CODEX_P2_H */
