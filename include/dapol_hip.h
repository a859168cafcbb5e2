/* dapol_hip.h -- C ABI of the MI355X-native DAPOL+ proving path (libdapol_hip.so).
 *
 * The reference crate (MystenLabs/dapol, Rust) exposes no FFI; its seams are Rust traits and generic
 * parameters.  Each entry point below names the reference interface it replaces (paths relative to the
 * reference root).  A Rust maintainer binds these with an `extern "C"` block (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - every function returns an int32 status (DAPOL_OK == 0); nothing aborts or throws across the boundary;
 *  - all pointers are caller-owned HOST pointers unless the parameter name ends in `_dev` (device pointers,
 *    for callers that already keep their arrays in HBM);
 *  - byte strings are little-endian, 32-byte scalars / compressed ristretto255 points as in curve25519-dalek;
 *  - a dapol_ctx is bound to one GPU and one HIP stream; use one ctx per host thread / GPU.
 *
 * Randomness ("tape") contract: the reference draws from thread_rng() (src/dapol/node.rs:87 and inside
 * bulletproofs' prover), so its outputs differ run to run.  Here every draw is an explicit input:
 *  - a WIDE draw is 64 bytes reduced mod l (== Scalar::random);
 *  - seed mode: draw(domain, a, b) = first 64-byte XOF block of BLAKE3-keyed(seed, LE32 domain|LE64 a|LE64 b);
 *    padding node at (level above leaves, index): domain 1, a = level, b = index;
 *    range-proof nonce: domain 2, a = stream id (the leaf's tree index), b = slot, under a key bound to the STATEMENT:
 *    k1 = draw(seed; 6, stream id, first slot of the proof)[:32], k2 = draw(k1; 7, n_bits, m)[:32], then for every group
 *    of 31 value commitments k = BLAKE3(k | V_g .. V_g+30); the nonces are draw(k; 2, stream id, slot).  The crate draws
 *    fresh thread_rng randomness per call; a deterministic stream that ignored the statement would reuse a_blinding,
 *    s_L, s_R, tau against new challenges whenever a leaf is proved again after its siblings changed (dapol_tree_update,
 *    another policy / aggregation factor) and leak them.  Same statement => same nonces => same proof bytes;
 *  - slot order of one aggregated proof with m parties of n bits (the crate's draw order): party j draws
 *    a_blinding = j(2n+2), s_blinding = j(2n+2)+1, s_L[i] = j(2n+2)+2+i, s_R[i] = j(2n+2)+2+n+i; then
 *    t1_blinding_j = m(2n+2)+2j, t2_blinding_j = m(2n+2)+2j+1.   m(2n+4) slots in total;
 *  - tape mode: the same slots read from a caller buffer of 64-byte draws.
 */
#ifndef DAPOL_HIP_H
#define DAPOL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes.  1-5 mirror DapolError (src/errors.rs:6-17); 6-7 mirror smtree DecodingError as used by
 * src/range/mod.rs:124-161 and src/proof/node.rs:81-102. */
enum {
    DAPOL_OK = 0,
    DAPOL_ERR_TREE_HEIGHT_TOO_BIG = 1,   /* DapolError::TreeHeightTooBig   (src/dapol/mod.rs:104-109) */
    DAPOL_ERR_SPARSITY_TOO_SMALL = 2,    /* DapolError::SparsityTooSmall   (src/dapol/mod.rs:110-116) */
    DAPOL_ERR_INVALID_DIGEST_SIZE = 3,   /* DapolError::InvalidDigestSize  (src/dapol/mod.rs:101-103) */
    DAPOL_ERR_DUPLICATED_INTERNAL_ID = 4,/* DapolError::DuplicatedInternalId (src/dapol/mod.rs:341-343) */
    DAPOL_ERR_FAILED_TO_MAP_INDEX = 5,   /* DapolError::FailedToMapIndex   (src/dapol/mod.rs:369-370) */
    DAPOL_ERR_BYTES_NOT_ENOUGH = 6,      /* DecodingError::BytesNotEnough */
    DAPOL_ERR_VALUE_DECODING = 7,        /* DecodingError::ValueDecodingError */
    DAPOL_ERR_INVALID_ARGUMENT = 8,      /* where the reference panics: unsorted/duplicate leaves (smtree build),
                                            aggregation_factor > #siblings (src/range/padding.rs:95-98), bad n/m
                                            (bulletproofs InvalidBitsize / InvalidAggregation) */
    DAPOL_ERR_UNKNOWN_LEAF = 9,          /* the `None` of Dapol::generate_proof* (src/dapol/mod.rs:148-190) */
    DAPOL_ERR_NO_DEVICE = 16,            /* no usable HIP device: the product path never falls back to the CPU */
    DAPOL_ERR_HIP = 17,                  /* a HIP runtime call failed; see dapol_last_error() */
    DAPOL_ERR_OUT_OF_MEMORY = 18,
    DAPOL_ERR_COMM = 19                  /* an RCCL call failed; see dapol_last_error() */
};

typedef struct dapol_ctx dapol_ctx;
typedef struct dapol_tree dapol_tree;

enum { DAPOL_POLICY_PADDING = 0, DAPOL_POLICY_SPLITTING = 1 };  /* RangeProofPadding / RangeProofSplitting */
/* D = blake3::Hasher (benches/dapol.rs:38), blake2::Blake2s (src/dapol/tests.rs:21), or blake2::Blake2b (src/tests.rs:100-101: the
 * reference's integration test also runs Dapol<Blake2b, R> through new_blank + build + prove + serialize + verify; only Dapol::new
 * rejects a digest that is not 32 bytes, src/dapol/mod.rs:101-103).  With DAPOL_DIGEST_BLAKE2B every node hash is 64 bytes: every
 * `H` buffer of this header -- whatever its parameter is called (H32, H_out32, path_H32 ...) -- then holds dapol_ctx_digest_bytes()
 * = 64 bytes per node instead of 32.  The Blake2b context serves the new_blank + build path: dapol_tree_build (enforce_sparsity = 0),
 * dapol_tree_update, roots / levels / paths, dapol_prove_entities, dapol_prove_batch, the wire format (*_d forms below),
 * dapol_verify_entities / dapol_verify_batch, dapol_merge_batch, dapol_padding_nodes, dapol_commit_hash_batch.  What the reference
 * refuses for such a digest is refused here with DAPOL_ERR_INVALID_DIGEST_SIZE: Dapol::new (dapol_tree_build with enforce_sparsity,
 * dapol_build_leaf_nodes); so are the paths that exist only for the benchmark and for multi-GPU sharding (workloads, shard trees,
 * the communicator, node records), whose records carry 32-byte hashes.
 * D = sha2::Sha256 (DAPOL_DIGEST_SHA256) and D = sha3::Sha3_256 (DAPOL_DIGEST_SHA3_256), the other two hash crates of the reference's
 * manifest: 32-byte digests, so every path of a BLAKE3 context works with them unchanged, sharding, workloads, records, the wire
 * format, the shared prover / re-prover / proof store / shared verifier and Dapol::new's leaf derivation included.
 * Id 3 is reserved and refused like every other value. */
enum { DAPOL_DIGEST_BLAKE3 = 0, DAPOL_DIGEST_BLAKE2S = 1, DAPOL_DIGEST_BLAKE2B = 2, /* 3: reserved */ DAPOL_DIGEST_SHA256 = 4, DAPOL_DIGEST_SHA3_256 = 5 };

/* Replaces the per-call PedersenGens::default() (src/dapol/node.rs:31, src/range/mod.rs:49,65,84,103) and
 * BulletproofGens::new(64, m) (src/range/mod.rs:50,66,85,104): generators and their window tables are derived
 * ONCE, on the GPU, for up to max_parties parties of 64 bits.  max_parties must be a power of two <= 1024.
 * digest_id: the node hash D of Dapol<D, R> used by every tree / merge / verify call of this context; anything but the
 * five digests above (3 included: reserved) -> DAPOL_ERR_INVALID_DIGEST_SIZE. */
int32_t dapol_ctx_create(int32_t device, int32_t max_parties, int32_t digest_id, dapol_ctx** out);
int32_t dapol_ctx_digest_bytes(dapol_ctx* ctx, int32_t* bytes);          /* D::output_size(): 32 or 64 -- the size of every node hash of this context */
/* Settings of a context.  Every field: 0 = the library's own choice (what a plain dapol_ctx_create gives).  The first three are
 * fixed at creation (dapol_ctx_create_opts), the others may be changed at any time between calls (dapol_ctx_set_options).
 * None of them changes a byte of any output (tests/test_gpu_parity.py::test_every_proving_strategy_gives_the_same_bytes); they
 * trade memory against speed or pick among equivalent schedules.
 * The DAPOL_* ENVIRONMENT variables the sources mention are measurement knobs: they are read ONLY when the process has opted in
 * (DAPOL_ENV_KNOBS=1 in the environment, or dapol_env_knobs(1)) -- a host embedding this library does not inherit behaviour from
 * stray variables.  When enabled, a variable overrides the corresponding field. */
typedef struct {
    int32_t struct_size;              /* = sizeof(dapol_options): lets the struct grow */
    int32_t window_bits;              /* creation: width of the fixed-base windows, 8..20 (0: widest <= 17 whose tables fit table_gb) */
    double  table_gb;                 /* creation: budget of the window tables in GB (0: 40 GB, at most 30 % of the free memory) */
    int32_t high_half_rows;           /* creation: 0 auto, 1 on, -1 off: second table row per generator (halves the window steps of lanes that cannot share doublings) */
    int32_t generator_stationary;     /* 0 auto (calls of at least 1,024 proofs over >= 1,024 generators a side that are not small calls; batches of shorter proofs --
                                         a policy's individual proofs, 2 ... 8 parties -- from 2,048 / 1,024 / 512 proofs at 64 / 128 / 256-512 generators a side),
                                         1 every call that is not a small one, -1 never */
    int32_t gs_tile_rows;             /* rows per launch of the generator-stationary sweep (multiple of 4; 0: 16) */
    int32_t streams;                  /* chunks in flight, 1..4 (0: 1 -- one chunk of two rounds of resident wavefronts; more only share the chip) */
    int64_t chunk_proofs;             /* proofs per chunk (0: whole rounds of resident wavefronts, 65,536 on MI355X) */
    double  scratch_gb;               /* scratch budget of the range prover / verifier in GB (0: 130 GB, at most what is free beyond 8 GB) */
    int32_t tail_length;              /* length T of the hybrid inner-product argument's tail: 32 / 64 / 128 / 256, -1 = no tail (0: 64; swept batches of short
                                         proofs: 32 at 512 generators a side, none below) */
    int32_t small_call_max;           /* calls of up to this many proofs take the latency shapes.  0: 1,023 for proofs of >= 1,024 generators a side (the sweep
                                         takes over at 1,024 proofs unless generator_stationary = -1), 8,191 for smaller proofs -- where the short-list sweep
                                         takes over earlier (see generator_stationary; it yields only to generator_stationary = -1).  An explicit value is
                                         taken as it is for proofs of >= 1,024 generators a side */
    int32_t verify_batch_min;         /* fewest proofs the verifier checks as ONE random linear combination (0: 112) */
    int64_t update_incremental_max;   /* dapol_tree_update / dapol_tree_remove: most leaves replaced, inserted or removed in place, and never more
                                         than an eighth of the tree's leaves (0: 65,536; -1: always rebuild) */
    int32_t gs_slices;                /* slices of a list swept side by side by the generator-stationary MSM: 1, 2, 4, 8, 16 (0: as many as fill the chip) */
    int32_t profile;                  /* creation: DAPOL_PROFILE_BENCH (0, the default) or DAPOL_PROFILE_HOST: the defaults of the memory fields above.
                                         BENCH spends HBM for the last percent of throughput: 17-bit windows + high-half rows (69 GB of tables for 32
                                         parties), chunks of two rounds of resident wavefronts (102 GB of scratch during a large call).  HOST is sized for
                                         an embedder that shares the GPU: 18 GB table budget (16-bit windows for 32 parties, no high-half rows), chunks of
                                         one round (<= 56 GB of scratch) -- INTEGRATION.md section 4 gives both footprints and throughputs.  Explicit
                                         table_gb / window_bits / high_half_rows / scratch_gb / chunk_proofs win over the profile. */
} dapol_options;
enum { DAPOL_PROFILE_BENCH = 0, DAPOL_PROFILE_HOST = 1 };
int32_t dapol_ctx_create_opts(int32_t device, int32_t max_parties, int32_t digest_id, const dapol_options* options, dapol_ctx** out);
int32_t dapol_ctx_get_options(dapol_ctx* ctx, dapol_options* out);      /* the stored settings (zeros = defaults) + window_bits / high_half_rows as built */
int32_t dapol_ctx_set_options(dapol_ctx* ctx, const dapol_options* options);   /* creation-time fields are ignored here */
int32_t dapol_env_knobs(int32_t enable);                                 /* process-wide opt-in to the DAPOL_* measurement knobs; returns the old setting */
/* Trees and workloads built on a context keep it alive: dapol_ctx_destroy releases the caller's handle, the storage goes
 * when the last tree / workload of the context is destroyed too -- handles may be destroyed in any order. */
int32_t dapol_ctx_destroy(dapol_ctx* ctx);
/* Compressed generators (for cross-checks): which = 0 B, 1 B_blinding, 2 G[party][bit], 3 H[party][bit]. */
int32_t dapol_ctx_generator(dapol_ctx* ctx, int32_t which, int32_t party, int32_t bit, uint8_t out32[32]);
const char* dapol_strerror(int32_t code);
const char* dapol_last_error(void);
/* Diagnostics: how many times a call was left between a fork onto one of the context's side streams and the matching join (an error
 * return) and therefore waited for that stream before returning, process-wide.  0 in a healthy run. */
int32_t dapol_diag_fork_guard_waits(uint64_t* count);
/* Diagnostics: combined (random-linear-combination) checks of dapol_range_verify_batch / dapol_verify_* that failed and went on to
 * bisection or the proof-by-proof check, process-wide.  Stays 0 while every proof handed in is valid. */
int32_t dapol_diag_verify_fallbacks(uint64_t* count);
/* Diagnostics: device milliseconds of the proving pipeline of the last dapol_range_prove_batch in this process (HIP events on the
 * context's stream: inputs already in HBM, proofs not yet copied back). */
int32_t dapol_diag_range_prove_ms(double* ms);

/* DapolNode::new (src/dapol/node.rs:29-45), batched: C_i = v_i*B + r_i*B_blinding (compressed), H_i = D(C_i).
 * r may be an unreduced Scalar::from_bits value (bit 255 clear; src/dapol/mod.rs:385). */
int32_t dapol_commit_hash_batch(dapol_ctx* ctx, size_t n, const uint64_t* v, const uint8_t* r32, uint8_t* C_out32,
                                uint8_t* H_out32);

/* build_leaf_nodes + shuffle_index (src/dapol/mod.rs:323-441), the leaf half of Dapol::new: liabilities in INPUT order
 * (ids as concatenated bytes with n+1 offsets) -> for every liability its tree index and blinding factor, returned both
 * per input entity (idx_by_entity, may be NULL = the id_to_idx_map of mod.rs:388) and sorted by index, ready for
 * dapol_tree_build (mod.rs:396): leaf_idx_sorted / v_sorted / r32_sorted, with order_sorted[p] = input position of the
 * p-th leaf.  digest_id: DAPOL_DIGEST_BLAKE3, DAPOL_DIGEST_BLAKE2S (the digest of the reference's known-answer tests,
 * src/dapol/tests.rs:13,21), DAPOL_DIGEST_SHA256 or DAPOL_DIGEST_SHA3_256; ids of any length, as in the reference (mod.rs:347-349, 358-360) -- BLAKE3 inputs beyond one
 * 1024-byte chunk go through the tree mode on the device.  Collisions are resolved exactly as the
 * reference does (an entity competes only with the entities before it in the input; up to 128 re-hashes).
 * Errors: DAPOL_ERR_TREE_HEIGHT_TOO_BIG, DAPOL_ERR_SPARSITY_TOO_SMALL (2^height < 2n), DAPOL_ERR_DUPLICATED_INTERNAL_ID,
 * DAPOL_ERR_FAILED_TO_MAP_INDEX. */
int32_t dapol_build_leaf_nodes(dapol_ctx* ctx, int32_t digest_id, const uint8_t* audit_seed, size_t audit_seed_len, int32_t height,
                               size_t n, const uint8_t* internal_ids, const uint32_t* internal_off, const uint8_t* external_ids,
                               const uint32_t* external_off, const uint64_t* values, uint64_t* leaf_idx_sorted, uint64_t* v_sorted,
                               uint8_t* r32_sorted, uint32_t* order_sorted, uint64_t* idx_by_entity);

/* Dapol::new_blank + Dapol::build (src/dapol/mod.rs:196-208 -> smtree SparseMerkleTree::build) with the leaf
 * nodes made by DapolNode::new; also the build half of Dapol::new (src/dapol/mod.rs:100-128).
 * leaf_idx must be strictly increasing and < 2^height (the reference panics otherwise -> INVALID_ARGUMENT);
 * enforce_sparsity != 0 applies the 2^height >= 2n check of Dapol::new.  Padding nodes (node.rs:86-88) take
 * their blinding from pad_seed32 (seed mode, positional). */
int32_t dapol_tree_build(dapol_ctx* ctx, int32_t height, size_t n, const uint64_t* leaf_idx, const uint64_t* v,
                         const uint8_t* r32, const uint8_t pad_seed32[32], int32_t enforce_sparsity, dapol_tree** out);
/* TAPE mode of the build (the randomness contract in this header's head comment): the padding nodes' blindings are read from
 * `tape` -- tape_draws x 64 bytes, each reduced mod l like Scalar::random, ONE PER PADDING NODE in the order (level bottom-up, index
 * ascending) -- instead of being derived from a seed.  dapol_tree_padding_positions (host only, pure index arithmetic) gives that
 * order and the count for a leaf set: *count, and, when non-NULL, level[] (0 = leaf level) and index[] of every padding node.  With
 * the draws a seed would have given, the tree equals dapol_tree_build's bit for bit.  A tape shorter than the tree's padding nodes ->
 * DAPOL_ERR_INVALID_ARGUMENT.  A tree built from a tape cannot be updated (no seed to draw new padding nodes from). */
int32_t dapol_tree_padding_positions(int32_t height, size_t n, const uint64_t* leaf_idx, size_t* count, uint8_t* level, uint64_t* index);
int32_t dapol_tree_build_tape(dapol_ctx* ctx, int32_t height, size_t n, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32,
                              const uint8_t* tape, size_t tape_draws, dapol_tree** out);
/* Multi-GPU sharding: builds only the subtree that holds all the given leaves, i.e. the
 * lowest (total_height - shard_bits) levels; every leaf index (GLOBAL, < 2^total_height) must share its top
 * shard_bits bits.  Padding seeds and nonce stream ids use the global indexes, so the nodes equal the ones a
 * single-GPU build of the whole tree produces.  dapol_tree_root then returns the subtree root. */
int32_t dapol_tree_build_shard(dapol_ctx* ctx, int32_t total_height, int32_t shard_bits, size_t n, const uint64_t* leaf_idx,
                               const uint64_t* v, const uint8_t* r32, const uint8_t pad_seed32[32], dapol_tree** out);
/* Paddable::padding (src/dapol/node.rs:86-88), batched: the padding node new(0, blinding) at (level above the leaves,
 * index within that level), its blinding drawn positionally from pad_seed (domain 1 of the randomness contract) -- the
 * very node dapol_tree_build puts there.  Value is 0.  Used e.g. as the record of an empty shard in a multi-GPU build. */
int32_t dapol_padding_nodes(dapol_ctx* ctx, const uint8_t pad_seed32[32], size_t n, const uint8_t* level, const uint64_t* index,
                            uint8_t* C32, uint8_t* H32, uint8_t* r32);
/* Mergeable::merge (src/dapol/node.rs:64-80; the (C,H) half is DapolProofNode::merge, src/proof/node.rs:56-69),
 * batched on compressed inputs: parent[i] = merge(left[i], right[i]).  Used for the replicated top levels above
 * the shard roots and by the Merkle-path re-merge of verification.  v/r pointers may all be NULL ((C,H) only).
 * A commitment that does not decode -> DAPOL_ERR_VALUE_DECODING. */
int32_t dapol_merge_batch(dapol_ctx* ctx, size_t n, const uint8_t* CL32, const uint8_t* HL32, const uint64_t* vL, const uint8_t* rL32,
                          const uint8_t* CR32, const uint8_t* HR32, const uint64_t* vR, const uint8_t* rR32, uint8_t* C32,
                          uint8_t* H32, uint64_t* v, uint8_t* r32);
int32_t dapol_tree_destroy(dapol_tree* tree);
/* Dapol::update (src/dapol/mod.rs:211-213 -> SparseMerkleTree::update), batched: the k leaves are applied in input
 * order -- a leaf is inserted, or replaces the liability already at its index (the last of several updates of one
 * index wins).  Afterwards the tree equals dapol_tree_build of the resulting leaf set bit for bit (padding nodes
 * are keyed by position, so the reference test's build-vs-update root equality, src/tests.rs:48, holds exactly).
 * Only for trees from dapol_tree_build / dapol_tree_build_shard.  An error reported before anything was written (bad arguments,
 * an index outside the tree or the shard, an allocation that failed) leaves the tree unchanged.  Small batches are re-merged IN
 * PLACE on the device; a HIP failure between the first and the last write of such an update leaves upper levels that no longer
 * match the leaves: the tree is then marked invalid and every later call on it returns DAPOL_ERR_INVALID_ARGUMENT ("left
 * inconsistent ...") -- destroy it and build it again.  The same holds for a batch that mixes new and existing indexes once its
 * inserts have been applied: whatever stops the replacements after that -- also an error before THEIR first write -- would leave a
 * consistent but half-updated tree, so the tree is marked invalid too (never "unchanged" with half the batch in).
 * On a context with a 64-byte digest the whole hash chain is laid again after the update; a tree built from a padding tape
 * (dapol_tree_build_tape) cannot be updated. */
int32_t dapol_tree_update(dapol_tree* tree, size_t k, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32);
/* Removes the k leaves at leaf_idx (in any order; a duplicate removes its leaf once; k = 0 does nothing).  Surviving leaves keep their
 * indexes, and afterwards the tree equals dapol_tree_build (dapol_tree_build_shard) over the remaining leaves with the tree's pad
 * seed bit for bit, at every level.  All or nothing: an index that is not a leaf of the tree (also one outside the tree or outside a
 * shard's prefix) -> DAPOL_ERR_UNKNOWN_LEAF, a batch that holds every leaf -> DAPOL_ERR_INVALID_ARGUMENT, both with the tree
 * unchanged.  Refused like dapol_tree_update: trees built from a padding tape, workload trees, trees marked invalid.  Batches within
 * update_incremental_max (dapol_options) and at most an eighth of the leaves are removed IN PLACE on the device; a HIP failure
 * between the first and the last write of such a removal marks the tree invalid, as for dapol_tree_update.  Larger batches rebuild
 * the tree from the surviving leaves (an error then leaves the old tree as it was). */
int32_t dapol_tree_remove(dapol_tree* tree, size_t k, const uint64_t* leaf_idx);
/* Adds k NEW leaves, given in any order (k = 0 does nothing); the counterpart of dapol_tree_remove.  All or nothing.  Afterwards the
 * tree equals dapol_tree_build (dapol_tree_build_shard) over (old leaves + new leaves) with the tree's pad seed bit for bit, at every
 * level -- node counts, padding records and parent pointers included -- whichever path ran.  A leaf keeps its blinding as given
 * (bit 255 cleared, possibly >= l); parents hold the reduced sums.  An index that is a leaf already, or that occurs twice in the batch
 * -> DAPOL_ERR_INVALID_ARGUMENT with nothing written and the tree usable (dapol_last_error says which); an index outside the tree or
 * outside a shard's prefix is refused with dapol_tree_update's code for the same batch, the tree unchanged.  Refused like
 * dapol_tree_update: trees built from a padding tape, workload trees, trees marked invalid.  Batches within update_incremental_max
 * (dapol_options) and at most an eighth of the leaves go IN PLACE on the device, whatever nodes their chains share (a sibling pair, a
 * whole new subtree): the levels that gain nodes are rewritten in order and only the new nodes and the ancestors of the new leaves
 * are merged.  A HIP failure between the first and the last write of such an insert marks the tree invalid, as for
 * dapol_tree_update.  Larger batches rebuild the tree (an error then leaves the old tree as it was).  dapol_tree_update keeps
 * rebuilding for new leaves whose chains share a node; a caller that only ADDS leaves should call this instead. */
int32_t dapol_tree_insert(dapol_tree* tree, size_t k, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32);
/* build_leaf_nodes for k liabilities that JOIN a built tree (ids and values as for dapol_build_leaf_nodes; the height is the tree's):
 * shuffle_index (src/dapol/mod.rs:408-441) with tree_index_set starting as the tree's current leaf indexes -- candidate c of
 * liability j is taken when it is a leaf of `tree` now, or held by a liability j' < j of this batch.  Writes nothing to the tree.
 * Outputs as dapol_build_leaf_nodes: sorted by index (leaf_idx_sorted / v_sorted / r32_sorted / order_sorted, positions within the
 * batch) and idx_by_entity (may be NULL).  With the tree made from dapol_build_leaf_nodes(L) and nothing removed since, the rows are
 * those of the new liabilities in dapol_build_leaf_nodes(L ++ new); after removals they are the sequential rule over the leaves that
 * are left (a freed index can be taken again).  Candidates are looked up in the tree's leaf array on the device: the cost is k hash
 * chains and k log2(n_leaves) index reads, nothing of the tree's size is allocated, copied or scanned.
 * Errors, all with the tree untouched: DAPOL_ERR_INVALID_DIGEST_SIZE (digest_id not BLAKE3 / Blake2s / SHA-256 / SHA3-256), DAPOL_ERR_SPARSITY_TOO_SMALL
 * (2^height < 2 (n_leaves + k): Dapol::new's rule on the joined count), DAPOL_ERR_DUPLICATED_INTERNAL_ID (an internal id twice IN THE
 * BATCH), DAPOL_ERR_FAILED_TO_MAP_INDEX (dapol_last_error names the position within the batch), DAPOL_ERR_INVALID_ARGUMENT for a
 * tree marked invalid and for a shard tree (dapol_tree_build_shard), whose leaf array is not the whole set of taken indexes.
 * k = 0 does nothing.  The tree holds no ids: an internal id that one of its leaves already carries CANNOT be seen here.  The
 * caller's id map is the check -- Dapol::insert_liabilities (dapol.hpp) refuses such an id before calling the library. */
int32_t dapol_tree_derive_leaves(dapol_tree* tree, int32_t digest_id, const uint8_t* audit_seed, size_t audit_seed_len, size_t k,
                                 const uint8_t* internal_ids, const uint32_t* internal_off, const uint8_t* external_ids,
                                 const uint32_t* external_off, const uint64_t* values, uint64_t* leaf_idx_sorted, uint64_t* v_sorted,
                                 uint8_t* r32_sorted, uint32_t* order_sorted, uint64_t* idx_by_entity);
/* dapol_tree_derive_leaves, then dapol_tree_insert of the result: all or nothing (the derived batch, k x 48 bytes, passes through the
 * host).  idx_by_entity[k] (may be NULL; written on success only) = where each new liability went.  Afterwards the tree equals
 * dapol_tree_build over the old and the new leaves, as after dapol_tree_insert.  Refuses what dapol_tree_derive_leaves refuses and
 * what dapol_tree_insert refuses of a tree (built from a padding tape, workload trees), before anything is written; the same
 * caveat on ids the tree already carries. */
int32_t dapol_tree_insert_liabilities(dapol_tree* tree, int32_t digest_id, const uint8_t* audit_seed, size_t audit_seed_len, size_t k,
                                      const uint8_t* internal_ids, const uint32_t* internal_off, const uint8_t* external_ids,
                                      const uint32_t* external_off, const uint64_t* values, uint64_t* idx_by_entity);
/* A mixed change set as ONE edit: afterwards the leaf set is (old leaves - the leaves at remove_idx) + the puts.  A put at an index that
 * is a leaf replaces that liability, a put at any other index adds a leaf; put_was_new[n_put] (may be NULL; written on success only)
 * says which it was, in input order.  The tree then equals dapol_tree_build (dapol_tree_build_shard) over that leaf set with the
 * tree's pad seed bit for bit, at every level -- node counts, padding records, has_pad and parent pointers included -- whichever path
 * ran.  Leaves keep their blinding as given (bit 255 cleared, possibly >= l), value sums wrap, as in dapol_tree_insert.
 * ALL OR NOTHING -- every refusal is decided before the first write and leaves the tree unchanged and usable (dapol_last_error says
 * which rule was broken), in this order: an index twice in put_idx, or an index in both remove_idx and put_idx (a replacement is a put
 * alone) -> DAPOL_ERR_INVALID_ARGUMENT; a remove_idx entry that is not a leaf (also one outside the tree or outside a shard's prefix)
 * -> DAPOL_ERR_UNKNOWN_LEAF; a put outside the tree or outside a shard's prefix -> the code dapol_tree_update returns for that index;
 * a result with no leaf left -> DAPOL_ERR_INVALID_ARGUMENT.  A duplicate in remove_idx removes its leaf once; n_remove = n_put = 0
 * does nothing.  Refused like dapol_tree_update: trees built from a padding tape, workload trees, trees marked invalid.
 * Batches with height >= 1, every index in range, n_remove + n_put within update_incremental_max (dapol_options), at most 65,536, at
 * most an eighth of the leaves plus one, and at most 2^31 leaves afterwards go IN PLACE on the device: one planning launch, every
 * level up to the highest that changes rewritten once with what it gains and what it loses, every touched node made once.  A HIP
 * failure between the first and the last write of that path marks the tree invalid, as for dapol_tree_update.  Any other batch
 * rebuilds the tree from the merged leaf set (an error then leaves the old tree as it was).  On a context with a 64-byte digest the
 * hash chain is laid again afterwards.  Unlike three calls to dapol_tree_remove / _insert / _update, a refusal of any part leaves no
 * part applied. */
int32_t dapol_tree_apply(dapol_tree* tree, size_t n_remove, const uint64_t* remove_idx, size_t n_put, const uint64_t* put_idx,
                         const uint64_t* put_v, const uint8_t* put_r32, uint8_t* put_was_new);
/* What the last dapol_tree_update / dapol_tree_insert / dapol_tree_remove / dapol_tree_apply on this tree did: 0 = rebuilt, 1 = replaced
 * existing leaves in place, 2 = inserted new leaves in place (disjoint chains), 3 = both, 4 = removed leaves in place, 5 = inserted new
 * leaves in place by dapol_tree_insert's general path, 6 = applied in place by dapol_tree_apply (diagnostics; the tree is the same
 * whichever path ran). */
int32_t dapol_tree_last_update_path(dapol_tree* tree, int32_t* path);
/* Dapol::root_raw / Dapol::root (src/dapol/mod.rs:134-141). Any out pointer may be NULL. */
int32_t dapol_tree_root(dapol_tree* tree, uint8_t C32[32], uint8_t H32[32], uint64_t* v, uint8_t r32[32]);
int32_t dapol_tree_node_count(dapol_tree* tree, uint64_t* real_nodes, uint64_t* padding_nodes);
/* Every stored node of one level (0 = leaves .. height = root), real nodes first then padding nodes, for
 * parity tests on small trees.  Arrays sized by dapol_tree_level_size. */
int32_t dapol_tree_level_size(dapol_tree* tree, int32_t level, uint64_t* n_real, uint64_t* n_pad);
int32_t dapol_tree_level_nodes(dapol_tree* tree, int32_t level, uint64_t* idx, uint64_t* v, uint8_t* r32, uint8_t* C32,
                               uint8_t* H32, uint8_t* is_pad);
/* The sibling half of Dapol::generate_proof_batch for single leaves (src/dapol/mod.rs:172-184): for each of the
 * b leaves, its `height` siblings root side first: (C, H) = the Merkle path proof nodes, (v, r) = the secrets
 * handed to R::generate_proof.  Unknown leaf -> DAPOL_ERR_UNKNOWN_LEAF.  Out pointers may be NULL. */
int32_t dapol_tree_paths(dapol_tree* tree, size_t b, const uint64_t* leaf_idx, uint8_t* sib_C32, uint8_t* sib_H32,
                         uint64_t* sib_v, uint8_t* sib_r32);

/* generate_aggregated_range_proof / generate_single_range_proof (src/range/mod.rs:48-78 ->
 * RangeProof::prove_multiple / prove_single), batched over b independent proofs of m parties x n_bits each
 * (reference: n_bits = 64, src/range/mod.rs:16).  v[b][m], r32[b][m][32];  proofs_out[b][32*(9+2*lg(n_bits*m))].
 * Nonces: seed mode (nonce_seed32, stream_id[b], slot_base) or tape mode (tape != NULL:
 * tape[b][m*(2*n_bits+4)][64], slot_base ignored). */
int32_t dapol_range_prove_batch(dapol_ctx* ctx, int32_t n_bits, int32_t m, size_t b, const uint64_t* v, const uint8_t* r32,
                                const uint8_t nonce_seed32[32], const uint64_t* stream_id, uint64_t slot_base,
                                const uint8_t* tape, uint8_t* proofs_out);
size_t dapol_range_proof_size(int32_t n_bits, int32_t m);

/* verify_aggregated_range_proof / verify_single_range_proof (src/range/mod.rs:83-119 -> verify_multiple), batched:
 * proofs[b][size], V32[b][m][32] -> ok[b] (1 = verifies).
 * verify_seed32 (here and in dapol_verify_entities / dapol_verify_batch) is SOUNDNESS-CRITICAL: it keys the verifier's
 * random scalars -- c, which combines the two equations of one proof (thread_rng in the crate), and the weights of the
 * cross-proof batch check.  Pass NULL (recommended): the library draws 32 bytes from the OS CSPRNG per call.  A caller
 * seed is for reproducible tests; even then every scalar is derived from BLAKE3(seed | digest of every proof and
 * commitment of the batch), so a weight cannot be predicted before the proofs are fixed (Fiat-Shamir). */
int32_t dapol_range_verify_batch(dapol_ctx* ctx, int32_t n_bits, int32_t m, size_t b, const uint8_t* proofs, const uint8_t* V32,
                                 const uint8_t verify_seed32[32], uint8_t* ok);

/* Dapol::generate_proof for b single leaves (src/dapol/mod.rs:167-190 + R::generate_proof,
 * src/range/padding.rs:88-118 / src/range/splitting.rs:100-129): gathers each leaf's siblings on the GPU and
 * proves them under `policy` with `aggregation_factor`.  Outputs, per leaf: the Merkle path proof nodes
 * (path_C32/path_H32: [b][height][32], root side first; may be NULL) and the range proofs concatenated in
 * generation order (aggregated proofs, then the individual 672-byte proofs): range_out[b][dapol_entity_proof_size].
 * stream id of a leaf = its tree index. */
int32_t dapol_prove_entities(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy,
                             int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32], uint8_t* path_C32,
                             uint8_t* path_H32, uint8_t* range_out);
size_t dapol_entity_proof_size(int32_t height, int32_t policy, int32_t aggregation_factor, int32_t n_bits);
/* TAPE mode of dapol_prove_entities: the nonces of entity e are the draws tape[e][slot][64], slot < dapol_entity_tape_slots(...), in
 * the crate's draw order -- the sub-proofs of the policy one after the other (ONE RNG runs through R::generate_proof,
 * src/range/padding.rs:104-112, splitting.rs:110-123), inside each the slot order given at the top of this header.  What a Rust
 * harness replays through a custom RngCore into prove_multiple_with_rng (tools/replay_tape.rs). */
size_t dapol_entity_tape_slots(int32_t height, int32_t policy, int32_t aggregation_factor, int32_t n_bits);
int32_t dapol_prove_entities_tape(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor,
                                  int32_t n_bits, const uint8_t* tape, uint8_t* path_C32, uint8_t* path_H32, uint8_t* range_out);
/* Same, for a shard tree: the n_upper siblings above the shard root (root side first; identical for every leaf
 * of the shard) are prepended to each leaf's own siblings before the policy is applied.  Path outputs are
 * [b][n_upper + tree height][32]. */
int32_t dapol_prove_entities_upper(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy,
                                   int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32], int32_t n_upper,
                                   const uint8_t* up_C32, const uint8_t* up_H32, const uint64_t* up_v, const uint8_t* up_r32,
                                   uint8_t* path_C32, uint8_t* path_H32, uint8_t* range_out);

/* SHARED sub-proofs -- the counterpart of the reference's test-only DFS Dapol::generate_all_proofs (src/dapol/mod.rs:216-314) with
 * generate_proof_by_new_com / remove_proof_by_last_com (src/range/padding.rs:120-166, splitting.rs:131-178): a sub-proof over the
 * upper siblings of a path is the same statement for every leaf below that point, so it is proven ONCE per call and written into
 * the blob of every entity that contains it.  The blobs keep dapol_prove_entities' layout (dapol_entity_proof_size, the order of
 * the policy's plan, the wire format): dapol_verify_entities, dapol_range_proofs_serialize and dapol_proof_serialize take them as
 * they are.  Sharing leaks nothing: the shared object is a range proof over sibling commitments that each of its recipients holds
 * in its Merkle path already.
 *   Definition.  H = tree height + n_upper siblings per entity, in dapol_tree_paths' order (dapol_wire_config.siblings_leaf_first):
 * sibling i lies at depth i + 1 below the root (root side first, the default) or H - i (leaf first).  The KEY DEPTH D of a
 * sub-proof {start, count, m} of the plan is the largest depth among its siblings (start + count, or H - start leaf first; 0 for
 * the siblingless pad proof of aggregation_factor = 0).  The SUBTREE KEY S of an entity for it is its global leaf index with the low
 * H - D bits cleared.  The sub-proof's bytes are those of dapol_range_prove_batch(ctx, n_bits, m, 1, v, r, nonce_seed, &S, 0, NULL,
 * out) over its siblings in order, padded to m parties with (0, Scalar::one()).  The only difference from dapol_prove_entities is
 * the nonce stream: id S and slot base 0 instead of the leaf index and a slot base that runs through the plan; the key stays bound
 * to the statement (top of this header), so equal inputs give equal bytes and another statement another key.  Where the plan's
 * only sub-proof has D = H (padding with aggregation_factor = H, root side first) the blobs equal dapol_prove_entities' byte for byte.
 *   dapol_shared_plan: host-only index arithmetic (no GPU, no tree).  For strictly increasing leaf_idx below 2^height (else
 * DAPOL_ERR_INVALID_ARGUMENT) n_unique_out[s] (may be NULL) = distinct keys of sub-proof s of the plan among the b leaves,
 * *total_unique their sum = range proofs the shared call computes, *total_per_entity = b x plan size = what dapol_prove_entities
 * computes.  `height` is H.  Honours the sibling order of dapol_wire_config.
 *   dapol_prove_entities_shared: arguments and outputs as dapol_prove_entities_upper (n_upper = 0: a plain tree; 64-byte digests
 * with n_upper = 0 only).  leaf_idx must be strictly increasing (DAPOL_ERR_INVALID_ARGUMENT otherwise): the keys of every depth
 * then ascend and equal keys are adjacent.  *unique_subproofs_out (may be NULL) = range proofs actually computed.  Refusals as
 * dapol_prove_entities; an unknown leaf -> DAPOL_ERR_UNKNOWN_LEAF with no output written; b = 0 is DAPOL_OK.  Entities x plan
 * size must stay below 2^32 per call.  There is NO tape mode: a tape is one RNG per entity by construction, which is exactly what
 * sharing gives up.
 *   When to use it (tools/bench_shared.py): the time follows the sum of m over the distinct statements.
 * 2^20 random leaves at height 32, 64-bit proofs, one MI355X, whole call with the blobs copied back: padding / 16 20.0 -> 9.3 s (x2.15;
 * the sum-of-m ratio is 2.29), splitting / 24 19.7 -> 10.7 s (x1.85 of 1.91); padding / 32, where dapol_shared_plan reports nothing
 * to share and the bytes are dapol_prove_entities', 18.671 -> 18.675 s: heads + scan + scatter cost +0.02 %, below the 0.1 %
 * run-to-run spread, so either call serves there. */
int32_t dapol_shared_plan(int32_t height, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor,
                          uint64_t* n_unique_out, uint64_t* total_unique, uint64_t* total_per_entity);
int32_t dapol_prove_entities_shared(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy,
                                    int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32], int32_t n_upper,
                                    const uint8_t* up_C32, const uint8_t* up_H32, const uint64_t* up_v, const uint8_t* up_r32,
                                    uint8_t* path_C32, uint8_t* path_H32, uint8_t* range_out, uint64_t* unique_subproofs_out);

/* COMPACT shared proofs: every distinct sub-proof of a call leaves the prover and enters the verifier ONCE.  The index that such a
 * form needs costs nothing: the rows ascend, so which proof row e of sub-proof s uses is a function of leaf_idx and the plan alone.
 *   Definition.  For strictly increasing leaf_idx below 2^height and the policy's plan in blob order, sub-proof s has n_unique[s]
 * distinct subtree keys S (above) among the rows.  The COMPACT BUFFER is, for s = 0 .. n_sub - 1 in plan order, the n_unique[s]
 * proofs of sub-proof s in ascending key order, each dapol_range_proof_size(n_bits, m_s) bytes.  ref[s][e] = (distinct keys of s among
 * rows 0 .. e) - 1 is the proof of that list that row e uses; sub_off[s] is the byte offset of the list of s and sub_off[n_sub] the
 * total length.  A run of the plan's sub-proofs of equal m is contiguous: one [rows][proof bytes] batch.  It is the order in which
 * dapol_prove_entities_shared holds the proofs before it expands them.  Honours the sibling order of dapol_wire_config.
 *   Host-only (no context, no GPU), refusals as dapol_shared_plan plus a bad n_bits (DAPOL_ERR_INVALID_ARGUMENT):
 *   dapol_shared_compact_plan: sub_off [n_sub + 1] (may be NULL), ref [n_sub][b] (may be NULL), *compact_len (may be NULL).
 *   dapol_shared_expand: the per-entity blobs (dapol_entity_proof_size layout) of rows [first, first + count) into range_out; count = 1
 * cuts one user's proof out.  A compact_len that is not the layout's length, or first + count > b -> DAPOL_ERR_INVALID_ARGUMENT with
 * nothing written.
 *   dapol_shared_compress: the inverse for a caller who holds expanded blobs [b][entity bytes]: the bytes of the first row of every
 * run of equal keys; the other rows are not read.  compact_cap below the layout's length -> DAPOL_ERR_INVALID_ARGUMENT, nothing written.
 *   dapol_prove_entities_shared_compact: arguments, refusals and path outputs as dapol_prove_entities_shared (n_upper included); the
 * range output is the compact buffer: compact_out [compact_cap], *compact_len_out (may be NULL) its length, which is
 * dapol_shared_compact_plan's for (tree height + n_upper, leaf_idx).  The length is computed on the host before anything is queued; a
 * compact_cap below it -> DAPOL_ERR_INVALID_ARGUMENT with nothing written.  dapol_shared_expand of the output equals
 * dapol_prove_entities_shared's blobs byte for byte.  No [b][entity bytes] buffer is allocated on the device.
 *   When to use it (tools/bench_shared_compact.py, DESIGN.md section 4.4, profiles/shared_compact_2e18_h30.json: 2^18 random leaves
 * at height 30, 64-bit proofs, one MI355X, whole calls): what the call saves is the scatter, the download of every copy and the
 * [b][entity bytes] device buffer.  The bytes follow the count of distinct proofs: x1.19 fewer at padding / 16 (2.706 -> 2.666 s,
 * -1.5 %), x1.14 at splitting / 24 (2.807 -> 2.803 s: inside the shared call's 1.2 % spread, a MISS), x2.36 at padding / 0 (2.249 ->
 * 2.122 s, -5.7 %).  Proving dominates these calls, so use it for the memory and for a consumer that takes the compact form
 * (dapol_verify_entities_compact), not for prover time.  Do not use it where dapol_shared_plan reports nothing to share (padding /
 * height: 4.490 -> 4.489 s, no gain): dapol_prove_entities' blobs are the same bytes there. */
int32_t dapol_shared_compact_plan(int32_t height, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                                  uint64_t* sub_off, uint32_t* ref, uint64_t* compact_len);
int32_t dapol_shared_expand(int32_t height, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                            const uint8_t* compact, size_t compact_len, size_t first, size_t count, uint8_t* range_out);
int32_t dapol_shared_compress(int32_t height, size_t b, const uint64_t* leaf_idx, int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                              const uint8_t* range_blobs, uint8_t* compact_out, size_t compact_cap, uint64_t* compact_len_out);
int32_t dapol_prove_entities_shared_compact(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy,
                                            int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32], int32_t n_upper,
                                            const uint8_t* up_C32, const uint8_t* up_H32, const uint64_t* up_v, const uint8_t* up_r32,
                                            uint8_t* path_C32, uint8_t* path_H32, uint8_t* compact_out, size_t compact_cap,
                                            uint64_t* compact_len_out, uint64_t* unique_subproofs_out);

/* RE-PROVING after an edit of the tree (dapol_tree_update / _insert / _remove): a sub-proof {start, count, m} is a statement about
 * `count` sibling commitments, a sibling changes only when an edited leaf lies below it, and the shared prover's nonce key is bound
 * to the seed, S, (n, m) and those commitments -- so an unchanged statement has unchanged bytes and a changed one gets fresh nonces.
 * dapol_reprove_entities_shared takes the caller's old paths and blobs and proves only what moved.  The plan, S and the sibling
 * order are dapol_prove_entities_shared's.  PLAIN TREES ONLY: there is no n_upper, the sharded form is out of scope (DESIGN.md
 * section 9); a 64-byte-digest context works as in dapol_prove_entities_shared.
 *   Arguments.  leaf_idx: strictly increasing, the leaves of the tree AS IT IS NOW.  old_path_C32 [b][H][32] (the paths the old blobs
 * were proved over) and old_range [b][dapol_entity_proof_size] are ALIGNED with leaf_idx: the caller drops the rows of removed
 * leaves and sets has_old[e] = 0 for newly inserted ones, whose old rows are ignored.  has_old = NULL: every row has old data.
 *   Definitions.  DIRTY(s, e): has_old[e] == 0, or the `count` commitments old_path_C32[e][start .. start + count) differ from the
 * tree's current ones -- a comparison of bytes: nothing is keyed, no index is trusted.  The siblingless pad proof of aggregation 0
 * (count = 0) is dirty only without an old row.  HEAD(s, e): DIRTY(s, e) and (e = 0, or the key S of row e differs from row e - 1's,
 * or row e - 1 is not dirty).  Every head is proved once, with stream id S and slot base 0: exactly the bytes
 * dapol_prove_entities_shared gives that statement.  A dirty non-head row takes the proof of the head before it; a row that is not
 * dirty keeps its old bytes.  *proved_out = heads, *kept_out = kept (s, e) pairs (both may be NULL).  A kept row in the middle of a
 * key run may split the run into two heads: both give the same bytes, so this costs only work.
 *   Consequences.  If the old data came from dapol_prove_entities_shared under the same seed, policy, factor and n_bits, the outputs
 * equal a fresh dapol_prove_entities_shared on the edited tree byte for byte.  With another seed the kept proofs stay valid but
 * differ from a fresh call.  Old bytes are NOT checked: what goes in on a kept row comes out unchanged -- dapol_verify_entities is
 * the check.  Outputs may alias the old arrays (every input is uploaded before anything is written back).  Refusals as
 * dapol_prove_entities_shared: an unknown leaf (DAPOL_ERR_UNKNOWN_LEAF) or non-increasing indexes write nothing; in addition a NULL
 * old array while some has_old is set (or implied by has_old = NULL) is DAPOL_ERR_INVALID_ARGUMENT.  b = 0 is DAPOL_OK.
 *   dapol_reprove_plan: host-only index arithmetic (no GPU, no tree) with the same HEAD rule.  edited_idx: strictly increasing, the
 * replaced, inserted and removed leaves.  DIRTY(s, e): !has_old[e], or some edited x != leaf e first differs from leaf e at a depth
 * that one of the sub-proof's siblings occupies (depth counted from the root: sibling i lies at depth i + 1, or H - i leaf first).
 * An entity's own edit dirties nothing of its own.  Exact when every edit really changes its leaf's commitment, an upper bound
 * otherwise.  n_proved_out[s] (may be NULL) = heads of sub-proof s, *total_proved their sum = what dapol_reprove_entities_shared
 * proves, *sum_m_proved = the sum of m over them, *sum_m_shared = the sum of m over dapol_shared_plan's statements: one call gives
 * the ratio.  Refusals as dapol_shared_plan (for edited_idx as for leaf_idx).
 *   When to use it (tools/bench_reprove.py): the time follows the sum of m over the heads plus the trip of the
 * old arrays to the device.  2^20 random leaves at height 32, 64-bit proofs, one MI355X, whole call against dapol_prove_entities_shared
 * on the same edited tree: padding / 16 9.33 -> 1.13-1.16 s (x8.0-8.2; the sum-of-m ratio is 13.8-14.0) and splitting / 24 10.67 ->
 * 0.97-1.29 s (x8.3-11.0 of 11.4-16.7) for 1, 64 and 4,096 replaced liabilities; padding / 0 9.13 -> 1.24 s (x7.3: 0.80 s of it is the
 * upload of the 24 GB of old blobs); padding / 32 18.744 -> 18.828 s, +0.45 % where the shared call's spread is 0.04 %.  Where
 * dapol_reprove_plan reports nothing to keep (padding with aggregation_factor = H: the one sub-proof covers every sibling, and an edit lies below one
 * sibling of every other leaf) the call can only add the upload and the comparison to the shared call: use the shared call there. */
int32_t dapol_reprove_plan(int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* has_old, size_t k, const uint64_t* edited_idx,
                           int32_t policy, int32_t aggregation_factor, uint64_t* n_proved_out, uint64_t* total_proved, uint64_t* sum_m_proved,
                           uint64_t* sum_m_shared);
int32_t dapol_reprove_entities_shared(dapol_ctx* ctx, dapol_tree* tree, size_t b, const uint64_t* leaf_idx, int32_t policy,
                                      int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32], const uint8_t* has_old,
                                      const uint8_t* old_path_C32, const uint8_t* old_range, uint8_t* path_C32, uint8_t* path_H32,
                                      uint8_t* range_out, uint64_t* proved_out, uint64_t* kept_out);

/* A PROOF STORE keeps what dapol_prove_entities_shared issues -- for one (context, tree, policy, aggregation factor, n_bits, nonce seed) --
 * in device memory between calls: the strictly increasing leaf indexes of its rows, their sibling commitments [rows][H][32] and hashes
 * [rows][H][dapol_ctx_digest_bytes], their blobs [rows][dapol_entity_proof_size], exactly the shared call's layout.  After an edit of the
 * tree a refresh re-proves what dapol_reprove_entities_shared would re-prove, with the old data where the last refresh left it: no
 * old array goes up and no blob comes down; a caller fetches the rows it serves.  PLAIN TREES ONLY, no tape mode, as the re-prover.
 *   Ownership.  The store retains its context and is counted by its tree: dapol_tree_destroy on a tree with a live store returns
 * DAPOL_ERR_INVALID_ARGUMENT and destroys nothing -- destroy the store first.  The tree may be edited freely between calls (update,
 * insert, remove, whichever path they take); the store reads it only inside its own calls, on the context's stream, so calls on one
 * context must not run concurrently, as everywhere.  Every call below except _destroy refuses (DAPOL_ERR_INVALID_ARGUMENT, nothing
 * written) a NULL store, a tree marked invalid, a store marked unusable, and a dapol_wire_config whose siblings_leaf_first differs
 * from the value recorded at creation (the stored paths and the plan's keys are in that order).
 *   dapol_proof_store_create: an empty store (0 rows).  Refuses what dapol_reprove_entities_shared refuses for the same context, tree,
 * policy, aggregation_factor and n_bits, with the same codes, messages and precedence, and a tree that does not own its leaves (a
 * workload's), as dapol_tree_update does.  *store is written only on success.
 *   dapol_proof_store_destroy: overwrites the seed on the device, frees everything, releases the context.  NULL is DAPOL_OK.
 *   dapol_proof_store_refresh: afterwards the store holds the shared call's outputs, for the tree as it is now, of the b strictly
 * increasing leaf_idx.  leaf_idx = NULL with b = 0: every leaf of the tree, read from the tree's own device array (no upload); a
 * non-NULL leaf_idx with b = 0 empties the store.  *proved = heads and *kept = (sub-proof, row) pairs not dirty, as
 * dapol_reprove_entities_shared defines them with the store's previous rows as the old data; *moved_rows = old rows copied into new
 * buffers.  Each of the three may be NULL.  When the leaf set is unchanged -- every update-only edit -- nothing moves (*moved_rows = 0):
 * the new paths are gathered into the store's spare sibling arrays and compared with the ones in use, the dirty pieces are written
 * into the blobs where they lie, the arrays swap.  Otherwise the surviving rows are copied into newly allocated buffers
 * (*moved_rows = their number; the old blob buffer is freed after the copy, so both exist for the length of the call), new leaves are
 * proved from scratch.  All or nothing up to the first write into the store: non-increasing indexes, an index that is no leaf
 * (DAPOL_ERR_UNKNOWN_LEAF) and a failed allocation (DAPOL_ERR_OUT_OF_MEMORY) leave the store byte for byte as it was; when rows
 * move every write goes to the new buffers, so any failure does.  A HIP failure after the first write of an in-place refresh marks
 * the store unusable, the way trees are marked: destroy it and create it again.
 *   dapol_proof_store_rows / _entity_bytes: the row count; dapol_entity_proof_size of the store's shape.  0 for NULL.
 *   dapol_proof_store_fetch: the rows of k leaves, in any order, duplicates allowed, gathered on the device into one staging buffer and
 * copied back from there: found[i] = 1 and row i of path_C32 [k][H][32], path_H32 [k][H][digest bytes], range_out [k][entity bytes]
 * filled, or found[i] = 0 and the rows zero for a leaf the store does not hold (whether or not the tree has it).  Output pointers may
 * be NULL.  k = 0 does nothing.
 *   dapol_proof_store_read: rows [first, first + count) by plain copies, leaf indexes included; refused when first + count exceeds
 * the rows.  Output pointers may be NULL.
 *   dapol_proof_store_verify: ok[rows] = what dapol_verify_entities returns for the rows read back, with the leaves' own commitments and
 * hashes and the root taken from the tree as it is now -- so in a store that has not been refreshed since an edit every row whose path
 * passes an edited leaf fails (all but a lone edited leaf's own row: its edit lies below none of its own siblings), which is the point
 * of the check.  Only the verdict bytes cross the bus.  verify_seed32 = NULL draws one, as elsewhere.  A stored leaf that the
 * tree no longer holds -> DAPOL_ERR_UNKNOWN_LEAF, nothing written.
 *   dapol_proof_store_read_compact: the range proofs of ALL stored rows in the compact layout of their own leaf indexes ("COMPACT
 * shared proofs" above: dapol_shared_compact_plan over dapol_proof_store_read's leaf indexes gives the length and the index;
 * dapol_shared_expand gives the blobs back).  The first row of every run of equal subtree keys is gathered on the device into a
 * staging buffer of exactly that length and copied back once; the store itself stays as it is.  compact_cap below the length ->
 * DAPOL_ERR_INVALID_ARGUMENT with nothing written; an empty store gives length 0.  Refresh + read of everything against refresh +
 * read_compact (same file): 0.187 -> 0.079 s at padding / 0, where the leg is all bus; within 1 % at padding / 16 and splitting / 24,
 * where the refresh is proving.
 *   When to use it (tools/bench_proof_store.py): whenever proofs are served after edits and the caller does not
 * need every blob back after every edit. */
typedef struct dapol_proof_store dapol_proof_store;
int32_t dapol_proof_store_create(dapol_ctx* ctx, dapol_tree* tree, int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                                 const uint8_t nonce_seed32[32], dapol_proof_store** store);
int32_t dapol_proof_store_destroy(dapol_proof_store* store);
int32_t dapol_proof_store_refresh(dapol_proof_store* store, size_t b, const uint64_t* leaf_idx, uint64_t* proved, uint64_t* kept,
                                  uint64_t* moved_rows);
size_t dapol_proof_store_rows(dapol_proof_store* store);
size_t dapol_proof_store_entity_bytes(dapol_proof_store* store);
int32_t dapol_proof_store_fetch(dapol_proof_store* store, size_t k, const uint64_t* leaf_idx, uint8_t* found, uint8_t* path_C32,
                                uint8_t* path_H32, uint8_t* range_out);
int32_t dapol_proof_store_read(dapol_proof_store* store, size_t first, size_t count, uint64_t* leaf_idx_out, uint8_t* path_C32,
                               uint8_t* path_H32, uint8_t* range_out);
int32_t dapol_proof_store_verify(dapol_proof_store* store, const uint8_t verify_seed32[32], uint8_t* ok);
int32_t dapol_proof_store_read_compact(dapol_proof_store* store, uint8_t* compact_out, size_t compact_cap, uint64_t* compact_len_out);

/* Serializable for RangeProofPadding / RangeProofSplitting (src/range/padding.rs:38-69, src/range/splitting.rs:36-84):
 * the range-proof blob of ONE entity as written by dapol_prove_entities <-> R::serialize() bytes
 * ((aggregated_num ||) (size || proof)... || individual_num || proofs...; field widths src/range/mod.rs:18-21).
 * Host-only.  Deserialisation applies RangeProof::from_bytes' framing / canonical-scalar checks and returns
 * DAPOL_ERR_BYTES_NOT_ENOUGH / DAPOL_ERR_VALUE_DECODING like deserialize_range_proof (src/range/mod.rs:124-139). */
size_t dapol_range_proofs_wire_size(int32_t height, int32_t policy, int32_t aggregation_factor, int32_t n_bits);
int32_t dapol_range_proofs_serialize(int32_t height, int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t* blob,
                                     uint8_t* wire_out);
int32_t dapol_range_proofs_deserialize(int32_t policy, int32_t n_bits, const uint8_t* wire, size_t wire_len, uint8_t* blob_out, size_t blob_cap,
                                       uint32_t* n_aggregated, uint64_t* agg_sizes, uint64_t* n_individual, size_t* consumed);

/* What smtree 0.1.2 owns and nothing in the reference repository pins (the crate is not vendored, no golden bytes exist):
 * one field per assumption, the defaults being the believed values.  Process-wide; set it before proving / serialising.
 * A maintainer with cargo closes these with tools/replay_tape.rs -> tests/golden/from_reference/ (INTEGRATION.md). */
typedef struct {
    int32_t int_big_endian;       /* smtree::utils::usize_to_bytes byte order: 1 = big-endian (default), 0 = little-endian */
    int32_t batch_num_bytes;      /* MerkleProof::serialize: width of the leaf-count field (default 8) */
    int32_t sibling_num_bytes;    /* MerkleProof::serialize: width of the sibling-count field (default 8) */
    int32_t tree_height_bytes;    /* TreeIndex::serialize: width of the height field (default 2) */
    int32_t path_bytes_full;      /* 0 (default): a path takes ceil(height / 8) bytes; 1: all 32 bytes of TreeIndex.pos */
    int32_t siblings_leaf_first;  /* order of a proof's siblings = of the range proof's parties: 0 (default) from the root side
                                     down, 1 from the leaf level up (batched proofs: level by level in that direction) */
} dapol_wire_config;
int32_t dapol_wire_config_get(dapol_wire_config* out);
int32_t dapol_wire_config_set(const dapol_wire_config* cfg);

/* Serializable for DapolProofNode (src/proof/node.rs:74-102), n nodes: wire = (C32 || hash32) per node.  Deserialisation
 * decompress-validates every commitment in one GPU launch: DAPOL_ERR_BYTES_NOT_ENOUGH / DAPOL_ERR_VALUE_DECODING ("Not the
 * canonical encoding of a point."). */
int32_t dapol_proof_nodes_serialize(size_t n, const uint8_t* C32, const uint8_t* H32, uint8_t* wire_out);
int32_t dapol_proof_nodes_deserialize(dapol_ctx* ctx, size_t n, const uint8_t* wire, size_t wire_len, uint8_t* C32_out, uint8_t* H32_out);
/* ... for a digest of hash_bytes = D::output_size() bytes (32 or 64): wire = (C32 || hash) per node, H holds hash_bytes per node.
 * (The context-taking deserialisers read the width from their context.) */
int32_t dapol_proof_nodes_serialize_d(int32_t hash_bytes, size_t n, const uint8_t* C32, const uint8_t* H, uint8_t* wire_out);

/* DapolProof::serialize / deserialize (src/proof/mod.rs:68-85): R::serialize() || MerkleProof::serialize(), the latter
 * restated as batch_num || sibling_num || tree_height || path_1..k || (C || hash)_1..S (smtree 0.1.2, from memory: see
 * dapol_wire_config).  k leaves (k = 1: a proof of dapol_prove_entities with n_siblings = height and the path arrays as
 * siblings; k > 1: the outputs of dapol_prove_batch); range_blob = the range proofs in dapol_prove_entities' blob layout.
 * dapol_proof_deserialize: first call with all four output arrays NULL -> height, k, n_siblings, aggregation_factor
 * (= n_siblings - number of individual proofs, src/range/padding.rs:172) and range_blob_len; second call fills the
 * arrays.  Errors as the reference: DAPOL_ERR_BYTES_NOT_ENOUGH, DAPOL_ERR_VALUE_DECODING (range-proof framing, non-canonical
 * scalars, sibling commitments that do not decompress -- validated on the GPU). */
size_t dapol_proof_wire_size(int32_t height, size_t k, size_t n_siblings, int32_t policy, int32_t aggregation_factor, int32_t n_bits);
int32_t dapol_proof_serialize(int32_t height, size_t k, const uint64_t* leaf_idx, size_t n_siblings, const uint8_t* sib_C32,
                              const uint8_t* sib_H32, int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                              const uint8_t* range_blob, uint8_t* wire_out);
size_t dapol_proof_wire_size_d(int32_t hash_bytes, int32_t height, size_t k, size_t n_siblings, int32_t policy, int32_t aggregation_factor, int32_t n_bits);
int32_t dapol_proof_serialize_d(int32_t hash_bytes, int32_t height, size_t k, const uint64_t* leaf_idx, size_t n_siblings, const uint8_t* sib_C32,
                                const uint8_t* sib_H, int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t* range_blob,
                                uint8_t* wire_out);
int32_t dapol_proof_deserialize(dapol_ctx* ctx, int32_t policy, int32_t n_bits, const uint8_t* wire, size_t wire_len, int32_t* height,
                                size_t* k, size_t* n_siblings, int32_t* aggregation_factor, size_t* range_blob_len,
                                uint64_t* leaf_idx_out, uint8_t* sib_C32_out, uint8_t* sib_H32_out, uint8_t* range_blob_out,
                                size_t* consumed);

/* DapolProof::verify (src/proof/mod.rs:41-47 + :89-95) for b single-leaf inclusion proofs as produced by
 * dapol_prove_entities: MerkleProof::verify by re-merging the leaf proof node with its siblings (DapolProofNode::merge,
 * src/proof/node.rs:56-69; a sibling commitment that is not a canonical point fails like deserialisation does, :88-94)
 * and then RangeVerifiable::verify of the policy over the sibling commitments.  ok[i] = 1 iff both hold. */
int32_t dapol_verify_entities(dapol_ctx* ctx, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32,
                              const uint8_t* leaf_H32, const uint8_t* path_C32, const uint8_t* path_H32, const uint8_t root_C32[32],
                              const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                              const uint8_t* range_proofs, const uint8_t verify_seed32[32], uint8_t* ok);

/* Batched inclusion proofs -- Dapol::generate_proof_batch for k >= 1 leaves (src/dapol/mod.rs:172-190) and
 * DapolProof::verify_batch (src/proof/mod.rs:49-54): ONE proof for all k leaves = the deduplicated siblings of the
 * batched Merkle paths + one R::generate_proof over exactly those siblings (values / blindings in sibling order).
 * leaf_idx must be strictly increasing.  Sibling order: level by level from the root side, left to right within a
 * level (for k = 1 this is dapol_tree_paths' order; smtree's own order is not pinned by the reference repository).
 *
 * dapol_batch_siblings: number of siblings and, optionally, their positions (sib_level: 0 = leaf level; sib_index:
 * node index within its level).  Pure index arithmetic -- no GPU, no tree.
 * dapol_prove_batch: sib_C32 / sib_H32: [n_siblings][32] (may be NULL); range_out:
 * dapol_entity_proof_size(n_siblings, policy, aggregation_factor, n_bits) bytes in dapol_prove_entities' blob layout.
 * aggregation_factor > n_siblings -> DAPOL_ERR_INVALID_ARGUMENT (the reference panics, src/range/padding.rs:95-98).
 * For k > 1 the nonce stream is keyed by the seed chained through the leaf list, so a batch never shares nonces with
 * a single-leaf proof made from the same seed; k = 1 gives exactly dapol_prove_entities' bytes.
 * dapol_verify_batch: *ok = 1 iff the leaves and siblings re-merge to the root and R::verify accepts. */
int32_t dapol_batch_siblings(int32_t height, size_t k, const uint64_t* leaf_idx, size_t* n_siblings, uint8_t* sib_level,
                             uint64_t* sib_index);
int32_t dapol_prove_batch(dapol_ctx* ctx, dapol_tree* tree, size_t k, const uint64_t* leaf_idx, int32_t policy,
                          int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32], uint8_t* sib_C32,
                          uint8_t* sib_H32, uint8_t* range_out);
int32_t dapol_verify_batch(dapol_ctx* ctx, int32_t height, size_t k, const uint64_t* leaf_idx, const uint8_t* leaf_C32,
                           const uint8_t* leaf_H32, size_t n_siblings, const uint8_t* sib_C32, const uint8_t* sib_H32,
                           const uint8_t root_C32[32], const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor,
                           int32_t n_bits, const uint8_t* range_proofs, const uint8_t verify_seed32[32], uint8_t* ok);

/* Length-checked forms for buffers that come from UNTRUSTED bytes (a decoded wire): the counts the caller holds are compared
 * with what (height, policy, aggregation_factor, n_bits) imply before anything is read; a proof of the wrong shape is an INVALID
 * proof (ok = 0, DAPOL_OK), never an over-read.  n_path_nodes = records in path_C32 / path_H32 (must be b * height);
 * range_proofs_len in bytes (must be b * dapol_entity_proof_size(height, ...), or the size over n_siblings for a batch proof). */
int32_t dapol_verify_entities_checked(dapol_ctx* ctx, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32, const uint8_t* leaf_H32,
                                      size_t n_path_nodes, const uint8_t* path_C32, const uint8_t* path_H32, const uint8_t root_C32[32],
                                      const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t* range_proofs,
                                      size_t range_proofs_len, const uint8_t verify_seed32[32], uint8_t* ok);
int32_t dapol_verify_batch_checked(dapol_ctx* ctx, int32_t height, size_t k, const uint64_t* leaf_idx, const uint8_t* leaf_C32, const uint8_t* leaf_H32,
                                   size_t n_siblings, const uint8_t* sib_C32, const uint8_t* sib_H32, const uint8_t root_C32[32], const uint8_t root_H32[32],
                                   int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t* range_proofs, size_t range_proofs_len,
                                   const uint8_t verify_seed32[32], uint8_t* ok);

/* MANY batched inclusion proofs in one call -- Dapol::generate_proof_batch_for_ids (src/dapol/mod.rs:155-190) for every customer
 * who holds several accounts, or for every sample of an auditor: nb batches, batch j = the leaves
 * leaf_idx[batch_off[j] .. batch_off[j + 1]) (batch_off[0] = 0).  Every batch is non-empty, strictly increasing and below 2^height;
 * batches may overlap each other and may repeat.
 *   Definition.  The prover's outputs are the concatenation, in the caller's batch order, of what dapol_prove_batch returns for
 * each batch under the same nonce_seed32 -- siblings and range blobs, byte for byte: batch j's siblings are records
 * [sib_off[j], sib_off[j + 1]) of sib_C32 / sib_H32 and its blob is bytes [range_off[j], range_off[j + 1]) of range_out, at
 * dapol_batches_plan's offsets.  So a batch of one leaf is proved under the caller's seed (dapol_prove_entities' bytes), a longer one
 * under the seed chained through its leaves, with its first leaf as the stream id.  ok[j] of the verifier is what
 * dapol_verify_batch_checked returns for batch j, for every input.
 *   How.  A batch with S deduplicated siblings is one row of the policy prover over S siblings, and the batches of a call with
 * equal S share one plan: each distinct S is ONE [rows][S] call of the batched prover (verifier) instead of one small call per
 * batch.  The groups run one after the other; *n_groups_out (may be NULL) is their number.  A call with few distinct S is fast; a
 * call whose every batch has an S of its own does what a loop over dapol_prove_batch does.
 *   dapol_batches_plan: host-only (no context, no GPU).  Each output may be NULL: n_siblings [nb], sib_off [nb + 1] in sibling
 * records, range_off [nb + 1] in bytes (dapol_entity_proof_size(n_siblings[j], policy, aggregation_factor, n_bits) each), *n_groups.
 * Honours dapol_wire_config.siblings_leaf_first.  Refusals: height > 64 -> DAPOL_ERR_TREE_HEIGHT_TOO_BIG; a batch_off that does
 * not start at 0 or decreases, or leaves x height >= 2^32 (the gather index has 32 bits) -> DAPOL_ERR_INVALID_ARGUMENT; then
 * dapol_prove_batch's refusals (bad leaf indexes, aggregation_factor outside [0, n_siblings[j]], a bad n_bits) for the FIRST batch in
 * caller order that it would refuse, with "batch <j>:" in dapol_last_error.  nb = 0 is DAPOL_OK with empty outputs.
 *   dapol_prove_batches: everything is validated on the host before anything is queued.  sib_C32 / sib_H32 (may be NULL):
 * [sib_off[nb]][32]; range_out: range_off[nb] bytes.  A leaf that the tree does not hold -> DAPOL_ERR_UNKNOWN_LEAF with no output
 * written; a shard tree is refused as dapol_prove_batch refuses it.
 *   dapol_verify_batches: leaf_C32 / leaf_H32 [batch_off[nb]][32]; sib_off [nb + 1] and range_off [nb + 1] are the lengths the caller
 * actually HOLDS (records of sib_C32 / sib_H32, bytes of range_proofs; non-decreasing, else DAPOL_ERR_INVALID_ARGUMENT): a batch
 * whose counts differ from the plan's is an invalid proof -- ok[j] = 0 -- not an error and never an over-read, and it never changes
 * another batch's verdict.  Errors are dapol_verify_batch_checked's, for the first batch in caller order.  verify_seed32 = NULL
 * draws a seed from the OS.  Only ok[nb] comes back from the device.
 *   Left out: 64-byte digests (a Blake2b context is refused with DAPOL_ERR_INVALID_DIGEST_SIZE by both calls), shard trees and the
 * records route, tape mode, S-groups side by side, sub-proofs shared between batches. */
int32_t dapol_batches_plan(int32_t height, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx, int32_t policy,
                           int32_t aggregation_factor, int32_t n_bits, uint64_t* n_siblings, uint64_t* sib_off, uint64_t* range_off,
                           uint64_t* n_groups);
int32_t dapol_prove_batches(dapol_ctx* ctx, dapol_tree* tree, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx,
                            int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32], uint8_t* sib_C32,
                            uint8_t* sib_H32, uint8_t* range_out, uint64_t* n_groups_out);
int32_t dapol_verify_batches(dapol_ctx* ctx, int32_t height, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx,
                             const uint8_t* leaf_C32, const uint8_t* leaf_H32, const uint64_t* sib_off, const uint8_t* sib_C32,
                             const uint8_t* sib_H32, const uint8_t root_C32[32], const uint8_t root_H32[32], int32_t policy,
                             int32_t aggregation_factor, int32_t n_bits, const uint64_t* range_off, const uint8_t* range_proofs,
                             const uint8_t verify_seed32[32], uint8_t* ok);

/* RE-PROVING BATCHES after an edit of the tree (dapol_tree_update / _insert / _remove / _apply) -- what dapol_reprove_entities_shared
 * is to single-leaf proofs.  A sub-proof {start, count, m} of a batch is a statement about `count` sibling commitments, and its nonce
 * key is derived from the batch's seed (the caller's for one leaf, the chain through the leaves otherwise), the stream id (the
 * batch's first leaf), the sub-proof's first slot (a function of the plan alone), (n, m) and those commitments -- from nothing else.
 * So a sub-proof whose sibling commitments did not move has exactly the bytes it had, and one whose commitments moved gets fresh
 * nonces.  dapol_reprove_batches takes the caller's old siblings and blobs and proves only what moved.
 *   Arguments.  The batches are dapol_prove_batches': non-empty, strictly increasing, free to overlap and repeat, and leaves of the
 * tree AS IT IS NOW (the caller drops the batches that lost a leaf).  The offsets are dapol_batches_plan's sib_off / range_off:
 * sibling positions depend on the batch's leaves alone, so no edit moves them.  old_sib_C32 [sib_off[nb]][32] and old_range
 * (range_off[nb] bytes) are in that layout.  has_old[j] = 0 marks a batch with no old proof, whose old rows are ignored;
 * has_old = NULL: every batch has an old proof.
 *   Definitions.  DIRTY(j, s): has_old[j] == 0, or the `count` commitments old_sib_C32[sib_off[j] + start .. + count) differ in any
 * byte from the tree's current ones -- a comparison of bytes: nothing is keyed, no index is trusted.  The siblingless pad proof of
 * aggregation 0 (count = 0) is dirty only without an old proof.  Every dirty sub-proof is proved with the seed, stream id and slot
 * that dapol_prove_batch uses for it, its padding parties the policy's (v = 0, r = 1, commitment B_blinding); one that is not dirty
 * keeps its old bytes.  There is no head rule: batches share nothing, and a repeated batch is proved twice.  *proved_out = dirty
 * sub-proofs, *kept_out = the other (batch, sub-proof) pairs, *n_calls_out = calls of the range prover made: all dirty sub-proofs
 * of one m are ONE call whatever their batch's sibling count, so at most the number of distinct m (each may be NULL).
 *   Consequences.  With old data from dapol_prove_batches or dapol_prove_batch under the same seed, policy, factor, n_bits and
 * sibling order, the outputs equal a fresh dapol_prove_batches on the edited tree byte for byte.  With another seed the kept pieces
 * stay valid but differ from a fresh call.  Old bytes are NOT checked: what goes in on a kept sub-proof comes out unchanged --
 * dapol_verify_batches is the check.  Outputs may alias the old arrays (every input is uploaded before anything is written back).
 * When nothing is dirty the range prover is not entered.
 *   Refusals.  What dapol_prove_batches refuses, with its codes, messages ("batch <j>:") and precedence, shard trees and 64-byte
 * digests included; an unknown leaf -> DAPOL_ERR_UNKNOWN_LEAF with nothing written; after those, a NULL old array (old_sib_C32 while
 * there are siblings, old_range while there are blob bytes) while some batch has an old proof -> DAPOL_ERR_INVALID_ARGUMENT.
 * nb = 0 is DAPOL_OK.
 *   dapol_reprove_batches_plan: host-only index arithmetic (no context, no GPU, no tree).  edited_idx [k]: strictly increasing and
 * below 2^height (else DAPOL_ERR_INVALID_ARGUMENT, after dapol_batches_plan's own refusals), the replaced, inserted and removed
 * leaves.  DIRTY(j, s): !has_old[j], or some edited x lies below a sibling of the sub-proof: x >> level == index for one of the
 * positions dapol_batch_siblings gives.  An edited leaf that is a leaf of the batch lies below none of its siblings and dirties
 * nothing of that batch.  Exact when every edit really changes its leaf's commitment, an upper bound otherwise.  n_proved [nb] (may
 * be NULL) = dirty sub-proofs of each batch, *total_proved their sum = what dapol_reprove_batches proves, *sum_m_proved and
 * *sum_m_all = the sums of m over the dirty sub-proofs and over all of them: one call gives the ratio.
 *   When to use it (tools/bench_reprove_batches.py): the time follows the sum of m over the dirty sub-proofs
 * plus the trip of the old arrays, and the call pays one latency chain per distinct m where dapol_prove_batches pays one per distinct
 * sibling count.  2^16 leaves at height 32, 4,096 batches of 2 / 4 random leaves, 64-bit proofs, one MI355X, whole call against
 * dapol_prove_batches on the same edited tree, 1 to 4,096 replaced liabilities: padding / 16 0.28 / 0.50 -> 0.07-0.14 s (x3.4-6.5; the
 * sum-of-m ratio is 2.8-7.7), splitting / 24 0.34 / 0.61 -> 0.07-0.15 s (x3.6-7.1 of 2.5-7.5), padding / 0 0.26 / 0.47 -> 0.02-0.13 s
 * (x3.3-13 of 2.9-118).  Padding with the factor at the smallest sibling count of the call (51; next to nothing is kept) still ran
 * in 0.18 s against 0.42 s, because all of its 64-party proofs are one call here and twelve S-groups there.
 *   Left out: shard trees and the records route, 64-byte digests, tape mode.  The old siblings and blobs cross
 * the bus in both directions on every call; dapol_batch_store below keeps them on the device. */
int32_t dapol_reprove_batches_plan(int32_t height, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx, const uint8_t* has_old,
                                   size_t k, const uint64_t* edited_idx, int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                                   uint64_t* n_proved, uint64_t* total_proved, uint64_t* sum_m_proved, uint64_t* sum_m_all);
int32_t dapol_reprove_batches(dapol_ctx* ctx, dapol_tree* tree, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx,
                              int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t nonce_seed32[32],
                              const uint8_t* has_old, const uint8_t* old_sib_C32, const uint8_t* old_range, uint8_t* sib_C32,
                              uint8_t* sib_H32, uint8_t* range_out, uint64_t* proved_out, uint64_t* kept_out, uint64_t* n_calls_out);

/* A BATCH STORE keeps what dapol_prove_batches issues for one batch list -- under one (context, tree, policy, aggregation factor, n_bits,
 * nonce seed) -- in device memory between calls: what dapol_proof_store is to single-leaf proofs.  A ROW is a batch; rows are in the
 * caller's order of the last successful refresh.  The store keeps, at dapol_batches_plan's offsets, the leaf lists, the sibling
 * commitments [sib_off[rows]][32], the sibling hashes and the blobs (range_off[rows] bytes) on the device, and a copy of batch_off /
 * leaf_idx on the host.  After an edit of the tree a refresh re-proves what dapol_reprove_batches would re-prove, with the old data
 * where the last refresh left it: no old array goes up and no blob comes down; a caller fetches the rows it serves.
 *   Ownership.  As dapol_proof_store: the store retains its context and is counted by its tree (the same counter: dapol_tree_destroy
 * on a tree with a live store returns DAPOL_ERR_INVALID_ARGUMENT and destroys nothing).  The tree may be edited freely between calls;
 * the store reads it only inside its own calls, on the context's stream.  Every call below except _destroy and _rows refuses
 * (DAPOL_ERR_INVALID_ARGUMENT, nothing written) a NULL store, a tree marked invalid, a store marked unusable, and a dapol_wire_config
 * whose siblings_leaf_first differs from the value recorded at creation.
 *   dapol_batch_store_create: an empty store (0 rows).  Refuses what dapol_reprove_batches refuses for the same context and tree, with
 * its codes: NULL arguments, a tree of another context, a shard tree, a 64-byte digest (DAPOL_ERR_INVALID_DIGEST_SIZE).  What depends
 * on a batch (aggregation_factor, n_bits, the parties) is refused by the refresh that brings the batch.  *store is written only on success.
 *   dapol_batch_store_destroy: overwrites the seed on the device, frees everything, releases the context.  NULL is DAPOL_OK.
 *   dapol_batch_store_refresh: afterwards _read(0, rows) equals, byte for byte (siblings C, siblings H, blobs), what dapol_prove_batches
 * returns for the store's list on the tree as it is now under the store's seed, policy, factor and n_bits.  batch_off = NULL with
 * nb = 0: the list the store already holds (every update-only edit); a non-NULL batch_off replaces the list, with nb = 0 it empties
 * the store.  CONTINUATION: new batch j continues an old row when their leaf lists are equal, in length and in every index; of several
 * equal old rows the lowest (equal lists have equal bytes under one seed -- the seed chains through the leaves -- so the choice cannot
 * be observed); a batch with no equal old row has no old proof.  *proved, *kept and *n_calls are dapol_reprove_batches' for the new
 * list with the store's previous rows as the old data and has_old = the continuation; *moved_rows = old rows copied into new buffers.
 * Each of the four may be NULL.  IN PLACE, when the list is unchanged (NULL, or equal to the stored list row for row): nothing moves
 * (*moved_rows = 0), the new siblings are gathered into the store's spare sibling arrays and compared with the ones in use, the dirty
 * pieces are written into the blobs where they lie, the arrays swap; the plan tables are on the device already, so nothing is
 * uploaded.  MOVING, in every other case: new buffers are allocated at the new offsets, continued rows are copied into them (blobs,
 * and the old commitments to compare against), everything else is proved fresh, the old buffers are freed after the copy.  All or
 * nothing: a bad list and an aggregation_factor above some batch's sibling count (dapol_prove_batches' refusals, with its codes, its
 * "batch <j>:" messages and its precedence), a leaf the tree does not hold (DAPOL_ERR_UNKNOWN_LEAF) and a failed allocation leave the
 * store byte for byte as it was.  A stored batch whose leaf has been removed meets the unknown-leaf case on a NULL-list refresh: pass
 * the list without that batch.  A HIP failure after the first write of an in-place refresh marks the store unusable: destroy it and
 * create it again.
 *   dapol_batch_store_rows: the row count; 0 for NULL.
 *   dapol_batch_store_layout: the host copy of the list and dapol_batches_plan's offsets for it: batch_off [rows + 1], leaf_idx
 * [batch_off[rows]], sib_off [rows + 1] (records), range_off [rows + 1] (bytes).  Each output may be NULL.
 *   dapol_batch_store_fetch: k row numbers, in any order, duplicates allowed; the rows are gathered on the device into one staging
 * buffer in the layout dapol_batches_plan gives for those batches in query order, and copied back from there.  A row number >= rows
 * -> DAPOL_ERR_INVALID_ARGUMENT with nothing written.  Output pointers may be NULL.  k = 0 does nothing.
 *   dapol_batch_store_read: rows [first, first + count) by plain copies; refused when first + count exceeds the rows.  Output pointers
 * may be NULL.
 *   dapol_batch_store_verify: ok[rows] = what dapol_verify_batches returns for the rows read back, with the leaves' commitments and
 * hashes taken from level 0 of the tree as it is now and the root from its top level -- so in a store that has not been refreshed
 * since an edit every batch with a sibling above an edited leaf fails (a batch that holds the edited leaf itself stays valid).  Only
 * ok crosses the bus.  verify_seed32 = NULL draws one.  A stored leaf that the tree no longer holds -> DAPOL_ERR_UNKNOWN_LEAF,
 * nothing written.
 *   When to use it (tools/bench_batch_store.py): whenever batch proofs are served after edits and the caller
 * does not need every blob back after every edit.  2^16 leaves at height 32, 4,096 batches of 2 / 4 random leaves, 64-bit proofs, one
 * MI355X, 1 to 4,096 replaced liabilities, refresh + fetch of 256 rows against the whole dapol_reprove_batches call on the same edited
 * tree: the gain is the bus trip, 6-20 ms a call -- padding / 16 0.067-0.142 -> 0.059-0.122 s (x1.10-1.29), splitting / 24 0.070-0.148
 * -> 0.064-0.132 s (x1.07-1.20), padding / 0 0.018-0.129 -> 0.010-0.109 s (x1.14-2.5); refresh + read of everything x1.05-1.55.
 *   Left out: shard trees, 64-byte digests, tape mode, persistence (a store lives and dies with its process), compact forms (DESIGN.md
 * section 9). */
typedef struct dapol_batch_store dapol_batch_store;
int32_t dapol_batch_store_create(dapol_ctx* ctx, dapol_tree* tree, int32_t policy, int32_t aggregation_factor, int32_t n_bits,
                                 const uint8_t nonce_seed32[32], dapol_batch_store** store);
int32_t dapol_batch_store_destroy(dapol_batch_store* store);
int32_t dapol_batch_store_refresh(dapol_batch_store* store, size_t nb, const uint64_t* batch_off, const uint64_t* leaf_idx, uint64_t* proved,
                                  uint64_t* kept, uint64_t* n_calls, uint64_t* moved_rows);
size_t dapol_batch_store_rows(dapol_batch_store* store);
int32_t dapol_batch_store_layout(dapol_batch_store* store, uint64_t* batch_off, uint64_t* leaf_idx, uint64_t* sib_off, uint64_t* range_off);
int32_t dapol_batch_store_fetch(dapol_batch_store* store, size_t k, const uint64_t* row, uint8_t* sib_C32, uint8_t* sib_H32, uint8_t* range_out);
int32_t dapol_batch_store_read(dapol_batch_store* store, size_t first, size_t count, uint8_t* sib_C32, uint8_t* sib_H32, uint8_t* range_out);
int32_t dapol_batch_store_verify(dapol_batch_store* store, const uint8_t verify_seed32[32], uint8_t* ok);

/* SHARED sub-proofs on the verifier's side -- the counterpart of dapol_prove_entities_shared: a call that checks many entities'
 * proofs (an exchange before it publishes them, an auditor who checks everyone's) verifies every run of equal sub-proofs once.
 * Arguments, refusals and error codes as dapol_verify_entities_checked / dapol_verify_entities (shared or per-entity blobs, decoded
 * wires and 64-byte digests go in unchanged), plus *unique_subproofs_out (may be NULL).
 *   Definition.  For sub-proof s = {start, count, m} of the policy's plan, row e REPEATS row e - 1 iff (1) the sub-proof's bytes in
 * the two blobs are equal and (2) the `count` sibling commitments path_C32[e][start .. start + count) equal those of row e - 1.
 * That is everything the range check of the sub-proof reads (the pad parties are constants; node hashes are not read).  A row
 * that does not repeat its predecessor is a HEAD; row 0 always is one.  Every head is verified once, a repeating row receives the
 * verdict of the head of its run.  ok[e] = the Merkle re-merge of entity e (per entity, unchanged) AND the verdicts of its
 * sub-proofs.  *unique_subproofs_out = the number of heads = range proofs actually checked.
 *   It works for any input: no keys, no trust in the leaf indexes and no ordering requirement -- adjacent equal bytes are the only
 * thing that is shared, so unsorted or per-entity blobs only share less and the result is still dapol_verify_entities' verdict
 * vector.  The verdict vector is the per-proof one, as everywhere in the verifier: the compact batch goes through the same random
 * linear combination with its eight-way split fallback, so a bad copy never drags a good neighbour down (a copy and its original
 * get the same verdict because the verdict is a function of the bytes; the combination's soundness error of about 2^-250 is the
 * one exception).  The verifier's scalars are bound to the compact batch: their digest covers every distinct proof and commitment.
 *   Errors and limits.  Length mismatches (n_path_nodes, range_proofs_len) -> ok = 0, *unique = 0, DAPOL_OK.  A bad policy /
 * aggregation_factor / n_bits, or more parties than the context has -> DAPOL_ERR_INVALID_ARGUMENT.  b = 0 is DAPOL_OK with
 * *unique = 0.  b x (plan size + 1) must stay below 2^32 (DAPOL_ERR_INVALID_ARGUMENT above).  Calls with b x plan size <= 64 --
 * the latency regime, where there is nothing to gain -- forward to dapol_verify_entities and report *unique = b x plan size (a test-only override,
 * DAPOL_VSHARED_FORWARD_MAX behind DAPOL_ENV_KNOBS and DAPOL_TEST_HOOKS, moves that limit).
 *   When to use it (tools/bench_verify_shared.py): the time of a call is its upload (which sharing cannot
 * shrink), the per-entity Merkle re-merge, and range checks that follow the sum of m over the distinct rows instead of over all rows.
 * The tool prints all three per shape; its numbers are not measured yet on an MI355X, so no ratio is claimed here: until they are,
 * treat this entry point as experimental and prefer dapol_verify_entities.  What the shared
 * call adds where nothing repeats is one pass over the uploaded blobs (compare), a scan and a gather of every row. */
int32_t dapol_verify_entities_shared(dapol_ctx* ctx, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32, const uint8_t* leaf_H32,
                                     size_t n_path_nodes, const uint8_t* path_C32, const uint8_t* path_H32, const uint8_t root_C32[32],
                                     const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t* range_proofs,
                                     size_t range_proofs_len, const uint8_t verify_seed32[32], uint8_t* ok, uint64_t* unique_subproofs_out);

/* dapol_verify_entities_compact: the verifier over the COMPACT form (above, "COMPACT shared proofs"): every distinct sub-proof is
 * uploaded once.  Arguments as dapol_verify_entities_shared with (compact, compact_len) in place of (range_proofs, range_proofs_len).
 * leaf_idx must be strictly increasing (DAPOL_ERR_INVALID_ARGUMENT otherwise); a wrong n_path_nodes, or a compact_len that is not the
 * layout's length for these leaves, gives ok = 0, *unique = 0 and DAPOL_OK.
 *   Definition.  ok[] equals what dapol_verify_entities returns for the same leaves, paths and root with dapol_shared_expand(compact)
 * as the blobs -- for every input, tampered ones included.  Nothing but bytes is trusted: row e of sub-proof s = {start, count, m} is a
 * HEAD iff e = 0, or its subtree key differs from row e - 1's, or any of the `count` sibling commitments the sub-proof covers differs
 * from row e - 1's.  A head is checked once, against its own row's commitments, with the proof at compact row ref[s][e] of s; the
 * rows behind it up to the next head inherit its verdict (they name the same proof bytes over the same commitments).
 * *unique_subproofs_out = the number of heads; on honest input that is dapol_shared_plan's total.  A corrupted row therefore fails
 * alone and does not take honest rows of the same subtree with it: the verdict vector is the per-proof one, through the same random
 * linear combination with its eight-way split as everywhere in the verifier.
 *   Limits as dapol_verify_entities_shared; calls with b x plan size <= 64 expand on the host, forward to dapol_verify_entities and
 * report *unique = b x plan size (the same test-only override moves that limit).
 *   When to use it (tools/bench_shared_compact.py, DESIGN.md section 4.6, profiles/shared_compact_2e18_h30.json: 2^18 random leaves at
 * height 30, 64-bit proofs, one MI355X, whole calls against dapol_verify_entities fed the expansion): padding / 16 0.398 -> 0.336 s
 * (x1.18), splitting / 24 0.243 -> 0.213 s (x1.14), padding / 0 0.756 -> 0.341 s (x2.22); the time follows the number of range proofs
 * checked, the upload (14-16 % of a call there) shrinks by the byte ratio.  Where nothing is shared (padding / height) 0.088 -> 0.089 s:
 * either call serves. */
int32_t dapol_verify_entities_compact(dapol_ctx* ctx, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32, const uint8_t* leaf_H32,
                                      size_t n_path_nodes, const uint8_t* path_C32, const uint8_t* path_H32, const uint8_t root_C32[32],
                                      const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor, int32_t n_bits, const uint8_t* compact,
                                      size_t compact_len, const uint8_t verify_seed32[32], uint8_t* ok, uint64_t* unique_subproofs_out);

/* COMPACT Merkle paths: every distinct sibling of a call's paths leaves the prover and enters the verifier ONCE.
 *   The form.  For strictly increasing leaf_idx [b] below 2^height, H = height in 1 .. 64: key_d(e) = leaf_idx[e] >> (H - d) for
 * d = 1 .. H and key_0 = 0.  The sibling of row e at depth d is the node (d, key_d(e) ^ 1): rows that share key_d share it.  Row e is a
 * HEAD at depth d iff e = 0 or key_d(e) != key_d(e - 1); a head at d is a head at every deeper depth.  The COMPACT PATH BUFFER is laid
 * out for d = 1 .. H, root side first, ALWAYS (it does not depend on dapol_wire_config.siblings_leaf_first): for each depth the
 * n_unique[d] records (C [32], H [hash_bytes]) of the siblings of the distinct keys of depth d, in ascending key order, as two arrays
 * cpath_C32 [n_records][32] and cpath_H [n_records][hash_bytes].  depth_off[d] = the record offset of depth d (depth_off[0] =
 * depth_off[1] = 0, depth_off[H + 1] = n_records), ref[d][e] = (distinct keys of depth d among rows 0 .. e) - 1.  Expansion gives
 * dapol_tree_paths' [b][H] arrays, and it is the expansion that honours siblings_leaf_first.  A sibling that is also an ancestor of
 * another row is still a record: this is deduplication, not a multiproof, and the per-entity meaning of a path does not change.
 *   Host-only (no GPU, no context):
 *   dapol_compact_paths_plan: depth_off [height + 2], ref [height][b] (ref[(d - 1) * b + e]), *n_records; every out pointer may be NULL.
 *   dapol_compact_paths_expand: rows [first, first + count) as path_C32_out [count][height][32], path_H_out [count][height][hash_bytes];
 * count = 1 cuts one user's path out.
 *   dapol_compact_paths_compress: the inverse; it writes the first row of every run and does not read the other rows.
 *   Refusals: indexes that are not strictly increasing or not below 2^height, hash_bytes other than 32 or 64, an n_records that is not
 * the layout's, first + count > b, a cap_records below the layout's -> DAPOL_ERR_INVALID_ARGUMENT with nothing written.  b = 0 is
 * DAPOL_OK with n_records = 0.
 *   dapol_tree_paths_compact: the compact buffer of the paths of b leaves, written from the tree's levels on the device: every row
 * walks its chain as dapol_tree_paths does and stores a record only at the depths at which it is a head.  No [b][H] array exists on
 * the device and only the records cross the bus.  cpath_H32 holds dapol_ctx_digest_bytes per record.  The length is checked on the
 * host before anything is queued (cap_records below it -> DAPOL_ERR_INVALID_ARGUMENT); an unknown leaf -> DAPOL_ERR_UNKNOWN_LEAF;
 * nothing is written in either case.  dapol_compact_paths_expand of the output equals dapol_tree_paths' (C, H) byte for byte.  The
 * provers accept path_C32 = path_H32 = NULL: a caller that wants compact paths passes NULL there and calls this.  Plain trees only (no
 * n_upper: a shard's upper siblings are one record each, which the caller can prepend).
 *   dapol_verify_entities_compact_paths: dapol_verify_entities_compact over compact paths.
 *   Definition.  ok[] equals what dapol_verify_entities_compact returns for the same leaves, root and compact proofs with
 * dapol_compact_paths_expand(cpath) as the paths -- for every input, tampered ones included.  A wrong n_records or compact_len gives
 * ok = 0, both counters 0 and DAPOL_OK; indexes that are not strictly increasing and below 2^height give DAPOL_ERR_INVALID_ARGUMENT,
 * as does a context with a 64-byte node digest.  Calls with b x plan size <= 64 expand on the host, forward to
 * dapol_verify_entities_compact and report *path_merges_out = b x height.
 *   Every distinct node (d, key) of the call's paths is merged with its record once: canonically where the head row of (d, key) is
 * also the head row of its parent (the result, extended point included, becomes the parent's value: a point this call has made is
 * never decoded again), as a JOIN where it is not (the result is compared, C and H, with the parent's canonical value).  If every
 * decoding succeeds, every join matches and row 0's chain ends in the root, every per-entity chain is the same function of the same
 * inputs as a chain that was checked, and every path verifies: *path_merges_out = n_records.  Otherwise the paths are expanded on the
 * device and the per-entity re-merge of dapol_verify_entities runs over them as it is (a non-canonical record fails exactly the rows
 * whose own path holds it; a join that fails says nothing about which of its two rows is wrong): *path_merges_out = n_records +
 * b x height.  The range proofs take the compact verifier's groups; a statement's commitments are read from the records that its
 * head row walks, so equal subtree keys imply equal commitments and *unique_subproofs_out = dapol_shared_plan's total on any input.
 *   dapol_diag_compact_paths: device time of the path stage of the last such call on any context (events around its path launches)
 * and its route (0 forwarded, 1 shared merges, 2 shared merges then the fallback, 3 the fallback alone -- a test knob).
 *   When to use it (tools/bench_compact_paths.py, DESIGN.md section 4.6, profiles/compact_paths_2e18_h30.json: 2^18 leaves at height
 * 30, 64-bit proofs, one MI355X, whole calls against dapol_verify_entities_compact fed the expanded paths): random leaves, x2.29 fewer
 * records: padding / 30 0.102 -> 0.085 s (x1.19), padding / 16 0.378 -> 0.326 s (x1.16), padding / 0 0.383 -> 0.329 s (x1.17);
 * consecutive leaves, x15 fewer records: 0.101 -> 0.074 s, 0.089 -> 0.057 s, 0.091 -> 0.059 s.  The path stage itself: 16.8 ms per
 * entity -> 10.4 ms (random) / 5.4 ms (consecutive) shared.  dapol_tree_paths_compact against dapol_tree_paths: 10.9 -> 10.0 ms and
 * 503 -> 220 MB returned (random), 10.8 -> 3.0 ms and 503 -> 34 MB (consecutive).  It gains at every aggregation factor, padding /
 * height included; a call in which anything fails to verify pays the shared merges and then the per-entity ones. */
int32_t dapol_compact_paths_plan(int32_t height, size_t b, const uint64_t* leaf_idx, uint64_t* depth_off, uint32_t* ref, uint64_t* n_records);
int32_t dapol_compact_paths_expand(int32_t hash_bytes, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* cpath_C32, const uint8_t* cpath_H,
                                   size_t n_records, size_t first, size_t count, uint8_t* path_C32_out, uint8_t* path_H_out);
int32_t dapol_compact_paths_compress(int32_t hash_bytes, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* path_C32, const uint8_t* path_H,
                                     uint8_t* cpath_C32_out, uint8_t* cpath_H_out, size_t cap_records, uint64_t* n_records_out);
int32_t dapol_tree_paths_compact(dapol_tree* tree, size_t b, const uint64_t* leaf_idx, uint8_t* cpath_C32, uint8_t* cpath_H32, size_t cap_records,
                                 uint64_t* n_records_out);
int32_t dapol_verify_entities_compact_paths(dapol_ctx* ctx, int32_t height, size_t b, const uint64_t* leaf_idx, const uint8_t* leaf_C32,
                                            const uint8_t* leaf_H32, size_t n_records, const uint8_t* cpath_C32, const uint8_t* cpath_H32,
                                            const uint8_t root_C32[32], const uint8_t root_H32[32], int32_t policy, int32_t aggregation_factor,
                                            int32_t n_bits, const uint8_t* compact, size_t compact_len, const uint8_t verify_seed32[32], uint8_t* ok,
                                            uint64_t* unique_subproofs_out, uint64_t* path_merges_out);
int32_t dapol_diag_compact_paths(double* path_ms, int32_t* route);

/* Multi-GPU: one process per GPU, rank g owning the top-level subtree with index prefix g (dapol_tree_build_shard /
 * dapol_workload_create_shard).  The reference has no communication (single process, single thread); the sharded path has
 * exactly one exchange step and one final reduce, both RCCL calls inside this library (librccl.so, over xGMI):
 *   dapol_comm_unique_id   rank 0 makes the 128-byte RCCL id; the host distributes it by whatever means it has
 *   dapol_comm_create      the communicator on the context's GPU (world must be a power of two), created NON-BLOCKING
 *                          (ncclCommInitRankConfig, blocking = 0) and polled with ncclCommGetAsyncError.
 *   dapol_comm_create_timeout  ... up to a deadline: a communicator that has not come up after timeout_ms is aborted
 *                          (ncclCommAbort) and the call returns DAPOL_ERR_COMM, so that one absent rank cannot hang the others
 *                          inside ncclCommInitRank for good; timeout_ms <= 0 waits without a deadline.  The communicator keeps
 *                          the deadline for its COLLECTIVES: a dapol_shard_exchange / dapol_comm_allreduce_u64 that has not
 *                          completed after timeout_ms, or during which RCCL reports an asynchronous error, aborts the
 *                          communicator (which ends an RCCL kernel waiting for a peer), returns DAPOL_ERR_COMM, and every
 *                          later call on the handle fails at once -- the host falls back to another transport or exits.
 *   dapol_comm_abort       the failure path (ncclCommAbort): tear down without waiting for the peers, once the ranks have
 *                          agreed not to use this communicator; dapol_comm_destroy is the orderly end (finalize + destroy).
 *   dapol_comm_count       the number of ranks as RCCL reports it (ncclCommCount)
 *   dapol_shard_exchange   ncclAllGather of the G subtree-root records (C | H | v LE64 | r = 104 bytes each; an empty shard
 *                          sends the padding node of its root position, dapol_padding_nodes), then every rank merges the
 *                          log2 G replicated top levels on its own GPU (Mergeable::merge) -> the global root record and the
 *                          upper siblings of this rank, root side first, ready for dapol_prove_entities_upper /
 *                          dapol_workload_prove.  records_out (may be NULL): the gathered [world][104] records.
 *   dapol_comm_allreduce_u64  ncclAllReduce over 64-bit words: the final reduce of the per-rank proof checksums (wrapping
 *                          sum), proof counts, or verdict masks (min = AND of 0/1 verdicts).
 *   dapol_shard_top_levels the merge half alone, for records gathered by other means (tests, other transports). */
typedef struct dapol_comm dapol_comm;
enum { DAPOL_COMM_ID_BYTES = 128, DAPOL_RECORD_BYTES = 104 };
enum { DAPOL_REDUCE_SUM = 0, DAPOL_REDUCE_MIN = 1, DAPOL_REDUCE_MAX = 2 };
int32_t dapol_comm_unique_id(uint8_t id_out[DAPOL_COMM_ID_BYTES]);
int32_t dapol_comm_create(dapol_ctx* ctx, const uint8_t id[DAPOL_COMM_ID_BYTES], int32_t rank, int32_t world, dapol_comm** out);
int32_t dapol_comm_create_timeout(dapol_ctx* ctx, const uint8_t id[DAPOL_COMM_ID_BYTES], int32_t rank, int32_t world, int64_t timeout_ms, dapol_comm** out);
int32_t dapol_comm_destroy(dapol_comm* comm);
int32_t dapol_comm_abort(dapol_comm* comm);
int32_t dapol_comm_count(dapol_comm* comm, int32_t* count);
int32_t dapol_shard_exchange(dapol_comm* comm, const uint8_t sub_C[32], const uint8_t sub_H[32], uint64_t sub_v, const uint8_t sub_r[32],
                             uint8_t root_C[32], uint8_t root_H[32], uint64_t* root_v, uint8_t root_r[32], uint8_t* up_C32, uint8_t* up_H32,
                             uint64_t* up_v, uint8_t* up_r32, uint8_t* records_out);
int32_t dapol_shard_top_levels(dapol_ctx* ctx, int32_t world, int32_t rank, const uint8_t* records, uint8_t root_C[32], uint8_t root_H[32],
                               uint64_t* root_v, uint8_t root_r[32], uint8_t* up_C32, uint8_t* up_H32, uint64_t* up_v, uint8_t* up_r32);
int32_t dapol_comm_allreduce_u64(dapol_comm* comm, int32_t op, uint64_t* inout, size_t n);
/* What the two collectives cost, measured inside the calls above (a multi-GPU bench line carries them per step, so that a scaling
 * curve can be read from its own records): DEVICE time between HIP events on the context's stream around ncclAllGather -- which
 * includes waiting for the slowest rank to arrive -- around the replicated merge of the top levels with its copies back, and
 * around ncclAllReduce; HOST wall time of each whole call.  Microseconds; last_* = the most recent call, sum_* since creation or
 * the last reset (reset != 0 clears the counters after copying them out). */
typedef struct {
    uint64_t exchanges, reduces;
    double last_allgather_us, last_top_levels_us, last_exchange_host_us, last_allreduce_us, last_reduce_host_us;
    double sum_allgather_us, sum_top_levels_us, sum_exchange_host_us, sum_allreduce_us, sum_reduce_host_us;
} dapol_comm_timing;
int32_t dapol_comm_timing_get(dapol_comm* comm, dapol_comm_timing* out, int32_t reset);

/* generate_proof_batch (src/dapol/mod.rs:172-190) on a SHARDED tree.  The siblings of a batch lie in several shards and in
 * the replicated top levels, so the proof is assembled from node RECORDS (C, H, v, r):
 *   dapol_batch_siblings            the positions (level above the leaves, index) of the proof's siblings;
 *   dapol_tree_node_records         this rank's records among them: the real or padding node a (shard) tree stores at each
 *                                   position, found[i] = 0 where the tree holds none (another shard's, or above the shard root);
 *   dapol_shard_top_node_records    the nodes at and above the shard roots (level_above = 0 .. log2 G), from the G exchanged
 *                                   subtree-root records;
 *   dapol_prove_batch_records       R::generate_proof over the assembled siblings, in dapol_batch_siblings' order.
 * Between the second and the last step the ranks exchange their 104-byte rows by any transport.  The result equals
 * dapol_prove_batch on the unsharded tree byte for byte.  dapol_workload_tree lends a workload's current (sub)tree to these
 * calls (valid until the workload's next build / destroy; do not destroy it). */
int32_t dapol_tree_node_records(dapol_tree* tree, size_t n, const uint8_t* level, const uint64_t* index, uint8_t* C32, uint8_t* H32,
                                uint64_t* v, uint8_t* r32, uint8_t* found);
int32_t dapol_shard_top_node_records(dapol_ctx* ctx, int32_t world, const uint8_t* records, size_t n, const uint8_t* level_above,
                                     const uint64_t* index, uint8_t* C32, uint8_t* H32, uint64_t* v, uint8_t* r32);
int32_t dapol_prove_batch_records(dapol_ctx* ctx, size_t k, const uint64_t* leaf_idx, size_t n_siblings, const uint8_t* sib_C32,
                                  const uint64_t* sib_v, const uint8_t* sib_r32, int32_t policy, int32_t aggregation_factor,
                                  int32_t n_bits, const uint8_t nonce_seed32[32], uint8_t* range_out);

/* Bench / roofline support: device-resident variant of build + prove-all used by bench.py so that the timed
 * region starts with inputs already in HBM and nothing is copied back.  Handles are opaque device buffers. */
typedef struct dapol_workload dapol_workload;
int32_t dapol_workload_create(dapol_ctx* ctx, int32_t height, size_t n, const uint64_t* leaf_idx, const uint64_t* v,
                              const uint8_t* r32, dapol_workload** out);
/* Sharded variant: this GPU holds the leaves of one top-level subtree (see dapol_tree_build_shard). */
int32_t dapol_workload_create_shard(dapol_ctx* ctx, int32_t total_height, int32_t shard_bits, size_t n, const uint64_t* leaf_idx,
                                    const uint64_t* v, const uint8_t* r32, dapol_workload** out);
int32_t dapol_workload_destroy(dapol_workload* w);
int32_t dapol_workload_tree(dapol_workload* w, dapol_tree** out);    /* borrowed: the tree of the last dapol_workload_build */
/* One pass: tree build + one padding-policy inclusion range proof per entity (aggregation_factor = height).
 * Returns device time of the two phases in milliseconds (HIP events on the ctx stream), the time and launch
 * count of the dominant kernel (the fixed-base MSM), and a 64-bit checksum of all proof bytes + the root. */
typedef struct {
    double tree_ms, prove_ms, msm_ms;
    uint64_t msm_launches, proofs, proof_bytes;
    uint64_t checksum;
    uint8_t root_C[32], root_H[32];
    /* (appended in round 3; the fields above keep their offsets)  msm_ms / msm_launches bracket the PLAIN fixed-base MSMs (S
     * commitment + never-fold rounds), mat_ms / mat_launches the materialisation of the folded generators; *_kernels = launches
     * of the dominant kernel inside those brackets (a generator-stationary MSM is a few hundred tile launches of k_rp_msm_gs). */
    double mat_ms;
    uint64_t mat_launches, msm_kernels, mat_kernels;
    double msm_all_ms;      /* time with a bracket of either kind open (msm_ms / mat_ms / this are UNIONS of the bracket intervals:
                             * two chunks are in flight on two streams and their brackets overlap) */
    double msm_span_ms;     /* SUM of the plain brackets' lengths: what a per-kernel profiler adds up for launches that overlap in time */
} dapol_workload_stats;
int32_t dapol_workload_run(dapol_workload* w, const uint8_t pad_seed32[32], const uint8_t nonce_seed32[32], int32_t n_bits,
                           size_t first_entity, size_t n_entities, dapol_workload_stats* stats);
/* The two halves of dapol_workload_run, so that the subtree-root exchange can sit between them: build returns the
 * (sub)tree root record; prove takes the siblings above it (n_upper may be 0).  Both fill their part of *stats. */
int32_t dapol_workload_build(dapol_workload* w, const uint8_t pad_seed32[32], uint8_t root_C[32], uint8_t root_H[32], uint64_t* root_v,
                             uint8_t root_r[32], dapol_workload_stats* stats);
int32_t dapol_workload_prove(dapol_workload* w, const uint8_t nonce_seed32[32], int32_t n_bits, size_t first_entity, size_t n_entities,
                             int32_t n_upper, const uint8_t* up_C32, const uint8_t* up_H32, const uint64_t* up_v, const uint8_t* up_r32,
                             dapol_workload_stats* stats);
/* dapol_workload_prove under either policy / any aggregation factor (the reference's bench also times RangeProofSplitting,
 * benches/dapol.rs:71-78); dapol_workload_prove = (DAPOL_POLICY_PADDING, height). */
int32_t dapol_workload_prove_policy(dapol_workload* w, const uint8_t nonce_seed32[32], int32_t n_bits, size_t first_entity, size_t n_entities,
                                    int32_t policy, int32_t aggregation_factor, int32_t n_upper, const uint8_t* up_C32, const uint8_t* up_H32,
                                    const uint64_t* up_v, const uint8_t* up_r32, dapol_workload_stats* stats);
/* Siblings of sampled leaves of the last build, with the upper siblings prepended: [b][n_upper+levels].  (v, r) are the
 * secrets handed to the range prover; (C, H) the Merkle path proof nodes.  Output / upper pointers may be NULL in pairs. */
int32_t dapol_workload_paths(dapol_workload* w, size_t b, const uint64_t* leaf_idx, int32_t n_upper, const uint64_t* up_v,
                             const uint8_t* up_r32, const uint8_t* up_C32, const uint8_t* up_H32, uint64_t* sib_v, uint8_t* sib_r32,
                             uint8_t* sib_C32, uint8_t* sib_H32);
/* Copies back the proofs of entities [first, first+count) of the last run (count*proof_size bytes). */
int32_t dapol_workload_proofs(dapol_workload* w, size_t first, size_t count, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* DAPOL_HIP_H */
