/*
 * qpgpu.h — C ABI of the MI355X (gfx950) Plonky2 prover backend.
 *
 * The reference (aletheia-labs/qp-zk-circuits-rm) has no FFI: its hot path is
 * the Rust crate qp-plonky2 1.1.1 called from qp-wormhole-prover.  Each entry
 * point below names the plonky2 routine it replaces and the reference call
 * site that reaches it.  A Rust binding is a
 * `[patch.crates-io]` qp-plonky2 whose routines call these functions
 * (INTEGRATION.md).
 *
 * Conventions
 *   - Field elements are canonical Goldilocks u64 (p = 2^64 - 2^32 + 1);
 *     extension elements are (c0, c1) pairs, X^2 = 7.
 *   - Host buffers are caller-owned and only borrowed for the call.  Device
 *     objects (qp_ctx, qp_batch, qp_prover) are opaque handles released by
 *     their _free / _destroy function.
 *   - `_dev` variants take device pointers and run on the context's stream
 *     without synchronising (inputs already resident in HBM).
 *   - Every function returns a qp_status; it never aborts or throws across
 *     the ABI.  qp_ctx_last_error() gives the message of the last failure.
 *   - A qp_ctx is single-thread-affine (one HIP stream); concurrent callers
 *     use distinct contexts, which are independent.
 */
#ifndef QPGPU_H
#define QPGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    QP_OK = 0,
    QP_ERR_ARG = 1,      /* bad shape / null pointer / out-of-range index */
    QP_ERR_HIP = 2,      /* HIP runtime error (no device, launch failure) */
    QP_ERR_OOM = 3,      /* device allocation failed */
    QP_ERR_STATE = 4,    /* call order violated (e.g. prove before commit) */
    QP_ERR_WITNESS = 5,  /* witness conflict ("set twice with different values") or unsatisfied */
    QP_ERR_FORMAT = 6    /* malformed serialized input */
} qp_status;

typedef struct qp_ctx qp_ctx;
typedef struct qp_batch qp_batch;

/* ---- context ---------------------------------------------------------- */
int qp_ctx_create(int device, qp_ctx **out);
void qp_ctx_destroy(qp_ctx *ctx);
const char *qp_ctx_last_error(const qp_ctx *ctx);
/* run subsequent work on an external HIP stream (e.g. torch's); NULL = own stream */
int qp_ctx_set_stream(qp_ctx *ctx, void *hip_stream);
int qp_ctx_synchronize(qp_ctx *ctx);
/* re-create the context's own stream at the device's greatest stream priority
 * (high != 0) or the default one; call before any work is queued on it */
int qp_ctx_set_priority(qp_ctx *ctx, int high);
/* library build/version string */
const char *qp_version(void);

/* ---- PolynomialBatch (plonky2 fri/oracle.rs) ----------------------------
 * Replaces PolynomialBatch::from_values (ifft -> coset LDE -> transpose ->
 * reverse_index_bits -> MerkleTree::new).  Reached from
 * WormholeProver::prove (wormhole/prover/src/lib.rs:233-237) for the wires,
 * zs/partial-products and quotient commitments, and from
 * WormholeProver::new -> CircuitBuilder::build (lib.rs:190-202) for the
 * constants/sigmas commitment.
 *   values: column-major [npolys][2^log_n]; salt: row-major [N][nsalt] (may be
 *   NULL when nsalt == 0), N = 2^(log_n+rate_bits).
 *   coeffs_out (optional): [npolys][2^log_n]; cap_out: [2^cap_height][4].
 *   out (optional): keeps the LDE matrix + tree resident for openings.     */
int qp_commit_values(qp_ctx *ctx, const uint64_t *values, uint32_t npolys, uint32_t log_n, uint32_t rate_bits,
                     uint32_t cap_height, const uint64_t *salt, uint32_t nsalt, uint64_t *coeffs_out,
                     uint64_t *cap_out, qp_batch **out);
/* PolynomialBatch::from_coeffs (quotient chunks) — same, from coefficients */
int qp_commit_coeffs(qp_ctx *ctx, const uint64_t *coeffs, uint32_t npolys, uint32_t log_n, uint32_t rate_bits,
                     uint32_t cap_height, const uint64_t *salt, uint32_t nsalt, uint64_t *cap_out, qp_batch **out);
/* device-resident variant: d_values [nbat][npolys][n] on the device; d_cap_out
 * [nbat][2^cap_h][4] on the device; no host sync.  Batches are independent
 * polynomial batches of identical shape (one per proof).                   */
int qp_commit_values_dev(qp_ctx *ctx, const uint64_t *d_values, uint32_t nbat, uint32_t npolys, uint32_t log_n,
                         uint32_t rate_bits, uint32_t cap_height, uint64_t *d_cap_out, qp_batch **out);

/* MerkleTree::get + MerkleTree::prove for a list of leaf indices:
 * leaves_out [nidx][npolys+nsalt], siblings_out [nidx][log_N - cap_h][4]    */
int qp_batch_open(qp_batch *b, const uint32_t *leaf_idx, uint32_t nidx, uint64_t *leaves_out,
                  uint64_t *siblings_out);
/* copies the LDE matrix, leaf order, column-major [npolys][N] (tests) */
int qp_batch_lde(qp_batch *b, uint64_t *out);
/* copies the coefficients [npolys][n] */
int qp_batch_coeffs(qp_batch *b, uint64_t *out);
void qp_batch_free(qp_batch *b);

/* ---- primitives (plonky2 field/fft.rs, hash/poseidon.rs) ----------------- */
/* PolynomialValues::ifft for ncols columns, in place, column-major          */
int qp_ifft(qp_ctx *ctx, uint64_t *data, uint32_t ncols, uint32_t log_n);
/* PolynomialCoeffs::lde(rate_bits).coset_fft(shift), output in Merkle-leaf
 * (bit-reversed) row order, column-major [ncols][N]                         */
int qp_lde(qp_ctx *ctx, const uint64_t *coeffs, uint32_t ncols, uint32_t log_n, uint32_t rate_bits, uint64_t shift,
           uint64_t *out);
/* Poseidon permutation of n 12-element states, in place                   */
int qp_poseidon_permute(qp_ctx *ctx, uint64_t *states, uint64_t n);
/* PoseidonHash::hash_no_pad on the host (no device): used to build circuit
 * inputs (nullifier, unspendable account, storage-proof roots)            */
int qp_hash_no_pad(const uint64_t *in, size_t n, uint64_t *out4);


/* ---- circuits and witnesses (host; no device needed) ---------------------
 * Native equivalent of plonky2's CircuitBuilder::build / build_prover and
 * generate_partial_witness for the reference circuits.                     */
typedef struct qp_circuit qp_circuit;
typedef struct qp_witness qp_witness;

/* CircuitInputs (wormhole/circuit/src/inputs.rs:25-52) in byte form */
typedef struct {
    uint8_t funding_amount[16];        /* u128, little-endian */
    uint8_t nullifier[32];
    uint8_t root_hash[32];
    uint8_t exit_account[32];
    uint8_t secret[32];
    uint64_t transfer_count;
    uint8_t funding_account[32];
    uint8_t unspendable_account[32];
    uint32_t num_nodes;                /* storage proof length (<= 20) */
    const uint8_t *const *nodes;       /* node byte strings */
    const uint32_t *node_lens;
    const uint64_t *indices;           /* hex-character child-hash indices */
    /* values of the PublicInputGate row's unused wires 4..num_wires-1
     * (num_wires - 4 canonical felts), which the reference fills from
     * RandomValueGenerator (plonky2 CircuitBuilder::build,
     * randomize_unused_pi_wires; qp-plonky2 under both configs).  Passing the
     * values a reference proof holds reproduces that proof's wires.  NULL =
     * zeros under standard_recursion_config; under the zk config derived
     * deterministically from the private inputs (a Poseidon nonce; DESIGN.md
     * "zk").                                                                 */
    const uint64_t *zk_randomness;
} qp_wormhole_inputs;

/* WormholeCircuit::new(config) + build_prover (wormhole/circuit/src/circuit.rs:76-108,
 * wormhole/prover/src/lib.rs:190-202) — host part.  zero_knowledge selects
 * standard_recursion_zk_config vs standard_recursion_config.  Under the
 * workspace's `no_random` feature the two share the preprocessing and proof
 * shape (no salt columns; tests/test_current_circuit_fixture.py) and both
 * fill the PublicInputGate row's spare cells (qp_wormhole_inputs.zk_randomness);
 * the constants||sigmas columns equal the reference's
 * (tests/test_reference_layout.py).                                        */
int qp_wormhole_circuit_new(int zero_knowledge, qp_circuit **out);
void qp_circuit_free(qp_circuit *c);
/* info[0..6] = degree_bits, num_wires, num_routed_wires, num_constants,
 *              num_public_inputs, gates used (before padding), num_gate_constraints
 * info[7..8] = witness generators, dependency levels of the device schedule
 * (info must hold 9 words)                                                  */
int qp_circuit_info(const qp_circuit *c, uint32_t *info);
/* generator and gate-row census: gens[k] = generators of GenKind k (constant,
 * arithmetic, Poseidon, BaseSum split, equality, wire split, extension
 * division, RandomAccess, ArithmeticExtension, MulExtension, Reducing,
 * ReducingExtension, PoseidonMds, CosetInterpolation: 14 words); rows[k] =
 * gate rows of kind k (noop, constant, public input, BaseSum, arithmetic,
 * Poseidon, RandomAccess, ArithmeticExtension, MulExtension, Reducing,
 * ReducingExtension, PoseidonMds, CosetInterpolation: 13 words; the n rows
 * of the trace, padding counted as noop); level_gens (may be null; 14 words
 * per device-witness level, info word 8 levels) = the generators of each
 * dependency level by kind.  Test/diagnostic entry point.                   */
int qp_circuit_census(const qp_circuit *c, uint32_t *gens, uint32_t *rows, uint32_t *level_gens);
/* the device witness's host part: gens[k] (14 words, GenKind order as above)
 * = generators the host runs before the device schedule (Poseidon chains over
 * inputs alone at least 64 permutations deep -- the public-input hashes and
 * the transcript sponges behind them -- with the constants they read);
 * *slots = value slots set on the host (commit()'s inputs and those chains'
 * outputs); *chains (may be null) = independent chains among them (a batch
 * smaller than the host pool runs them in parallel).  Test/diagnostic entry
 * point.                                                                      */
int qp_circuit_host_chains(const qp_circuit *c, uint32_t *gens, uint32_t *slots, uint32_t *chains);
/* CommonCircuitData::to_bytes (plonky2 util/serialization.rs) */
int qp_circuit_common_data(const qp_circuit *c, uint8_t *out, size_t cap, size_t *len);
/* preprocessed constants||sigmas values over H, [num_constants+num_routed][n] */
int qp_circuit_constants_sigmas(const qp_circuit *c, uint64_t *out);
/* their coefficients (PolynomialValues::ifft per column, host), the polynomials
 * of ProverOnlyCircuitData.constants_sigmas_commitment                     */
int qp_circuit_constants_sigmas_coeffs(const qp_circuit *c, uint64_t *out);
/* ProverOnlyCircuitData::to_bytes through DefaultGeneratorSerializer (the
 * prover.bin of wormhole/circuit-builder/src/lib.rs:53-59, read by
 * WormholeProver::new_from_bytes, prover/src/lib.rs:104-137) of a leaf circuit
 * (Wormhole, voting; QP_ERR_ARG for an aggregation circuit), computed on the
 * host: generators, watch index, the constants||sigmas PolynomialBatch with its
 * Merkle tree, sigmas, subgroup, public inputs, representative map, fft root
 * table, circuit digest.  out == NULL: *len = the size (the bytes are kept until
 * the copying call).  Restated from upstream plonky2; parity unpinned.        */
int qp_circuit_prover_only_bytes(const qp_circuit *c, uint8_t *out, size_t cap, size_t *len);
/* WormholeProver::commit (lib.rs:209-225) + witness generation.  On a witness
 * conflict returns QP_ERR_WITNESS with the reference's message in err.     */
int qp_wormhole_commit(const qp_circuit *c, const qp_wormhole_inputs *in, qp_witness **out, char *err,
                       size_t errcap);
/* VotePublicInputs + VotePrivateInputs (voting/src/lib.rs:26-52), felt form */
typedef struct {
    uint64_t proposal_id[4];
    uint64_t merkle_root[4];
    uint64_t nullifier[4];
    uint8_t vote;                      /* 0 = no, 1 = yes */
    uint64_t private_key[4];
    uint32_t num_siblings;             /* merkle_siblings.len() */
    const uint64_t *siblings;          /* [num_siblings][4] */
    uint32_t num_path_indices;         /* path_indices.len() */
    const uint8_t *path_indices;       /* [num_path_indices], 0 = left, 1 = right */
    uint64_t actual_merkle_depth;
    const uint64_t *zk_randomness;     /* as in qp_wormhole_inputs */
} qp_voting_inputs;

/* VoteTargets::new + VoteCircuitData::circuit + builder.build()
 * (voting/src/lib.rs:71-197, :346-357) — host part.                         */
int qp_voting_circuit_new(int zero_knowledge, qp_circuit **out);
/* VoteCircuitData::fill_targets (voting/src/lib.rs:199-261) + witness
 * generation.  Input validation errors return QP_ERR_ARG and witness
 * conflicts (an invalid Merkle proof or nullifier: plonky2's prove() fails)
 * QP_ERR_WITNESS, both with the reference's message in err.               */
int qp_voting_commit(const qp_circuit *c, const qp_voting_inputs *in, qp_witness **out, char *err, size_t errcap);
/* ---- recursive aggregation (wormhole/aggregator/src/circuits/tree.rs) -----
 * aggregate_chunk's circuit (tree.rs:106-127): a native recursive verifier
 * (plonky2 verify_proof: in-circuit challenger, vanishing polynomial at zeta,
 * FRI with Merkle paths to the caps, coset interpolation, PoW) of nproofs
 * proofs of the circuit whose CommonCircuitData bytes are inner_common (this
 * library's leaf or aggregation circuits), their public inputs registered in
 * order.  Prove it from chunks with qp_prover_prove_aggregation (witness
 * generation on the device) or from host witnesses (qp_aggregation_commit +
 * qp_prover_prove).                                                        */
int qp_aggregation_circuit_new(const uint8_t *inner_common, size_t len, uint32_t nproofs, qp_circuit **out);
/* one aggregate_chunk call's inputs (tree.rs:129-134): verifier_only =
 * VerifierOnlyCircuitData bytes of the inner circuit (cap height u64, cap,
 * circuit digest), proofs = nproofs serialized ProofWithPublicInputs,
 * zk_randomness = the PublicInputGate row's num_wires - 4 random cells (NULL:
 * OS randomness under the zk config, zeros otherwise).                      */
typedef struct {
    const uint8_t *verifier_only;
    size_t vlen;
    const uint8_t *const *proofs;
    const size_t *lens;
    uint32_t nproofs;
    const uint64_t *zk_randomness;
} qp_aggregation_chunk;
/* aggregate_chunk's witness on the host (set_verifier_data_target +
 * set_proof_with_pis_target + generate_partial_witness).  An invalid inner
 * proof fails witness generation (QP_ERR_WITNESS), as plonky2's prove() of the
 * aggregation circuit fails.  zk_randomness: as in qp_aggregation_chunk.    */
int qp_aggregation_commit(const qp_circuit *c, const uint8_t *verifier_only, size_t vlen,
                          const uint8_t *const *proofs, const size_t *lens, uint32_t nproofs,
                          const uint64_t *zk_randomness, qp_witness **out, char *err, size_t errcap);
/* full wire matrix, column-major [num_wires][n] */
int qp_witness_wires(const qp_witness *w, uint64_t *out);
int qp_witness_public_inputs(const qp_witness *w, uint64_t *out, uint32_t cap, uint32_t *n);
void qp_witness_free(qp_witness *w);

/* ---- prover (device) -------------------------------------------------------
 * plonky2 prove() (plonk/prover.rs) for B proofs of one circuit at a time,
 * replacing ProverCircuitData::prove as called by WormholeProver::prove
 * (wormhole/prover/src/lib.rs:233-237) and by the aggregator
 * (wormhole/aggregator/src/circuits/tree.rs:136).  qp_prover_new runs the
 * circuit's device preprocessing (constants/sigmas LDE + Merkle cap, circuit
 * digest: CircuitBuilder::build) and sizes the workspace for max_batch proofs.
 * Proof bytes follow ProofWithPublicInputs::to_bytes; the PoW witness is the
 * minimal one, so proofs are a deterministic function of the witness.      */
typedef struct qp_prover qp_prover;
int qp_prover_new(qp_ctx *ctx, const qp_circuit *c, uint32_t max_batch, qp_prover **out);
void qp_prover_free(qp_prover *p);
int qp_prover_proof_size(const qp_prover *p, size_t *len);
/* VerifierOnlyCircuitData || CommonCircuitData bytes (cap height, constants/sigmas
 * cap, circuit digest, common data) — the wormhole/bench-data/verifier.bin layout */
int qp_prover_verifier_data(const qp_prover *p, uint8_t *out, size_t cap, size_t *len);
/* prove from witnesses made by qp_wormhole_commit; proof b at out + b*stride */
int qp_prover_prove(qp_prover *p, const qp_witness *const *w, uint32_t nproofs, uint8_t *out, size_t stride,
                    size_t *lens);
/* prove from raw wire matrices [nproofs][num_wires][n] + public inputs [nproofs][npis] */
int qp_prover_prove_wires(qp_prover *p, const uint64_t *wires, const uint64_t *pis, uint32_t nproofs, uint8_t *out,
                          size_t stride, size_t *lens);
/* End to end: WormholeProver::commit(inputs) + prove() (wormhole/prover/src/lib.rs:
 * 209-237) for a batch of CircuitInputs.  commit() (the fragments' fill_targets)
 * runs on the host thread pool; generate_partial_witness (plonky2
 * iop/generator.rs: Poseidon, BaseSum, arithmetic, equality and constant
 * generators) runs on the device, one workgroup per proof, level by level;
 * then the proof.  A witness conflict returns QP_ERR_WITNESS with the
 * reference's "set twice with different values" message naming the proof. */
int qp_prover_prove_wormhole_inputs(qp_prover *p, const qp_wormhole_inputs *in, uint32_t nproofs, uint8_t *out,
                                    size_t stride, size_t *lens);
/* the same for the voting circuit: VoteCircuitData::fill_targets + prove
 * (voting/src/lib.rs:199-261, :346-357)                                     */
int qp_prover_prove_voting_inputs(qp_prover *p, const qp_voting_inputs *in, uint32_t nproofs, uint8_t *out,
                                  size_t stride, size_t *lens);
/* the same for aggregation circuits: nchunks aggregate_chunk calls
 * (tree.rs:106-143) proven as one batch — the chunks' proof bytes are
 * deserialized into the circuit's input targets on the host pool, the
 * recursive verifier's generators (Poseidon, arithmetic, BaseSum, wire split,
 * extension division, RandomAccess, ...) run on the device; an invalid inner
 * proof returns QP_ERR_WITNESS naming the chunk.                            */
int qp_prover_prove_aggregation(qp_prover *p, const qp_aggregation_chunk *chunks, uint32_t nchunks, uint8_t *out,
                                size_t stride, size_t *lens);
/* same, with the wire matrices already resident on the device:
 * d_wires = device pointer [nproofs][num_wires][n]; pis on the host          */
int qp_prover_prove_wires_dev(qp_prover *p, const uint64_t *d_wires, const uint64_t *pis, uint32_t nproofs,
                              uint8_t *out, size_t stride, size_t *lens);
/* HIP-event timing of the hot kernels on the prover's stream (off by default):
 * slot 0 = wires LDE (NTT; units = algorithmic bytes 8*(n+N) per column),
 * 1 = wires leaf hashing (units = permutations), 2 = wires Merkle levels
 * (units = permutations), 3 = quotient evaluation (units = LDE points)     */
int qp_prover_set_timing(qp_prover *p, int enable);
/* TEST-ONLY: use `witness` as every proof's FRI proof-of-work witness instead
 * of grinding the minimal one (enable = 0 restores grinding).  The reference's
 * rayon find_any witness is nondeterministic, so reproducing one of its proofs
 * byte for byte needs its witness (tests/test_gpu_reference_proof.py); a
 * witness without the required leading zeros gives a proof that fails
 * verification.                                                            */
int qp_prover_debug_force_pow(qp_prover *p, uint64_t witness, int enable);
/* TEST-ONLY: release one of the prover's device tables ("wg_wslot_cm",
 * "wg_gens" or "qtab") to check that a launch whose table is missing returns
 * QP_ERR_STATE naming it instead of faulting (every prove entry point checks
 * the tables its kernels read before launching them).                      */
int qp_prover_debug_drop_table(qp_prover *p, const char *name);
/* TEST-ONLY: the device field arithmetic, one function at a time
 * (csrc/field_probe.hip).  Lane i applies `op` to a[i], b[i] and stores the
 * RAW result (no canonicalisation) to out[i]; the kernel calls the functions
 * the production kernels call (ntt16.h nt::, field_nc.h gfn::,
 * poseidon_fast.h pf::, field.h gl::; the op names keep the namespace the
 * function had when the probe was written).  The operands must respect the
 * function's own contract (noted per op); the probe does not check them.
 * The 4-wide and K-wide forms take a group of consecutive elements per lane
 * (n a multiple of the group size) and store the group's results in place,
 * QP_FOP_ACC3 one word per group (out holds n / param words).  b may be NULL
 * for the unary ops.  Unknown op, unknown param (nonzero where none is taken)
 * or n not a multiple of the group size: QP_ERR_ARG.                        */
enum {
    QP_FOP_NT_ADD = 0,        /* nt::add (add_mad): a + b, any u64                         */
    QP_FOP_NT_ADD4,           /* nt::add4: groups of 4                                     */
    QP_FOP_GFN_ADD,           /* gfn::add                                                  */
    QP_FOP_GFN_ADD_C,         /* gfn::add_c: b < p                                         */
    QP_FOP_PF_ADD_C,          /* pf::add_c: b < p                                          */
    QP_FOP_GL_ADD,            /* gl::add: a, b < p; result < p                             */
    QP_FOP_NT_SUB,            /* nt::sub (gfn::sub by name): a - b, any u64                */
    QP_FOP_NT_SUB4,           /* nt::sub4: groups of 4                                     */
    QP_FOP_GL_SUB,            /* gl::sub: a, b < p; result < p                             */
    QP_FOP_NT_REDUCE,         /* nt::reduce(lo = a, hi = b)                                */
    QP_FOP_GFN_REDUCE,        /* gfn::reduce(lo = a, hi = b)                               */
    QP_FOP_GL_REDUCE128,      /* gl::reduce128(lo = a, hi = b); result < p                 */
    QP_FOP_PF_REDUCE_ROW,     /* pf::reduce_row(al = a, ah = b): a, b < 2^60               */
    QP_FOP_PF_REDUCE_ROW_C,   /* pf::reduce_row_c, same operands                           */
    QP_FOP_PF_SUB_SMALL,      /* pf::sub_small(r = a, y = b): b < 2^40                     */
    QP_FOP_PF_MUL,            /* gfn::mul (pf::mul, nt::mul by name)                       */
    QP_FOP_PF_MUL_C,          /* gfn::mul_c                                                */
    QP_FOP_PF_MULK2,          /* gfn::mulk<2>: groups of 2                                 */
    QP_FOP_PF_MULK3,          /* gfn::mulk<3>: groups of 3                                 */
    QP_FOP_GL_MUL,            /* gl::mul (device mul_wide); result < p                     */
    QP_FOP_PF_SBOX,           /* pf::sbox(a) = a^7                                         */
    QP_FOP_PF_SBOX_C,         /* pf::sbox_c(a)                                             */
    QP_FOP_NT_MUL_POW2,       /* nt::mul_pow2<param>(a): param a multiple of 6 below 192   */
    QP_FOP_ACC3,              /* gfn::Acc3, groups of param (1..256) elements: mac(a[k],
                               * b[k]) for each, add_shifted(a[0], param % 64), value()   */
    QP_FOP_PF_REDUCE_ROW_WIDE, /* pf::reduce_row_wide(al = a, ah = b): b < 2^64 - 2^32     */
    QP_FOP_COUNT
};
int qp_debug_field_op(qp_ctx *ctx, uint32_t op, uint32_t param, const uint64_t *a, const uint64_t *b, uint64_t n,
                      uint64_t *out);
/* TEST-ONLY: the device Poseidon forms, one at a time (csrc/poseidon_probe.hip).
 * State i is states[12 i .. 12 i + 12); out gets 12 RAW words per state (no
 * canonicalisation).  The one-lane forms (pf::, poseidon_fast.h) run one state
 * per lane; the cooperative forms (pc::, poseidon_coop.h) hold element j on lane
 * j < 12 of a 64-lane wave or of a 16-lane row (four states per wave), every
 * launched wave whole and a wave / row past nstates exiting whole.  Inputs are
 * any u64 unless noted; `param` is 0 where none is taken.  Unknown form or
 * param, a null pointer, more than 2^20 states or a capz state whose lanes
 * 8..11 are not 0: QP_ERR_ARG.                                             */
enum {
    QP_PFORM_PERMUTE_NC = 0,   /* pf::permute_nc                                            */
    QP_PFORM_PERMUTE_CAPZ,     /* pf::permute_nc_capz<0xF>: lanes 8..11 enter 0; lanes 0..3 defined */
    QP_PFORM_ROUNDS1_L7,       /* pf::rounds<1, 0x80> on the state entering round 1; lane 7 defined */
    QP_PFORM_COOP_PERMUTE,     /* pc::permute, one state per wave                           */
    QP_PFORM_ROW_PERMUTE,      /* pc::permute_row, one state per 16-lane row                */
    QP_PFORM_MDS_BLOCK,        /* pf::mds_block<-1> (param 0) or mds_block<27> (param 27)   */
    QP_PFORM_MDS_K,            /* pf::mds_k(s, RC[param]), param 1..29                      */
    QP_PFORM_MDS_MADS,         /* pf::mds_mads                                              */
    QP_PFORM_CAPZ_ROUND0,      /* round 0 of permute_nc_capz (8 S-boxes, capz_mds): lanes 8..11 enter 0 */
    QP_PFORM_MDS_INIT_SPARSE,  /* pf::mds_init_sparse                                       */
    QP_PFORM_PARTIAL_GROUP,    /* pf::partial_group<param, 4>, param 0, 4, .., 16; <20, 2> folds KLAST */
    QP_PFORM_FULL_ROUND_DYN,   /* pf::full_round_dyn folding RC[param], param 1..29         */
    QP_PFORM_PARTIAL_DYN,      /* pf::sbox on lane 0, then mds_rows_block_dyn folding RC[param], 1..29 */
    QP_PFORM_COOP_MDS,         /* pc::wave_mds_row with pc::mds_coef, one state per wave    */
    QP_PFORM_ROW_MDS,          /* pc::row_mds with pc::mds_coef, one state per 16-lane row  */
    QP_PFORM_DENSE_GROUP,      /* pf::dense_group<param, pfd::GLEN[param]>, param a group start: 0, 3, .., 15, 18, 20 */
    QP_PFORM_COUNT,            /* the forms above; it stays the first id they reject        */
    QP_PFORM_DENSE_GROUP4 = QP_PFORM_COUNT + 1, /* pf::dense_group<param, pfd4::GLEN[param], pf::TabG4>, param a group
                                * start of the hashing path's plan: 0, 4, 8, 12, 16, 19      */
    QP_PFORM_END
};
int qp_debug_poseidon_op(qp_ctx *ctx, uint32_t form, uint32_t param, const uint64_t *states, uint64_t nstates,
                         uint64_t *out);
/* TEST-ONLY: a caller's witness-generator program through the production
 * witness kernels (csrc/witness_probe.cpp; the launches are those of the
 * prover's gen_witness_batch, csrc/witness_launch.h): every slot unset, the
 * inputs stored, then the generators by the scheduler `form` names.
 * gens: ngens records of five words (kind | row << 32, s[0] | s[1] << 32,
 * s[2] | s[3] << 32, k0, k1: qc::DevGen, csrc/circuit.h) in level order;
 * level_off[nlevels + 1] and level_pos[nlevels][2] (first Poseidon record of
 * the level, count) as CircuitData holds them; wslot[nrows][W] the row-major
 * wire -> slot table.  Slot ids in gens and wslot may carry bit 31 (several
 * writers: compare-and-swap); in_slots, wslot_cm and pi_slots are plain ids.
 * Results: vals[B][nslots] raw (2^64 - 1 where nothing was written), err[B]
 * (0, or 1 + the index of a failing generator).  With wslot_cm (the
 * column-major slot map [W][nrows]) also wires[B][W][nrows] and
 * pis[B][npis] of witness_expand (wires, and pis when npis > 0, then required).
 * The program is validated before any launch (csrc/witness_program.h): a
 * malformed one returns QP_ERR_ARG with a text naming the fault and launches
 * nothing.                                                                  */
enum {
    QP_WFORM_PROOF_256 = 0,    /* k_witness_gen, one 256-thread workgroup per proof          */
    QP_WFORM_PROOF_512,        /* k_witness_gen, 512 threads (the aggregation circuits)      */
    QP_WFORM_LEVEL_ROW,        /* k_witness_level per level, Poseidons one per 16-lane row   */
    QP_WFORM_LEVEL_WAVE,       /* k_witness_level per level, Poseidons one per wave (wit_row=0) */
    QP_WFORM_PROOF_256_WAVE,   /* k_witness_gen, 256 threads, cooperative Poseidons one per wave */
    QP_WFORM_PROOF_512_WAVE,   /* k_witness_gen, 512 threads, cooperative Poseidons one per wave */
    QP_WFORM_COUNT
};
typedef struct {
    const uint64_t *gens;
    uint32_t ngens;
    const uint32_t *level_off;
    const uint32_t *level_pos;
    uint32_t nlevels;
    const uint32_t *wslot;
    uint32_t nrows, W, nslots, limbs, zero_slot, num_consts;
    const uint32_t *in_slots;
    const uint64_t *in_vals;   /* [B][nin] */
    uint32_t nin, B, form;
    const uint32_t *wslot_cm;  /* NULL: no expansion */
    const uint32_t *pi_slots;
    uint32_t npis;
} qp_witness_program;
int qp_debug_witness_program(qp_ctx *ctx, const qp_witness_program *prog, uint64_t *vals, uint32_t *err,
                             uint64_t *wires, uint64_t *pis);
/* host threads (the caller included) of the prover's pool for commit() and the
 * per-proof host stages; default min(hardware threads, 16).  Several provers in
 * one process should split the host cores (cores / provers each).           */
int qp_prover_set_host_threads(qp_prover *p, uint32_t nthreads);
int qp_prover_kernel_stats(qp_prover *p, double *ms, double *units, uint64_t *launches, uint32_t n, int reset);
/* accumulated host wall time per stage (ms): [0] commit wires, [1] zs, [2] quotient,
 * [3] openings, [4] FRI, [5] PoW, [6] queries, [7] serialize, [8] commit() of the
 * inputs (host), [9] device witness generation; reset != 0 clears */
int qp_prover_stage_times(qp_prover *p, double *ms, uint32_t n, int reset);

/* ---- voter registry (device) ------------------------------------------------
 * The electorate's Merkle tree of a proposal, built once, and the Merkle paths
 * the voting circuit walks, by voter index.  The reference has no such object:
 * its test builds the tree with a host loop (voting/src/lib.rs:285-316), and
 * that loop is the convention: leaf = hash_no_pad(private key), node =
 * hash_no_pad(left || right), the last node of an odd-length level moves to
 * the next level unchanged.  A voter's path holds the siblings of the levels
 * where its node was hashed, in order from the leaf, one side bit each
 * (VotePrivateInputs.merkle_siblings / path_indices / actual_merkle_depth,
 * lib.rs:42-52, as the circuit's walk reads them, :123-180); promoted levels
 * contribute nothing.  A registry belongs to its context: free it before
 * qp_ctx_destroy.                                                          */
typedef struct qp_registry qp_registry;
/* replaces the leaf and level loops of voting/src/lib.rs:292-316.  keys
 * [n][4] canonical felts.  QP_ERR_ARG for n == 0, a felt >= p, or n > 2^31 (a
 * path deeper than 31 does not fit the circuit's 5-bit depth split).  Device
 * memory: 64 n bytes of digests (every level stays resident).              */
int qp_registry_new(qp_ctx *ctx, const uint64_t *keys, uint64_t n, qp_registry **out);
void qp_registry_free(qp_registry *r);
/* VotePublicInputs.merkle_root (lib.rs:318) */
int qp_registry_root(const qp_registry *r, uint64_t out[4]);
/* the voter count and the deepest path, ceil(log2 n) (either may be NULL) */
int qp_registry_size(const qp_registry *r, uint64_t *n, uint32_t *max_depth);
/* replaces the hand-picked merkle_siblings / path_indices /
 * actual_merkle_depth of lib.rs:320-322 for voters idx[0..nidx): siblings
 * [nidx][32][4] (the zero digest from the depth up, as fill_targets sets
 * them, lib.rs:254-257), path_bits[b] bit j = path_indices[j] (1: the voter's
 * node is the right child), depth[b] = actual_merkle_depth.  An index >= n
 * is QP_ERR_ARG (checked before the launch).                               */
int qp_registry_paths(qp_registry *r, const uint64_t *idx, uint32_t nidx, uint64_t *siblings, uint32_t *path_bits,
                      uint32_t *depth);
/* copies one level's digests [len][4] (level 0 = the leaves, the last = the
 * root); out == NULL: only *len.  Test/diagnostic entry point.             */
int qp_registry_level(qp_registry *r, uint32_t level, uint64_t *out, uint64_t *len);
/* HIP-event times of the build on the context's stream (ms): [0] key upload,
 * [1] leaf digests (n permutations), [2] the levels (n - 1 permutations).
 * Diagnostic entry point (tools/registry_bench.py).                        */
int qp_registry_build_times(const qp_registry *r, double ms[3]);

/* ---- a registry from commitments: what an election operator holds ----------
 * The operator never sees a private key, only each voter's commitment, the
 * leaf hash_no_pad(key) the voter sends when registering; voters arrive over
 * time and some are struck off.  A commitment registry keeps no keys, reserves
 * room to grow in place and is updated on the device: an update recomputes
 * only the nodes it changes.  The entries above work on it as on a keyed one,
 * except that on an empty one (n == 0) qp_registry_root, _paths and _level
 * return QP_ERR_STATE; qp_registry_build_times then gives the last build or
 * update: [0] upload, [1] 0 (there is no leaf kernel), [2] the levels.
 * qp_prover_prove_voters on it is QP_ERR_STATE (it holds no keys); the calls
 * below on a registry made by qp_registry_new are QP_ERR_STATE too (its host
 * key copy would go stale).  A refused call leaves the registry as it was:
 * same root, size and epoch.  A path is valid only under the root of the
 * epoch it was taken in.                                                   */
/* a registry over registered commitments: leaves[n][4] canonical felts, each the voter's
 * hash_no_pad(private key), computed by the voter.  n may be 0 (registration opens empty).
 * capacity >= max(n, 1), <= 2^31: the digest buffer is laid out for `capacity` leaves
 * (64 * capacity bytes), so the tree can grow in place.  No keys are held anywhere.       */
int qp_registry_new_commitments(qp_ctx *ctx, const uint64_t *leaves, uint64_t n, uint64_t capacity, qp_registry **out);
/* registers k more voters at indices [n, n + k); *first (may be NULL) = n before the call.
 * n + k > capacity: QP_ERR_ARG (call qp_registry_reserve); a felt >= p: QP_ERR_ARG naming
 * the voter and the felt; k == 0: QP_OK, nothing changes                                  */
int qp_registry_append(qp_registry *r, const uint64_t *leaves, uint64_t k, uint64_t *first);
/* replaces the commitments of voters idx[0..k) (each < n, no index twice); a voter is
 * struck off by replacing the commitment with one nobody holds a key for                  */
int qp_registry_replace(qp_registry *r, const uint64_t *idx, const uint64_t *leaves, uint32_t k);
/* moves the tree to a layout for new_capacity >= n leaves (device-to-device, level by level) */
int qp_registry_reserve(qp_registry *r, uint64_t new_capacity);
/* capacity, and the number of completed append / replace / reserve calls (either may be NULL);
 * a keyed registry reports capacity == n and epoch == 0                                   */
int qp_registry_state(const qp_registry *r, uint64_t *capacity, uint64_t *epoch);
/* one voter's ballot: the public inputs the voter chooses (lib.rs:324-326) */
typedef struct {
    uint64_t proposal_id[4];
    uint8_t vote;                      /* 0 = no, 1 = yes */
    const uint64_t *zk_randomness;     /* as in qp_voting_inputs */
} qp_vote_ballot;
/* create_test_inputs + prove (lib.rs:285-343, :346-357) for voters idx[] of
 * a registry: the private key and the root are the registry's, the path comes
 * from the device tree, the nullifier is H(leaf || proposal_id) (lib.rs:
 * 277-283); then qp_prover_prove_voting_inputs on those inputs, so the proofs
 * are the bytes that call gives for the same inputs.  The prover must be a
 * voting-circuit prover of the registry's context (QP_ERR_ARG otherwise).  */
int qp_prover_prove_voters(qp_prover *p, qp_registry *r, const uint64_t *idx, const qp_vote_ballot *ballots,
                           uint32_t nproofs, uint8_t *out, size_t stride, size_t *lens);

/* ---- ballot box: count voting proofs once per nullifier ----------------------
 * The counter's side of an election.  A verified voting proof says only that
 * some registered voter voted `vote` on `proposal_id` under `merkle_root`, with
 * this `nullifier` ("the nullifier to prevent double voting", voting/src/
 * lib.rs:33-34); the reference has no object that uses it.  A box is opened for
 * one proposal with the Merkle roots the operator published (1 to 64; a
 * registry's root changes with every epoch) and a capacity of admitted
 * ballots.  Every ballot cast gets a number: its position in the stream of all
 * ballots cast into the box, rejected ones included, from 0.  The 13 public
 * inputs are proposal[0:4] root[4:8] vote[8] nullifier[9:13] (lib.rs:55-62);
 * a ballot's status is the first of these checks that fails, in this order:  */
typedef enum {
    QP_BALLOT_COUNTED = 0,        /* admitted and counted; first = its own number */
    QP_BALLOT_PROOF_REJECTED = 1, /* the verifier's verdict is not QP_VERIFY_OK (it is in verify_status) */
    QP_BALLOT_MALFORMED = 2,      /* a public input >= p (reachable only through qp_ballot_box_cast_public) */
    QP_BALLOT_WRONG_PROPOSAL = 3, /* proposal differs from the box's */
    QP_BALLOT_UNKNOWN_ROOT = 4,   /* root is not among the accepted roots */
    QP_BALLOT_BAD_VOTE = 5,       /* vote is neither 0 nor 1 (a sound proof cannot carry that; screened anyway) */
    QP_BALLOT_DOUBLE_VOTE = 6     /* an earlier ballot with the same nullifier was counted; first = its number */
} qp_ballot_status;
/* A ballot that passes the first five checks is admitted and takes one of the
 * capacity's entries; the sixth decides between counted and double vote.  The
 * lowest number wins: of the admitted ballots with one nullifier the counted
 * one is the one with the lowest number, inside a batch and across batches.
 * Statuses, `first` and the tally are a function of the ballot stream alone:
 * not of how it is cut into batches, of the path (device or host) or of the
 * device's scheduling.  Nothing is ever removed from a box.
 *
 * With a context the admitted ballots' log (nullifier, number, flags) and the
 * nullifier table live on the device and the box uses the context's stream
 * (free it before qp_ctx_destroy); ctx == NULL runs the same semantics on the
 * host.  Every call is all or nothing: what it can refuse is checked before
 * anything is enqueued, and a refused call leaves the cast and admitted
 * counts, the tally and the log as they were (out[] is then unspecified).   */
typedef struct qp_ballot_box qp_ballot_box;
struct qp_verifier;
typedef struct {
    uint32_t status;         /* qp_ballot_status */
    uint32_t verify_status;  /* qp_verify_status of the proof (cast_public: verdicts[i]) */
    uint64_t number;         /* the ballot's number */
    uint64_t first;          /* counted: number; double vote: the counted ballot's number; else number */
} qp_ballot_result;
/* proposal_id: 4 canonical felts; roots [nroots][4] canonical, 1 <= nroots <= 64 (a root given
 * twice counts once); 1 <= capacity <= 2^31 admitted ballots.  Device memory: 41 bytes per
 * entry of capacity and 4 per table slot (the power of two >= 2 capacity slots).           */
int qp_ballot_box_new(qp_ctx *ctx /* NULL: host */, const uint64_t proposal_id[4], const uint64_t *roots,
                      uint32_t nroots, uint64_t capacity, qp_ballot_box **out);
void qp_ballot_box_free(qp_ballot_box *b);
/* the reason of the box's last refused call; b == NULL: of this thread's last refused qp_ballot_box_new */
const char *qp_ballot_box_last_error(const qp_ballot_box *b);
/* one more accepted root (a new epoch's); a root the box already accepts: QP_OK, held once; a 65th: QP_ERR_ARG */
int qp_ballot_box_accept_root(qp_ballot_box *b, const uint64_t root[4]);
/* verifies proofs[0..n) with v, a verifier of the voting circuit's data (13 public inputs, else
 * QP_ERR_ARG), then casts them: out[n].  More admitted ballots than the capacity has room for:
 * QP_ERR_ARG (call qp_ballot_box_reserve); n == 0: QP_OK                                   */
int qp_ballot_box_cast(qp_ballot_box *b, struct qp_verifier *v, const uint8_t *const *proofs, const size_t *lens,
                       uint32_t n, qp_ballot_result *out);
/* the routine-level seam: public inputs pis[n][13] of proofs verified elsewhere (verdicts[i] != 0
 * marks a rejected one; NULL = all verified); also the small-shape test surface of the kernels */
int qp_ballot_box_cast_public(qp_ballot_box *b, const uint64_t *pis, const uint32_t *verdicts, uint32_t n,
                              qp_ballot_result *out);
/* moves the box to a log and table for new_capacity >= admitted (and >= 1, <= 2^31); statuses
 * already handed out stay true                                                             */
int qp_ballot_box_reserve(qp_ballot_box *b, uint64_t new_capacity);
/* counted yes and no votes (either may be NULL) */
int qp_ballot_box_tally(const qp_ballot_box *b, uint64_t *yes, uint64_t *no);
/* ballots cast, admitted, capacity (each may be NULL) */
int qp_ballot_box_state(const qp_ballot_box *b, uint64_t *cast, uint64_t *admitted, uint64_t *capacity);
/* the log, for publication and audit: entries [first, first + k) in admission order: nullifiers
 * [k][4], numbers [k], flags [k] (bit 0 the vote, bit 1 counted); each may be NULL          */
int qp_ballot_box_entries(qp_ballot_box *b, uint64_t first, uint64_t k, uint64_t *nullifiers, uint64_t *numbers,
                          uint8_t *flags);
/* the audit: yes, no, counted, admitted recomputed from the log's flags alone */
int qp_ballot_box_recount(qp_ballot_box *b, uint64_t out[4]);
/* HIP-event times of the last device cast that admitted a ballot (ms): [0] the log upload, [1]
 * insert + resolve.  Diagnostic entry point (tools/ballot_bench.py); 0 on the host path.    */
int qp_ballot_box_cast_times(const qp_ballot_box *b, double ms[2]);

/* ---- the log commitment: what the operator publishes, and a voter's receipt --
 * The log is append-only and final: an entry never changes once its cast
 * returned.  Its commitment is (root, n), n = the admitted count:
 *   log leaf of entry seq = hash_no_pad([nullifier[0..4], number, flags]), six
 *     felts, flags the log's byte (bit 0 the vote, bit 1 counted);
 *   the tree over leaves [0, n) in the registry's convention: node =
 *     hash_no_pad(left || right), the last node of an odd level moves up
 *     unchanged.
 * The operator publishes (root, n, tally).  A receipt ties one entry to that
 * pair: the entry, its siblings compacted as qp_registry_paths compacts them,
 * the side bits and the depth.  A receipt is valid only under the (root, n) it
 * was made under: every later cast that admits a ballot changes both.  The
 * checker takes the tree's shape from (seq, n) alone (at level l the node
 * seq >> l has a sibling iff ((seq >> l) ^ 1) < ceil(n / 2^l)) and rejects a
 * receipt whose depth or side bits say otherwise, so a node cannot be offered
 * as a leaf.  The tree (64 bytes per entry of capacity on the device) is
 * allocated by the first commit and brought up to date on demand only; reserve
 * drops it, and the next commit rebuilds it to the same root.  A device step
 * that fails is QP_ERR_HIP and leaves the box dead, as in qp_ballot_box_cast. */
/* seq_out[i] = the log index of the *counted* entry with nullifiers[i][4] (a double vote's
 * nullifier gives the counted entry, not its own), UINT64_MAX if that nullifier was never
 * admitted.  A felt >= p: QP_ERR_ARG naming the position.  k == 0: QP_OK, nothing launched */
int qp_ballot_box_find(qp_ballot_box *b, const uint64_t *nullifiers, uint32_t k, uint64_t *seq_out);
/* hashes the leaves the tree does not hold yet and the nodes above them; root_out, *n_out (either
 * may be NULL) = the commitment.  Nothing admitted: QP_ERR_STATE "empty log"; nothing new since
 * the last commit: the same pair, nothing launched                                          */
int qp_ballot_box_commit_log(qp_ballot_box *b, uint64_t root_out[4], uint64_t *n_out);
/* commits, then the paths of entries seqs[0..k) (each < admitted, else QP_ERR_ARG before anything
 * is enqueued): siblings [k][32][4] (the zero digest from the depth up), path_bits[i] bit j = side
 * of sibling j (1: the entry's node is the right child), depth[i], leaves [k][4] (may be NULL) =
 * the entries' log leaves; root_out, *n_out (either may be NULL) = the commitment they hold under */
int qp_ballot_box_receipts(qp_ballot_box *b, const uint64_t *seqs, uint32_t k, uint64_t *siblings, uint32_t *path_bits,
                           uint32_t *depth, uint64_t *leaves, uint64_t root_out[4], uint64_t *n_out);
/* the log entries seqs[0..k) (each < admitted, any order): nullifiers [k][4], numbers [k], flags [k]
 * as qp_ballot_box_entries gives them; each may be NULL.  What a receipt carries beside its path */
int qp_ballot_box_entries_at(qp_ballot_box *b, const uint64_t *seqs, uint32_t k, uint64_t *nullifiers,
                             uint64_t *numbers, uint8_t *flags);
typedef enum {
    QP_RECEIPT_OK = 0,
    QP_RECEIPT_SHAPE = 1,         /* seq >= n, n outside 1..2^31, depth or path_bits not the shape of (seq, n),
                                     or a non-zero sibling slot above the depth */
    QP_RECEIPT_ROOT = 2,          /* the walk from the entry's leaf does not end at root */
    QP_RECEIPT_NON_CANONICAL = 3, /* a felt >= p in root, nullifier, number or siblings, or flags > 3 */
    QP_RECEIPT_NULL = 4           /* a null pointer */
} qp_receipt_status;
/* checks a receipt against a published (root, n); needs no box and no device.  siblings [32][4].
 * Returns a qp_receipt_status: the first reason found, in the order non-canonical, shape, root  */
int qp_ballot_receipt_check(const uint64_t root[4], uint64_t n, uint64_t seq, const uint64_t nullifier[4],
                            uint64_t number, uint8_t flags, const uint64_t *siblings, uint32_t path_bits,
                            uint32_t depth);

/* ---- the audit of a published log, prefix roots, reopening a box -------------
 * A published log is what qp_ballot_box_entries returns: nullifiers[n][4],
 * numbers[n], flags[n], 1 <= n <= 2^31.  Beside it come optional claims: a
 * root, a tally (yes, no), and earlier commitments (root_i, n_i).  The audit
 * reports the first reason that fires, in this order, with the lowest offender
 * as its witness, so the report is a function of the input alone:            */
typedef enum {
    QP_AUDIT_OK = 0,
    QP_AUDIT_NON_CANONICAL = 1, /* a nullifier felt >= p, a number >= p or a flags byte > 3; witness = the lowest
                                   such seq.  Nothing is hashed: the report's root and counts are zero */
    QP_AUDIT_ORDER = 2,         /* numbers[seq] <= numbers[seq - 1] (a box's log has strictly increasing numbers);
                                   witness = the lowest such seq >= 1 */
    QP_AUDIT_COUNT_RULE = 3,    /* an entry's counted bit != "no earlier entry has this nullifier"; witness = the
                                   lowest such seq, first = the lowest seq holding that nullifier */
    QP_AUDIT_TALLY = 4,         /* a tally is claimed and differs from (counted & vote, counted & !vote) of the flags */
    QP_AUDIT_ROOT = 5,          /* a root is claimed and differs from the log tree's root over [0, n) */
    QP_AUDIT_COMMITMENT = 6     /* some (root_i, n_i) has n_i > n, or the root of the prefix [0, n_i) != root_i;
                                   witness = the lowest such index i */
} qp_audit_status;
/* On every status but QP_AUDIT_NON_CANONICAL the report carries the recomputed
 * root and (yes, no, counted) of the flags.
 * Prefix root of m, 1 <= m <= n, in a tree of n leaves: acc = leaf m - 1; at
 * each level l while c = ceil(m / 2^l) > 1: c odd, acc moves up unchanged; c
 * even, acc = hash_no_pad(dig[l][c - 2] || acc).  dig[l][c - 2] covers only
 * leaves below m, so it is the same digest in the larger tree: the log tree's
 * shape, with the odd node promoted, is the append-only shape.  The prefix root
 * at m = n is the root.  With a context the audit runs on the device: one lane
 * per entry inserts the whole log into a fresh nullifier table, whose slots
 * end at the lowest seq of each nullifier whatever the scheduling.            */
typedef struct {
    uint32_t status;         /* qp_audit_status */
    uint32_t pad;
    uint64_t witness, first; /* UINT64_MAX: none */
    uint64_t root[4], yes, no, counted;
} qp_audit_report;
/* audits a published log against the claims given (each NULL / ncommit == 0: not claimed).  QP_OK:
 * the audit ran, the verdict is out->status.  QP_ERR_ARG: a null buffer, n outside 1..2^31, a claimed
 * or commitment root with a felt >= p, some n_i == 0.  Needs no box; the log is not altered.      */
int qp_ballot_log_audit(qp_ctx *ctx /* NULL: host */, const uint64_t *nullifiers, const uint64_t *numbers,
                        const uint8_t *flags, uint64_t n, const uint64_t *claimed_root /* NULL: none */,
                        const uint64_t *claimed_tally /* [2] or NULL */, const uint64_t *commit_roots,
                        const uint64_t *commit_ns, uint32_t ncommit, qp_audit_report *out);
/* commits, as qp_ballot_box_receipts does, then roots_out[i][4] = the root the log had at ms[i]
 * entries: the commitment (root, ms[i]) the box gave, or would have given, then.  Each ms[i] in
 * 1..admitted, else QP_ERR_ARG naming the position, before anything is enqueued.  Nothing admitted:
 * QP_ERR_STATE "empty log".  k == 0: QP_OK, nothing launched beyond the commit.                  */
int qp_ballot_box_roots_at(qp_ballot_box *b, const uint64_t *ms, uint32_t k, uint64_t *roots_out /* [k][4] */);
/* reopens a box from a published log: the arguments of qp_ballot_box_new, the log, and cast_count,
 * the number the next ballot takes.  Runs the audit's reasons 1-3, and 5 when expect_root is given;
 * on a failing audit QP_ERR_FORMAT, no box, and qp_ballot_box_last_error(NULL) names the reason and
 * the witness.  QP_ERR_ARG unless capacity >= max(n, 1) and cast_count > numbers[n - 1]; n == 0 is
 * allowed, with any cast_count.  The box keeps the uploaded log and the table the audit built; its
 * tally comes from the flags, cast = cast_count, admitted = n, nothing is committed yet; from there
 * it is an ordinary box.  A failed HIP step: QP_ERR_HIP, no box.                                  */
int qp_ballot_box_restore(qp_ctx *ctx, const uint64_t proposal_id[4], const uint64_t *roots, uint32_t nroots,
                          uint64_t capacity, const uint64_t *nullifiers, const uint64_t *numbers,
                          const uint8_t *flags, uint64_t n, uint64_t cast_count,
                          const uint64_t *expect_root /* NULL: none */, qp_ballot_box **out);

/* ---- transfer ledger: settle Wormhole transfers once per nullifier ------------
 * The settler's side of the Wormhole circuit.  A verified proof says only that
 * some unspent transfer of `funding_amount` under storage root `root_hash` may
 * be paid to `exit_account`, with this `nullifier` ("its purpose is to prevent
 * double-spending"); the reference has no object that uses it.  A ledger is
 * opened with the storage roots of the blocks the settler knows (1 to 4096),
 * optionally the public inputs of the aggregator's padding proof, and a
 * capacity of admitted transfers.  The 16 public inputs are nullifier[0:4]
 * root_hash[4:8] funding_amount[8:12] exit_account[12:16] (wormhole/circuit/
 * src/inputs.rs:12-19,92-97); funding_amount is four 32-bit limbs, most
 * significant first (felts_to_u128).  Every transfer cast gets a number: its
 * position in the stream of all transfers cast into the ledger, rejected ones
 * included, from 0.  Its status is the first of these checks that fails, in
 * this order:                                                                  */
typedef enum {
    QP_TRANSFER_CREDITED = 0,       /* admitted and credited; first = its own number */
    QP_TRANSFER_PROOF_REJECTED = 1, /* the verifier's verdict is not QP_VERIFY_OK (it is in verify_status) */
    QP_TRANSFER_MALFORMED = 2,      /* a public input >= p (reachable only through qp_ledger_cast_public) */
    QP_TRANSFER_PADDING = 3,        /* all 16 public inputs equal the ledger's padding inputs */
    QP_TRANSFER_BAD_AMOUNT = 4,     /* an amount limb >= 2^32 (the reference's felts_to_u128 refuses it) */
    QP_TRANSFER_UNKNOWN_ROOT = 5,   /* root_hash is not among the accepted roots */
    QP_TRANSFER_DOUBLE_SPEND = 6    /* an earlier transfer with this nullifier was credited; first = its number */
} qp_transfer_status;
/* A transfer that passes the first six checks is admitted and takes a log
 * entry: nullifier, number, amount limbs, exit account, flags (bit 0 =
 * credited).  Of the admitted transfers with one nullifier the one with the
 * lowest number is credited, inside a batch and across batches; a transfer
 * rejected by an earlier check does not spend its nullifier.  A credited
 * transfer adds its amount to its exit account's total.  Totals may exceed
 * 2^128 and nothing is rejected for that: an account's total is reported as four
 * limb sums, total = sum over i of sums[i] << (96 - 32 i); with at most 2^31
 * entries each sum stays below 2^63.  Statuses, `first`, the log and every total
 * are a function of the transfer stream alone: not of how it is cut into
 * batches, of the path (device or host) or of the device's scheduling.
 *
 * With a context the log, both tables (nullifiers, accounts) and the sums live
 * on the device and the ledger uses the context's stream (free it before
 * qp_ctx_destroy): a cast uploads the raw public inputs and the verdicts, and
 * the screen, the pack, the insert and the credit run there (ledger.hip).
 * ctx == NULL runs the same semantics on the host.  Every call is all or
 * nothing: a refused call leaves every count, the log and the totals as they
 * were (out[] is then unspecified).  A device step that fails, or a set error
 * word of the kernels' cannot-be-reached branches, is QP_ERR_HIP and leaves the
 * ledger dead: later calls return QP_ERR_STATE.                               */
typedef struct qp_ledger qp_ledger;
typedef struct {
    uint32_t status;         /* qp_transfer_status */
    uint32_t verify_status;  /* qp_verify_status of the proof (cast_public: verdicts[i]) */
    uint64_t number;         /* the transfer's number */
    uint64_t first;          /* double spend: the credited transfer's number; else number */
} qp_transfer_result;
/* roots [nroots][4] canonical, 1 <= nroots <= 4096 (a root given twice is held once); padding_pis:
 * the 16 canonical public inputs of the padding proof, or NULL for none; 1 <= capacity <= 2^31
 * admitted transfers.  Device memory: 93 bytes per entry of capacity and 40 per table slot (the
 * power of two >= 2 capacity slots).                                                        */
int qp_ledger_new(qp_ctx *ctx /* NULL: host */, const uint64_t *roots, uint32_t nroots,
                  const uint64_t *padding_pis /* [16] or NULL */, uint64_t capacity, qp_ledger **out);
void qp_ledger_free(qp_ledger *l);
/* the reason of the ledger's last refused call; l == NULL: of this thread's last refused qp_ledger_new */
const char *qp_ledger_last_error(const qp_ledger *l);
/* one more accepted root (a new block's); a root the ledger already accepts: QP_OK, held once; a 4097th: QP_ERR_ARG */
int qp_ledger_accept_root(qp_ledger *l, const uint64_t root[4]);
/* moves the ledger to a log and tables for new_capacity >= admitted (and >= 1, <= 2^31): the log is
 * copied, both tables and the sums are rebuilt from the credited entries; everything handed out stays true */
int qp_ledger_reserve(qp_ledger *l, uint64_t new_capacity);
/* transfers cast, admitted, credited, accounts credited so far, capacity (each may be NULL) */
int qp_ledger_state(const qp_ledger *l, uint64_t *cast, uint64_t *admitted, uint64_t *credited, uint64_t *accounts,
                    uint64_t *capacity);
/* verifies proofs[0..n) with v, a verifier of a circuit with 16 public inputs (else QP_ERR_ARG), then
 * casts them: out[n].  More admitted transfers than the capacity has room for: QP_ERR_ARG (call
 * qp_ledger_reserve); n == 0: QP_OK; n > 2^22: QP_ERR_ARG                                   */
int qp_ledger_cast(qp_ledger *l, struct qp_verifier *v, const uint8_t *const *proofs, const size_t *lens,
                   uint32_t n, qp_transfer_result *out);
/* the routine-level seam: public inputs pis[n][16] of proofs verified elsewhere (verdicts[i] != 0
 * marks a rejected one; NULL = all verified), e.g. the leaves of a verified aggregation root; also
 * the small-shape test surface of the kernels.  n <= 2^22 per call, more is QP_ERR_ARG        */
int qp_ledger_cast_public(qp_ledger *l, const uint64_t *pis, const uint32_t *verdicts, uint32_t n,
                          qp_transfer_result *out);
/* seq_out[i] = the log index of the credited entry with nullifiers[i][4] (canonical, else QP_ERR_ARG),
 * or UINT64_MAX if that nullifier was never admitted                                        */
int qp_ledger_find(qp_ledger *l, const uint64_t *nullifiers, uint32_t k, uint64_t *seq_out);
/* the log, entries [first, first + k) in admission order: nullifiers [k][4], numbers [k], amounts
 * [k][4] (32-bit limbs, most significant first), accounts [k][4], flags [k]; each may be NULL */
int qp_ledger_entries(qp_ledger *l, uint64_t first, uint64_t k, uint64_t *nullifiers, uint64_t *numbers,
                      uint32_t *amounts, uint64_t *accounts, uint8_t *flags);
/* the accounts credited so far, [first, first + k) in the order of the log index of each account's
 * first credited entry (a function of the stream alone; qp_ledger_state gives their count):
 * accounts [k][4], sums [k][4], first_seq [k]; each may be NULL                             */
int qp_ledger_payouts(qp_ledger *l, uint64_t first, uint64_t k, uint64_t *accounts, uint64_t *sums,
                      uint64_t *first_seq);
/* the limb sums of accounts[k][4] given by the caller (canonical, else QP_ERR_ARG): sums [k][4],
 * found [k]; an account never credited gives zeros and found = 0; sums and found may be NULL   */
int qp_ledger_totals_for(qp_ledger *l, const uint64_t *accounts, uint32_t k, uint64_t *sums, uint8_t *found);
/* the audit: out = credited, admitted, then the four limb sums over all credited entries, recomputed
 * from the log alone; the grand total equals the sum of the payouts                         */
int qp_ledger_recount(qp_ledger *l, uint64_t out[6]);
/* HIP-event times of the last device cast (ms): [0] the upload of the public inputs and verdicts,
 * [1] screen to credit, the read-back of the admitted count included.  Diagnostic entry point
 * (tools/ledger_bench.py); 0 on the host path.                                              */
int qp_ledger_cast_times(const qp_ledger *l, double ms[2]);

/* ---- the ledger's log commitment: what the settler publishes, and an exit
 * account's receipt.  The log is append-only and final, like the ballot box's,
 * and its commitment is (root, n), n = the admitted count:
 *   log leaf of entry seq = hash_no_pad([nullifier[0..4], number, amount[0..4],
 *     account[0..4], flags]): 14 felts.  amount is the four 32-bit limbs as the
 *     log holds them, most significant first, each as one felt; flags is the
 *     log's byte (bit 0 credited).  In plonky2's overwrite sponge that is two
 *     permutations: state = 0; felts 0..7 into state[0..8], permute; felts
 *     8..13 into state[0..6], state[6..12] as the first permutation left them,
 *     permute; the digest is state[0..4];
 *   the accumulator tree over leaves [0, n): node = hash_no_pad(left || right),
 *     the last node of an odd level moves up unchanged; laid out for the
 *     ledger's capacity.
 * The settler publishes (root, n, payouts), or in place of the list the payout
 * claims commitment of the round (below).  A receipt is the entry
 * (nullifier, number, amount limbs, account, flags) plus at most 31 siblings
 * compacted as qp_registry_paths compacts them, the side bits and the depth,
 * and holds only under the (root, n) it was made under.  The checker takes the
 * tree's shape from (seq, n) alone, as qp_ballot_receipt_check does.  The tree
 * (64 bytes per entry of capacity on the device) is allocated by the first
 * commit and brought up to date on demand only: qp_ledger_cast and
 * qp_ledger_cast_public do no tree work.  qp_ledger_reserve drops it, and the
 * next commit rebuilds it to the same root.                                    */
/* hashes the leaves the tree does not hold yet and the nodes above them; root_out, *n_out (either
 * may be NULL) = the commitment.  Nothing admitted: QP_ERR_STATE "empty log"; nothing new since the
 * last commit: the same pair, nothing launched                                              */
int qp_ledger_commit_log(qp_ledger *l, uint64_t root_out[4], uint64_t *n_out);
/* the log entries seqs[0..k) (each < admitted, else QP_ERR_ARG naming the position; any order), as
 * qp_ledger_entries gives them: nullifiers [k][4], numbers [k], amounts [k][4], accounts [k][4],
 * flags [k]; each may be NULL.  What a receipt carries beside its path                          */
int qp_ledger_entries_at(qp_ledger *l, const uint64_t *seqs, uint32_t k, uint64_t *nullifiers, uint64_t *numbers,
                         uint32_t *amounts, uint64_t *accounts, uint8_t *flags);
/* commits, then the paths of entries seqs[0..k) (each < admitted, else QP_ERR_ARG naming the position,
 * before anything is enqueued): siblings [k][32][4] (the zero digest from the depth up), path_bits[i]
 * bit j = side of sibling j (1: the entry's node is the right child), depth[i], leaves [k][4] (may be
 * NULL) = the entries' log leaves; root_out, *n_out (either may be NULL) = the commitment they hold under */
int qp_ledger_receipts(qp_ledger *l, const uint64_t *seqs, uint32_t k, uint64_t *siblings, uint32_t *path_bits,
                       uint32_t *depth, uint64_t *leaves, uint64_t root_out[4], uint64_t *n_out);
/* commits, then roots_out[i][4] = the root the log had at ms[i] entries.  Each ms[i] in 1..admitted,
 * else QP_ERR_ARG naming the position, before anything is enqueued.  Nothing admitted: QP_ERR_STATE
 * "empty log".  k == 0: QP_OK, nothing launched beyond the commit.                               */
int qp_ledger_roots_at(qp_ledger *l, const uint64_t *ms, uint32_t k, uint64_t *roots_out /* [k][4] */);
/* checks a receipt against a published (root, n); needs no ledger and no device.  siblings [32][4].
 * Returns a qp_receipt_status: the first reason found, in the order non-canonical (a felt >= p in root,
 * nullifier, number, account or siblings, or flags > 1; an amount limb is in range by its type), shape, root */
int qp_ledger_receipt_check(const uint64_t root[4], uint64_t n, uint64_t seq, const uint64_t nullifier[4],
                            uint64_t number, const uint32_t amount[4], const uint64_t account[4], uint8_t flags,
                            const uint64_t *siblings, uint32_t path_bits, uint32_t depth);

/* ---- the audit of a published transfer log ----------------------------------
 * A published log is what qp_ledger_entries returns, 1 <= n <= 2^31 entries.
 * Beside it come optional claims: a root, totals (credited, then the four limb
 * sums over the credited entries: what qp_ledger_recount gives as out[0] and
 * out[2..6]), the payouts as qp_ledger_payouts gives them, and earlier
 * commitments (root_i, n_i).  The audit reports the first reason that fires,
 * in this order, with the lowest offender as its witness, so the report is a
 * function of the input alone:                                                 */
typedef enum {
    QP_LEDGER_AUDIT_OK = 0,
    QP_LEDGER_AUDIT_NON_CANONICAL = 1, /* a nullifier or account felt >= p, a number >= p or flags > 1; witness = the
                                          lowest such seq.  Nothing is hashed: the report's root and counts are zero */
    QP_LEDGER_AUDIT_ORDER = 2,         /* numbers[seq] <= numbers[seq - 1]; witness = the lowest such seq >= 1 */
    QP_LEDGER_AUDIT_CREDIT_RULE = 3,   /* an entry's credited bit != "no earlier entry has this nullifier"; witness =
                                          the lowest such seq, first = the lowest seq holding that nullifier */
    QP_LEDGER_AUDIT_TOTALS = 4,        /* totals are claimed and differ from (credited, limb sums) of the entries
                                          whose credited bit is set */
    QP_LEDGER_AUDIT_PAYOUTS = 5,       /* payouts are claimed and differ from the log's (per account the limb sums of
                                          its entries with the credited bit, accounts in the order of their first
                                          such entry): witness = the lowest i < min(A, K) where account, sums or
                                          first_seq differ; none and A != K: min(A, K).  A = the log's accounts */
    QP_LEDGER_AUDIT_ROOT = 6,          /* a root is claimed and differs from the log tree's root over [0, n) */
    QP_LEDGER_AUDIT_COMMITMENT = 7     /* some (root_i, n_i) has n_i > n, or the root of the prefix [0, n_i) != root_i;
                                          witness = the lowest such index i */
} qp_ledger_audit_status;
/* On every status but NON_CANONICAL the report carries the recomputed root, credited, the four limb sums and
 * the account count.  Claimed limb sums are compared with the log's as the totals they name (sum of sums[i] <<
 * (96 - 32 i)), so a claim may split an exact total into its four words in any way.  With a context the audit
 * runs on the device: one lane per entry inserts the whole log into a fresh nullifier table, whose slots end
 * at the lowest seq of each nullifier whatever the scheduling; the entries with the credited bit build a fresh
 * account table and its sums; the claimed payouts are compared one lane each, in a launch after the one that
 * adds the sums.                                                                                 */
typedef struct {
    uint32_t status;         /* qp_ledger_audit_status */
    uint32_t pad;
    uint64_t witness, first; /* UINT64_MAX: none */
    uint64_t root[4], credited, sums[4], accounts;
} qp_ledger_audit_report;
/* audits a published log against the claims given (claimed_root, claimed_totals [5], pay_accounts NULL, ncommit
 * == 0: not claimed; pay_accounts [npay][4], pay_sums [npay][4], pay_first_seq [npay]).  QP_OK: the audit ran,
 * the verdict is out->status.  QP_ERR_ARG: a null buffer, n outside 1..2^31, a claimed or commitment root or a
 * claimed account with a felt >= p, some n_i == 0; the reason is qp_ledger_last_error(NULL)'s.  Needs no
 * ledger; the log is not altered.                                                               */
int qp_ledger_log_audit(qp_ctx *ctx /* NULL: host */, const uint64_t *nullifiers, const uint64_t *numbers,
                        const uint32_t *amounts, const uint64_t *accounts, const uint8_t *flags, uint64_t n,
                        const uint64_t *claimed_root, const uint64_t *claimed_totals, const uint64_t *pay_accounts,
                        const uint64_t *pay_sums, const uint64_t *pay_first_seq, uint64_t npay,
                        const uint64_t *commit_roots, const uint64_t *commit_ns, uint32_t ncommit,
                        qp_ledger_audit_report *out);

/* ---- reopening a ledger from its published log --------------------------------
 * With a context the ledger's only copy of the nullifier set, the account table
 * and the sums is in device memory; a settler whose process died counts on from
 * the log.  The arguments of qp_ledger_new with their refusals, the log in the
 * layout qp_ledger_entries returns and qp_ledger_log_audit takes, and cast_count,
 * the number the next transfer takes.  QP_ERR_ARG unless capacity >= max(n, 1)
 * and cast_count > numbers[n - 1]; n == 0 is allowed with any cast_count and
 * gives what qp_ledger_new gives, plus the counter.  Runs the audit's reasons 1-3
 * (NON_CANONICAL, ORDER, CREDIT_RULE) and ROOT when expect_root is given, on the
 * new ledger's own buffers; a failing audit is QP_ERR_FORMAT, leaves no ledger,
 * and qp_ledger_last_error(NULL) names the reason and the witness.  A failed HIP
 * step: QP_ERR_HIP, no ledger.  *out is written on QP_OK only.  The restored
 * ledger keeps the log, laid out for `capacity`, a nullifier table and an account
 * table for `capacity`, the sums of the entries whose credited bit is set and
 * each entry's account slot: cast = cast_count, admitted = n, credited and
 * accounts as the log gives them; from there it is an ordinary ledger.  With
 * expect_root the log tree is built by the ledger's own first commit and kept, so
 * a qp_ledger_commit_log that follows returns (expect_root, n) with nothing
 * launched; without it nothing is hashed until the first commit.  Device: one
 * upload of the log, the audit's screen, a synchronise (a non-canonical log ends
 * there), the whole-log insert, the audit's resolve, then the leaves and the tree
 * when a root is expected.                                                      */
int qp_ledger_restore(qp_ctx *ctx /* NULL: host */, const uint64_t *roots, uint32_t nroots,
                      const uint64_t *padding_pis /* [16] or NULL */, uint64_t capacity,
                      const uint64_t *nullifiers, const uint64_t *numbers, const uint32_t *amounts,
                      const uint64_t *accounts, const uint8_t *flags, uint64_t n, uint64_t cast_count,
                      const uint64_t *expect_root /* NULL: none */, qp_ledger **out);

/* ---- payout rounds --------------------------------------------------------------
 * qp_ledger_payouts is cumulative since the ledger opened; a settler pays per
 * round, per published commitment (root_k, n_k): round k pays the log entries
 * [n_{k-1}, n_k).  Only entries with m0 <= seq < m1 and flags bit 0 set count;
 * the flags are trusted, as qp_ledger_payouts and qp_ledger_recount trust them
 * (the audit is what checks flags).  An account credited before m0 and again
 * inside the range appears with its in-range sums and its in-range first_seq.
 * The rounds of consecutive ranges add up, account by account, to the cumulative
 * payouts, and [0, admitted) gives those.  With a context the range is credited
 * into a scratch account table of the call's own (the power of two >= 2 (m1 -
 * m0) slots) and the owners are compacted in log order; the ledger's tables, log
 * and tree are only read.                                                        */
/* the accounts credited by log entries [m0, m1), 0 <= m0 <= m1 <= admitted: one row per account with
 * a credited entry in the range: account, the four limb sums over those entries, first_seq = the
 * lowest such seq; rows in first_seq order.  *count = the number of rows, always written; at most
 * cap rows are stored (cap == 0 with null arrays: a sizing call).  The ledger is not changed.
 * m0 == m1: *count = 0.  QP_ERR_ARG, nothing stored: m0 > m1, m1 > admitted, a null count, cap > 0
 * with a null array.                                                                             */
int qp_ledger_payouts_between(qp_ledger *l, uint64_t m0, uint64_t m1, uint64_t cap, uint64_t *accounts,
                              uint64_t *sums, uint64_t *first_seq, uint64_t *count);
/* the same over a published log (accounts_log [n][4], amounts [n][4], flags [n], 1 <= n <= 2^31), no
 * ledger needed; ctx == NULL: host.  Only the entries of [m0, m1) are read (with a context: uploaded):
 * a non-canonical account or flags > 1 among them is QP_ERR_ARG, as the range errors above; the
 * reason is qp_ledger_last_error(NULL)'s.                                                        */
int qp_ledger_log_payouts_between(qp_ctx *ctx, const uint64_t *accounts_log, const uint32_t *amounts,
                                  const uint8_t *flags, uint64_t n, uint64_t m0, uint64_t m1, uint64_t cap,
                                  uint64_t *accounts, uint64_t *sums, uint64_t *first_seq, uint64_t *count);

/* ---- the nullifier-set commitment: membership and absence proofs ----------------
 * The log commitment proves what was admitted; it cannot prove that a nullifier
 * was not.  A second commitment over the sorted set of admitted nullifiers can:
 * absence is two adjacent leaves that straddle the key.  The ballot box and the
 * transfer ledger share these definitions:
 *   set      = the log entries whose member flag is set (a box's counted bit, a
 *              ledger's credited bit); m = their number.  By the handles'
 *              invariant these are the distinct admitted nullifiers;
 *   order    = the nullifier's four felts, felt 0 first, each as a full 64-bit
 *              unsigned word, then the log index seq as a fifth, least
 *              significant word: total even on a malformed published log;
 *   set leaf at sorted position j = hash_no_pad([K_j[0..4], seq_j, 2]), six
 *              felts, one permutation;
 *   set tree over leaves [0, m) in the log tree's convention: node =
 *              hash_no_pad(left || right), the odd node moves up unchanged;
 *   commitment = (set_root, m); m = 0: the root is four zeros and every absence
 *              holds with no path;
 *   proof for a key x: pos = the number of set keys below x, and found.  found:
 *              the leaf at pos has key x, in the `hi` slot.  Not found: the leaf
 *              at pos - 1 (if pos > 0; the `lo` slot) has a key below x and the
 *              leaf at pos (if pos < m; the `hi` slot) a key above x; the two
 *              positions are adjacent, so nothing lies between them.
 * The constant 2 does not keep a set leaf apart from a box's log leaf (felt 5 a
 * flags byte <= 3), nor from a node with such a right child; the position does:
 * the checker takes the tree's shape from (j, m), never from the proof, as for
 * receipts.  A proof holds only under the (set_root, m) it was made under.
 * The set tree is rebuilt whole by a commit, because sorted positions move, and
 * cached by the admitted count: a commit with nothing new launches nothing.  Its
 * buffers (on the device two record buffers of 36 bytes per member and 64
 * bytes per member for the tree) are its own: no other call allocates, launches or copies anything for it, and a
 * handle that never asks for a set root pays nothing.  With a context the
 * members are selected, sorted (a tile sort in LDS, then merge passes), hashed
 * and searched on the device.                                                  */
/* rebuilds the set commitment if an entry was admitted since the last one; root_out, *m_out (either
 * may be NULL) = (set_root, m).  An empty log: (four zeros, 0).  A duplicate member cannot be
 * reached in a handle's own log: the box's QP_ERR_STATE (the ledger's QP_ERR_HIP), and the handle is dead */
int qp_ballot_box_commit_set(qp_ballot_box *b, uint64_t root_out[4], uint64_t *m_out);
int qp_ledger_commit_set(qp_ledger *l, uint64_t root_out[4], uint64_t *m_out);
/* commits the set if it is stale, then the proofs of keys[0..k) ([k][4], canonical felts, else
 * QP_ERR_ARG naming the position before anything is enqueued): found [k], pos [k], and per slot
 * key [k][4], seq [k], siblings [k][32][4], bits [k], depth [k] as qp_ballot_box_receipts lays a path
 * out.  A found key's leaf is in the hi slot at pos; a slot the proof has no use for (lo: pos == 0
 * or found; hi: pos == m) is all zero.  root_out, *m_out (either may be NULL) = the pair the proofs
 * hold under.  k == 0: QP_OK, nothing beyond the commit                                          */
int qp_ballot_box_set_proofs(qp_ballot_box *b, const uint64_t *keys, uint32_t k, uint8_t *found, uint64_t *pos,
                             uint64_t *lo_key, uint64_t *lo_seq, uint64_t *lo_siblings, uint32_t *lo_bits,
                             uint32_t *lo_depth, uint64_t *hi_key, uint64_t *hi_seq, uint64_t *hi_siblings,
                             uint32_t *hi_bits, uint32_t *hi_depth, uint64_t root_out[4], uint64_t *m_out);
int qp_ledger_set_proofs(qp_ledger *l, const uint64_t *keys, uint32_t k, uint8_t *found, uint64_t *pos, uint64_t *lo_key,
                         uint64_t *lo_seq, uint64_t *lo_siblings, uint32_t *lo_bits, uint32_t *lo_depth,
                         uint64_t *hi_key, uint64_t *hi_seq, uint64_t *hi_siblings, uint32_t *hi_bits,
                         uint32_t *hi_depth, uint64_t root_out[4], uint64_t *m_out);
/* the set commitment of a published log, no handle needed: nullifiers [n][4], member [n] (non-zero:
 * the entry is in the set: a box's counted bit, a ledger's credited bit), 0 <= n <= 2^31.  root_out,
 * *m_out = (set_root, m); order_out (may be NULL; room for n) = the members' seqs in sorted order,
 * m of them; *dup_out (may be NULL) = UINT64_MAX, or the lowest seq of a member whose nullifier a
 * member with a lower seq holds (the pair is then the commitment of the malformed set as sorted).
 * QP_ERR_ARG: a null buffer, n > 2^31, a member's nullifier with a felt >= p; the reason is
 * qp_nullifier_set_last_error()'s                                                               */
int qp_nullifier_set_root(qp_ctx *ctx /* NULL: host */, const uint64_t *nullifiers, const uint8_t *member, uint64_t n,
                          uint64_t root_out[4], uint64_t *m_out, uint64_t *order_out, uint64_t *dup_out);
const char *qp_nullifier_set_last_error(void);
typedef enum {
    QP_SET_ORDER = 5 /* not lo.key < x < hi.key, or found with a key other than x; beside qp_receipt_status 0..4 */
} qp_set_status;
/* checks one proof against a published (set_root, m); host only, needs no handle and no device.
 * siblings [32][4] each.  Returns QP_RECEIPT_OK or the first reason found, in this order:
 * QP_RECEIPT_NULL; QP_RECEIPT_NON_CANONICAL (a felt >= p in root, x, a key, a seq or the siblings);
 * QP_RECEIPT_SHAPE (m > 2^31, pos > m, found > 1, found with pos == m, a path whose depth or side
 * bits are not the ones (j, m) gives, a non-zero sibling slot above the depth, a slot the proof has
 * no use for that is not all zero); QP_SET_ORDER; QP_RECEIPT_ROOT (a walk does not end at root)   */
int qp_nullifier_set_check(const uint64_t root[4], uint64_t m, const uint64_t x[4], uint32_t found, uint64_t pos,
                           const uint64_t lo_key[4], uint64_t lo_seq, const uint64_t *lo_siblings, uint32_t lo_bits,
                           uint32_t lo_depth, const uint64_t hi_key[4], uint64_t hi_seq, const uint64_t *hi_siblings,
                           uint32_t hi_bits, uint32_t hi_depth);
/* the records one workgroup sorts in LDS: the sizes at which the device sort changes path */
uint32_t qp_nullifier_set_tile(void);
/* the stage times (ms) of the last device build of a set on this thread: ms[0..4) = select, tile
 * sort (with the host's wait for m), duplicates + leaves, levels; ms[4 + p] = merge pass p.  Returns
 * the number written; 0: no build yet, or cap is too small (36 always suffices)                    */
uint32_t qp_nullifier_set_times(double *ms, uint32_t cap);

/* ---- payout claims: one root per round, a short proof per payee -----------------
 * A settler that publishes (root, n, payouts) makes every payee trust the list,
 * and every payer keep it.  The claims commitment replaces the list by a root, as
 * a Merkle distributor does: each account claims its total with a short proof,
 * and an account that is owed nothing in the round can be shown that.  For a log
 * range [m0, m1), 0 <= m0 <= m1 <= admitted:
 *   rows     = exactly the rows qp_ledger_payouts_between(m0, m1) gives, A of
 *              them: an account, four limb sums, first_seq (the lowest credited
 *              seq of the account in the range, counted from 0 in the whole log);
 *   order    = by account: its four felts, felt 0 first, each a full unsigned
 *              64-bit word (the nullifier set's order, first_seq as the fifth
 *              word); accounts are distinct within a range by construction;
 *   total    of a row: T = sum_i sums[i] << (96 - 32 i), carry-normalised into
 *              five 32-bit limbs t[0..5), most significant first (at most 2^31
 *              entries of at most 2^128 each: T < 2^160): one canonical form, so
 *              a payer reads a number, not a split;
 *   claim leaf at sorted position j = hash_no_pad([account[0..4], t[0..5],
 *              first_seq, 3]): 11 felts, two permutations of plonky2's overwrite
 *              sponge, as the 14-felt log leaf: felts 0..7 into state[0..8],
 *              permute; felts 8..10 into state[0..3] with state[3..12] kept,
 *              permute; the digest is state[0..4];
 *   claims tree over leaves [0, A): node = hash_no_pad(left || right), the odd
 *              node moves up unchanged;
 *   commitment = (claims_root, A, total[5]) for the named (m0, m1); total = the
 *              five-limb sum of all rows (for m0 = 0, m1 = admitted: the grand
 *              total of qp_ledger_recount).  A = 0: the zero root, a zero total,
 *              and every absence holds with no path;
 *   claim for account x: pos = the number of rows with an account below x, and
 *              found.  Found: the leaf at pos (the `hi` slot) has account x, and
 *              its total is what x is owed.  Not found: the leaf at pos - 1 (`lo`,
 *              if pos > 0) is below x and the leaf at pos (`hi`, if pos < A)
 *              above.  A slot the claim has no use for is all zero.
 * A claim holds only under the (claims_root, A) of its range.  The total is
 * published beside the root and binds nothing by itself: an auditor recomputes
 * it from the log (qp_ledger_log_claims_root).  The ledger keeps the commitment
 * of one range, keyed by (m0, m1): the log is append-only and final, so the same
 * range again launches nothing, and another range rebuilds.  Its buffers are its
 * own: no other call allocates, launches or copies anything for it, and a ledger
 * that never asks pays nothing.  With a context the range is credited into a
 * scratch account table (the payout round's launches), the owners are sorted by
 * account (the nullifier set's tile sort and merge passes), and the leaves, the
 * grand total, the levels, the search and the gathers run on the device.       */
/* the claims commitment of log entries [m0, m1): root_out, *count_out, total_out (each may be NULL) =
 * (claims_root, A, total).  m0 == m1: the empty commitment.  QP_ERR_ARG: m0 > m1, m1 > admitted   */
int qp_ledger_commit_claims(qp_ledger *l, uint64_t m0, uint64_t m1, uint64_t root_out[4], uint64_t *count_out,
                            uint32_t total_out[5]);
/* commits the range if it is not the one held, then the claims of accounts[0..k) ([k][4], canonical
 * felts, else QP_ERR_ARG naming the position before anything is enqueued): found [k], pos [k], and
 * per slot account [k][4], total [k][5], first_seq [k], siblings [k][32][4], bits [k], depth [k], a
 * path laid out as qp_ledger_set_proofs lays it out.  root_out, *count_out (either may be NULL) = the
 * pair the claims hold under.  k == 0: QP_OK, nothing beyond the commit                          */
int qp_ledger_claims(qp_ledger *l, uint64_t m0, uint64_t m1, const uint64_t *accounts, uint32_t k, uint8_t *found,
                     uint64_t *pos, uint64_t *lo_account, uint32_t *lo_total, uint64_t *lo_first_seq,
                     uint64_t *lo_siblings, uint32_t *lo_bits, uint32_t *lo_depth, uint64_t *hi_account,
                     uint32_t *hi_total, uint64_t *hi_first_seq, uint64_t *hi_siblings, uint32_t *hi_bits,
                     uint32_t *hi_depth, uint64_t root_out[4], uint64_t *count_out);
/* the auditor's side, from a published log alone (accounts_log [n][4], amounts [n][4], flags [n], 1
 * <= n <= 2^31); ctx == NULL: host.  root_out, *count_out, total_out (each may be NULL) as above;
 * order_out (may be NULL; room for m1 - m0) = the rows' first_seq in sorted order, A of them.  Only
 * the entries of [m0, m1) are read (with a context: uploaded).  Refusals and their error slot as
 * qp_ledger_log_payouts_between's                                                              */
int qp_ledger_log_claims_root(qp_ctx *ctx /* NULL: host */, const uint64_t *accounts_log, const uint32_t *amounts,
                              const uint8_t *flags, uint64_t n, uint64_t m0, uint64_t m1, uint64_t root_out[4],
                              uint64_t *count_out, uint32_t total_out[5], uint64_t *order_out);
/* checks one claim against a published (claims_root, A); host only, needs no ledger and no device.
 * siblings [32][4] each.  Returns QP_RECEIPT_OK or the first reason found, in qp_nullifier_set_check's
 * order: QP_RECEIPT_NULL; QP_RECEIPT_NON_CANONICAL (a felt >= p in root, x, an account, a first_seq
 * or the siblings); QP_RECEIPT_SHAPE (count > 2^31, pos > count, found > 1, found with pos == count,
 * a path whose depth or side bits are not the ones (j, count) gives, a non-zero sibling slot above
 * the depth, a slot the claim has no use for that is not all zero); QP_SET_ORDER (not lo.account < x
 * < hi.account, or found with an account other than x); QP_RECEIPT_ROOT.  Total limbs are in range
 * by their type                                                                                  */
int qp_ledger_claim_check(const uint64_t root[4], uint64_t count, const uint64_t x[4], uint32_t found, uint64_t pos,
                          const uint64_t lo_account[4], const uint32_t lo_total[5], uint64_t lo_first_seq,
                          const uint64_t *lo_siblings, uint32_t lo_bits, uint32_t lo_depth, const uint64_t hi_account[4],
                          const uint32_t hi_total[5], uint64_t hi_first_seq, const uint64_t *hi_siblings,
                          uint32_t hi_bits, uint32_t hi_depth);
/* the stage times (ms) of the last device build of a claims tree on this thread: ms[0..4) = credit
 * + compaction (with the scratch's allocation and the host's wait for A), tile sort, leaves + grand
 * total, levels; ms[4 + p] = merge pass p.  Returns the number written; 0: no build yet, or cap is
 * too small (36 always suffices)                                                                  */
uint32_t qp_ledger_claims_times(double *ms, uint32_t cap);

/* ---- routine-level seams ---------------------------------
 * The pieces of plonky2's prove() (qp-plonky2 1.1.1 plonk/prover.rs,
 * fri/prover.rs) a patched crate routes to the GPU for any circuit over the
 * supported gate set within the shape limits below — e.g. the aggregator's
 * per-chunk circuits (wormhole/aggregator/src/circuits/tree.rs:127-136).  The
 * Fiat-Shamir transcript stays with the caller (INTEGRATION.md shows the call
 * sequence).
 *
 * Shape limits (a call outside them returns QP_ERR_ARG with the reason in the
 * context's last error, never a wrong result): commitments of up to 2^16
 * values per polynomial with LDE domains up to 2^18 points (log_n + rate_bits
 * <= 18, i.e. circuits up to degree 2^15 at rate 3, the top of a 2048-leaf
 * aggregation tree, and the level-1 circuits of 5- to 7-ary trees);
 * qp_quotient: 2^6 <= degree <= 2^15 (the same kernels as the whole-circuit
 * prover; above 2^14 the coset iNTT runs its first levels in HBM), 2
 * challenges, quotient_degree_factor == 2^rate_bits <= 16, at most 16 gates,
 * unsalted batches of one; qp_fri_layer_commit: at most 2^16 nonzero
 * coefficients.                                                             */

/* gate kinds of CommonCircuitData.gates (DefaultGateSerializer ids in brackets).
 * 0-5: the leaf circuits' gates (fast single-read quotient kernel); 6-13: the
 * recursive-verifier gates of the aggregator circuits (tree.rs:106-143; generic
 * quotient kernel; parity unpinned: no reference fixture holds such a circuit). */
enum { QP_GATE_NOOP = 0 /* 9 */, QP_GATE_CONSTANT = 1 /* 3 */, QP_GATE_PUBLIC_INPUT = 2 /* 12 */,
       QP_GATE_BASE_SUM = 3 /* 2, BaseSumGate<2> */, QP_GATE_ARITHMETIC = 4 /* 0 */, QP_GATE_POSEIDON = 5 /* 11 */,
       QP_GATE_ARITHMETIC_EXTENSION = 6 /* 1 */, QP_GATE_MUL_EXTENSION = 7 /* 8 */,
       QP_GATE_RANDOM_ACCESS = 8 /* 13 */, QP_GATE_EXPONENTIATION = 9 /* 5 */, QP_GATE_REDUCING = 10 /* 15 */,
       QP_GATE_REDUCING_EXTENSION = 11 /* 14 */, QP_GATE_POSEIDON_MDS = 12 /* 10 */,
       QP_GATE_COSET_INTERPOLATION = 13 /* 4 */ };
#define QP_MAX_GATES 16

/* the parts of CommonCircuitData the vanishing polynomial reads */
typedef struct {
    uint32_t num_gates;                    /* <= QP_MAX_GATES, in CommonCircuitData.gates order */
    uint32_t kind[QP_MAX_GATES];           /* QP_GATE_* */
    uint32_t param[QP_MAX_GATES];          /* Constant num_consts, BaseSum num_limbs, Arithmetic(Extension) /
                                              MulExtension num_ops, RandomAccess bits, Exponentiation
                                              num_power_bits, Reducing(Extension) num_coeffs,
                                              CosetInterpolation subgroup_bits */
    uint32_t param2[QP_MAX_GATES];         /* RandomAccess num_copies, CosetInterpolation degree */
    uint32_t param3[QP_MAX_GATES];         /* RandomAccess num_extra_constants */
    uint32_t selector_index[QP_MAX_GATES]; /* selectors_info.selector_indices */
    uint32_t num_selectors;                /* selectors_info.groups.len() */
    uint32_t group_lo[QP_MAX_GATES], group_hi[QP_MAX_GATES];
    uint32_t num_constants;                /* selectors + gate constants */
    uint32_t num_routed_wires, num_wires, quotient_degree_factor, num_challenges, num_gate_constraints;
} qp_gate_desc;

/* fill a qp_gate_desc from a built circuit of this library */
int qp_circuit_gate_desc(const qp_circuit *c, qp_gate_desc *g);

/* compute_quotient_polys (plonk/prover.rs): vanishing polynomial at every
 * point of the LDE coset from the committed batches (constants||sigmas, wires,
 * zs||partial products; qp_commit_values batches of one, kept), alpha-reduced
 * per challenge, divided by Z_H, coset-iFFT'd and split:
 * quotient_coeffs_out [num_challenges * quotient_degree_factor][n].
 * betas/gammas/alphas [num_challenges] (num_challenges == 2), pi_hash =
 * hash_no_pad(public inputs).  Replaces prover.rs:compute_quotient_polys as
 * reached from CircuitData::prove (tree.rs:136, lib.rs:233-237).            */
int qp_quotient(qp_ctx *ctx, const qp_batch *cs, const qp_batch *wires, const qp_batch *zs_pp, const qp_gate_desc *g,
                const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas, const uint64_t pi_hash[4],
                uint64_t *quotient_coeffs_out);

/* one reduction layer of fri_committed_trees (fri/prover.rs): values =
 * coeffs.coset_fft(shift) of size 2^log_values, reverse_index_bits, leaves of
 * 2^arity_bits ext values, MerkleTree -> cap_out [2^cap_height][4].  coeffs are
 * ext coefficients as two rows [2][2^log_coeffs] (c0, c1); the reference keeps
 * them full length with a zero tail, so log_coeffs may equal log_values: only
 * the nonzero prefix (at most 2^16 coefficients) is transformed.  The caller
 * observes the cap, draws beta and calls qp_fri_fold; out (optional) keeps the
 * layer for qp_fri_layer_open in the query rounds.  A layer uses its context's
 * stream: free it (qp_fri_layer_free) before qp_ctx_destroy.                */
typedef struct qp_fri_layer qp_fri_layer;
int qp_fri_layer_commit(qp_ctx *ctx, const uint64_t *coeffs, uint32_t log_coeffs, uint32_t log_values, uint64_t shift,
                        uint32_t arity_bits, uint32_t cap_height, uint64_t *cap_out, qp_fri_layer **out);
/* leaf evals_out [nidx][2^arity_bits][2] (ext, c0 c1) and Merkle siblings
 * [nidx][log_leaves - cap_height][4] of layer leaves idx[]                 */
int qp_fri_layer_open(qp_fri_layer *layer, const uint32_t *idx, uint32_t nidx, uint64_t *evals_out,
                      uint64_t *siblings_out);
void qp_fri_layer_free(qp_fri_layer *layer);
/* coeffs_out[k] = sum_{i < 2^arity_bits} beta^i coeffs[2^arity_bits k + i]
 * (reduce_with_powers over chunks), ext rows [2][2^(log_coeffs - arity_bits)] */
int qp_fri_fold(qp_ctx *ctx, const uint64_t *coeffs, uint32_t log_coeffs, uint32_t arity_bits, const uint64_t beta[2],
                uint64_t *coeffs_out);

/* fri_proof_of_work (fri/prover.rs) for n transcripts: states [n][12] are the
 * duplex intermediate states (sponge_state with the pending input_buffer
 * written into lanes 0..pos-1), pos[b] = input_buffer.len() < 8.  Returns the
 * MINIMAL witness w with leading_zeros(permute(state with lane pos = w)[7])
 * >= pow_bits, 1 <= pow_bits <= 32 (the reference's rayon find_any returns any
 * such w).                                                                 */
int qp_pow_grind(qp_ctx *ctx, const uint64_t *states, const uint32_t *pos, uint32_t n, uint32_t pow_bits,
                 uint64_t *witness_out);

/* The three polynomial stages between the commitments (the whole-circuit
 * prover's stages 2, 4 and 5 for one proof of any circuit).  Limits of the
 * circuit-level calls (qp_partial_products_and_zs, qp_opening_set,
 * qp_fri_initial_poly): 2^6 <= degree <= 2^15 (qp_quotient's), 1 or 2
 * challenges, batches of one context and one log_n, unsalted, of one proof. */

/* permutation data of a circuit, uploaded once (the sigmas and k_is of
 * ProverOnlyCircuitData / CommonCircuitData):
 * sigmas: values over H, column-major [num_routed][2^log_n] (the sigma columns of
 * constants||sigmas); k_is [num_routed].  1 <= num_routed <= 256.  A qp_perm
 * uses its context: free it before qp_ctx_destroy.                          */
typedef struct qp_perm qp_perm;
int qp_perm_new(qp_ctx *ctx, const uint64_t *sigmas, const uint64_t *k_is, uint32_t num_routed,
                uint32_t log_n, qp_perm **out);
void qp_perm_free(qp_perm *p);

/* wires_permutation_partial_products_and_zs (plonk/prover.rs), reached from
 * CircuitData::prove (tree.rs:136, lib.rs:233-237) after the wires commitment.
 * wires: values over H, column-major, column stride 2^log_n; the first num_routed columns are read.
 * zs_pp_out [num_challenges * nchunks][2^log_n], nchunks = ceil(num_routed / quotient_degree_factor)
 * <= 16, in the order prove() commits them (all Zs, then the partial products per challenge): what
 * qp_commit_values takes next and what qp_quotient expects as zs_pp.  beta = 0 is legal.  A zero
 * denominator w + beta sigma + gamma (plonky2 panics in its batch inversion; probability about
 * num_routed * n / p per challenge for transcript-drawn challenges) is not detected, as in the
 * whole-circuit prover: its row quotient comes out as 0.                                         */
int qp_partial_products_and_zs(qp_perm *p, const uint64_t *wires, uint32_t quotient_degree_factor,
                               const uint64_t *betas, const uint64_t *gammas, uint32_t num_challenges,
                               uint64_t *zs_pp_out);

/* OpeningSet::new (plonk/proof.rs), reached from CircuitData::prove after zeta is drawn:
 * every polynomial of the four committed batches at zeta, in oracle order (constants||sigmas, wires,
 * Zs||partial products, quotient chunks), then the first num_challenges polynomials of zs_pp (the Zs)
 * at g*zeta: out [(sum of npolys) + num_challenges][2], at most 260 extension values (a
 * standard-config circuit has 257).  One launch (+ the slice reduction), one copy back.
 * zeta != 0 and zeta^n != 1 (plonky2's prover refuses the latter too).                           */
int qp_opening_set(qp_ctx *ctx, const qp_batch *cs, const qp_batch *wires, const qp_batch *zs_pp,
                   const qp_batch *quotient, uint32_t num_challenges, const uint64_t zeta[2], uint64_t *out);
/* the general form: polynomials [first, first + npolys) of one batch (of one proof, any log_n
 * qp_commit_values accepts) at npts extension points, out [npts][npolys][2], npts * npolys <= 2^20.
 * For other opening schedules and as the small-shape test surface.                               */
int qp_batch_eval_ext(const qp_batch *b, uint32_t first, uint32_t npolys, const uint64_t *points,
                      uint32_t npts, uint64_t *out);

/* the initial polynomial of PolynomialBatch::prove_openings (fri/oracle.rs), reached from
 * CircuitData::prove after the openings are observed and the FRI alpha is drawn:
 * alpha-reduce the zeta batch and the g*zeta batch, divide each by (X - point), combine as plonky2 does
 * (what stage 5 of the whole-circuit prover computes): coeffs_out [2][2^log_n] (c0 row, c1 row), the
 * layout qp_fri_layer_commit takes with log_coeffs = log_n.  zeta != 0 and zeta^n != 1.           */
int qp_fri_initial_poly(qp_ctx *ctx, const qp_batch *cs, const qp_batch *wires, const qp_batch *zs_pp,
                        const qp_batch *quotient, uint32_t num_challenges, const uint64_t alpha[2],
                        const uint64_t zeta[2], uint64_t *coeffs_out);

/* ---- batch proof verifier (plonky2 VerifierCircuitData::verify; the
 * reference's qp-wormhole-verifier, wormhole/verifier/src/lib.rs) ----------
 * Per proof the host parses, replays the transcript and checks the vanishing
 * identity and the PoW; the query rounds of the whole batch (Merkle paths, FRI
 * folding) run as two gfx950 kernels on the context's stream.              */
typedef struct qp_verifier qp_verifier;

/* verdict of one proof: plonky2's verify / verify_fri_proof checks in their order */
typedef enum {
    QP_VERIFY_OK = 0,
    QP_VERIFY_PUBLIC_INPUT_COUNT = 1,
    QP_VERIFY_ZETA_IN_SUBGROUP = 2,
    QP_VERIFY_VANISHING_IDENTITY = 3,
    QP_VERIFY_POW = 4,
    QP_VERIFY_INITIAL_MERKLE_PATH = 5,
    QP_VERIFY_FRI_CONSISTENCY = 6,
    QP_VERIFY_FRI_MERKLE_PATH = 7,
    QP_VERIFY_FINAL_POLY = 8,
    QP_VERIFY_MALFORMED = 9 /* wrong length, wrong sibling count, field element >= p */
} qp_verify_status;

/* plonky2 VerifierCircuitData: verifier_only = VerifierOnlyCircuitData bytes (cap height,
 * constants||sigmas cap, circuit digest), common = CommonCircuitData bytes.
 * ctx == NULL: everything runs on the host (no device needed).
 * Supported circuits: the gate set of this library's circuits (the six leaf
 * gates and the seven recursive-verifier gates), two challenges, no lookup
 * tables, salted (hiding) or not; anything else returns QP_ERR_FORMAT (with
 * *out set to a handle that only carries the reason for
 * qp_verifier_last_error; free it as usual).                               */
int qp_verifier_new(qp_ctx *ctx, const uint8_t *verifier_only, size_t vlen,
                    const uint8_t *common, size_t clen, uint32_t max_batch, qp_verifier **out);
void qp_verifier_free(qp_verifier *v);
const char *qp_verifier_last_error(const qp_verifier *v);
/* VerifierCircuitData::verify for n serialized ProofWithPublicInputs; status_out[i] is a
 * qp_verify_status. Returns QP_OK whenever the call itself completed, whatever the verdicts.
 * Where several checks fail the verdict is the first in plonky2's sequential
 * order (checks 1-4, then the lowest failing query; within it the four initial
 * trees, per layer consistency before the layer's path, the final polynomial).
 * n > max_batch is processed in chunks; a verdict never depends on the
 * neighbouring proofs.  Not thread-safe per handle.                         */
int qp_verifier_verify(qp_verifier *v, const uint8_t *const *proofs, const size_t *lens,
                       uint32_t n, uint32_t *status_out);
/* host threads of the per-proof work, the calling thread included (default:
 * the machine's, at most 16)                                               */
int qp_verifier_set_host_threads(qp_verifier *v, uint32_t nthreads);
/* verify_merkle_proof_to_cap for n independent (leaf, index, siblings) triples against one cap:
 * leaves [n][width], idx [n], siblings [n][nsib][4], cap [2^cap_height][4]; ok_out[i] = 0/1.
 * Routine-level seam; also the small-shape test surface of the path kernel.
 * An index past the tree (idx >> nsib >= 2^cap_height) gives 0.  Shapes:
 * width >= 1, nsib <= 32, cap_height <= 20, nsib + cap_height <= 32.  Unlike
 * the handle-based seams above it keeps nothing between calls: every call
 * allocates and frees its device buffers and copies from the caller's
 * (pageable) memory, so it is for checks and tests, not for a hot loop;
 * qp_verifier_verify keeps its buffers.                                     */
int qp_merkle_verify(qp_ctx *ctx, const uint64_t *leaves, uint32_t width, const uint32_t *idx,
                     const uint64_t *siblings, uint32_t nsib, const uint64_t *cap,
                     uint32_t cap_height, uint32_t n, uint8_t *ok_out);

/* ---- the input screen: prove a batch around its bad inputs --------------------
 * qp_prover_prove_wormhole_inputs fails as a whole on one inconsistent input and
 * names only the lowest.  The screen decides per input what the Wormhole circuit
 * decides (the constraints of csrc/wormhole.cpp, which restate wormhole/circuit/
 * src/{nullifier,unspendable_account,storage_proof/mod}.rs), without building a
 * witness: an input's status is the first of these checks that fails, in this
 * order, and `witness` says where:                                             */
typedef enum {
    QP_INPUT_OK = 0,             /* the circuit is satisfiable by this input; witness 0 */
    QP_INPUT_FIELD_RANGE = 1,    /* a 32-byte digest has an 8-byte chunk >= p (commit refuses these); witness = the
                                    lowest of 0 nullifier, 1 unspendable account, 2 root hash, 3 funding account,
                                    4 exit account */
    QP_INPUT_PROOF_TOO_LONG = 2, /* num_nodes > 20; witness = num_nodes */
    QP_INPUT_NODE_TOO_LARGE = 3, /* a node longer than 752 bytes (188 felts of 4 bytes); witness = the lowest such node */
    QP_INPUT_NULLIFIER = 4,      /* nullifier != H(H("~nullif~" || secret || transfer_count)); witness 0 */
    QP_INPUT_UNSPENDABLE = 5,    /* unspendable account != H(H("wormhole" || secret)); witness 0 */
    QP_INPUT_STORAGE_NODE = 6,   /* some node i < num_nodes does not hash (its 188 felts, zero-padded) to the root
                                    (i = 0) or to the digest found in node i - 1; witness = the lowest such i */
    QP_INPUT_STORAGE_LEAF = 7    /* num_nodes < 20 and felts 1..3 of the leaf hash differ from felts 1..3 of the
                                    digest found in the last node (of the root when num_nodes = 0); witness = num_nodes */
} qp_input_status;
/* The circuit's quirks are part of the definition: felt 0 of the leaf hash is
 * not compared, with 20 nodes the leaf is not checked at all, the digest found
 * in a node is zero when its hex index / 8 is 180 or more, the exit account is
 * unconstrained.  Statuses 1-3 are decided on the host.
 * screens in[0..n): status[n], witness[n].  With a context the hashes run on the
 * device, on the context's stream: one upload, two launches, one download; the
 * call allocates and frees its buffers.  ctx == NULL: the same rules in host
 * C++.  QP_OK: the screen ran, whatever it found.  QP_ERR_ARG for the whole
 * call: a null array, or an input whose nodes / node_lens / indices is null
 * with num_nodes > 0, or a null node with a length: programming errors, not bad
 * inputs.  zk_randomness is not read.  n == 0: QP_OK.                          */
int qp_wormhole_inputs_screen(qp_ctx *ctx /* NULL: host */, const qp_wormhole_inputs *in, uint32_t n,
                              uint32_t *status /* [n] */, uint32_t *witness /* [n] */);
/* one line of text for a qp_input_status (a static string; "unknown input status" beyond the enum) */
const char *qp_input_status_text(uint32_t status);
/* the screen (device path, the prover's context), then qp_prover_prove_wormhole_inputs' machinery,
 * unchanged, over the inputs with status 0, gathered in their order into dense batches of at most
 * max_batch: proof i at out + i * stride, the row of its ORIGINAL index, lens[i] its length; a bad
 * input gets lens[i] = 0 and its row is left alone.  QP_OK when the call ran, however many inputs
 * were bad; with no good input no witness or proving kernel is launched.  If an input the screen
 * passed still meets a witness conflict the call fails with QP_ERR_WITNESS and "input screen and
 * circuit disagree" before the prover's message: a bug in the screen, never hidden.  lens may be
 * NULL; status and witness may not.                                           */
int qp_prover_prove_wormhole_inputs_status(qp_prover *p, const qp_wormhole_inputs *in, uint32_t n, uint8_t *out,
                                           size_t stride, size_t *lens, uint32_t *status, uint32_t *witness);
/* times of this thread's last device-path qp_wormhole_inputs_screen (ms): [0] host checks and
 * packing (wall), HIP-event times of [1] the upload, [2] the node kernel, [3] the resolve kernel;
 * all 0 after a host-path call.  Diagnostic entry point (tools/screen_bench.py). */
int qp_wormhole_inputs_screen_times(double ms[4]);

#ifdef __cplusplus
}
#endif
#endif
