"""qp_wormhole — host-side mirror of the reference's prover API over the
MI355X-native C ABI (include/qpgpu.h, libqpgpu.so).

Mirrors qp-wormhole-prover's WormholeProver (wormhole/prover/src/lib.rs:74-237)
and plonky2's PolynomialBatch for the parity tests.  The HIP library is the
only backend: importing the native pieces raises if it is not built.
"""
from ._native import (GATE_KINDS, Context, FriLayer, GateDesc, PermutationData, PolynomialBatch, QpError,  # noqa: F401
                      debug_field_op, debug_poseidon_op, debug_witness_program, fri_fold, fri_initial_poly, gate_desc,
                      header_symbols, ifft, lde, lib, opening_set, poseidon_permute, pow_grind, quotient)

from .circuits import (Circuit, CircuitInputs, PrivateCircuitInputs, ProcessedStorageProof,  # noqa: F401,E402
                       PublicCircuitInputs, VoteCircuitData, VotePrivateInputs, VotePublicInputs, Witness)
from .prover import (Prover, ProofWithPublicInputs, WormholeProver, generate_circuit_binaries,  # noqa: F401,E402
                     prover_only_bytes)
from .aggregator import (AggregatedProof, CircuitData, TreeAggregationConfig, WormholeProofAggregator,  # noqa: F401,E402
                         aggregate_chunk, aggregate_level, aggregate_to_tree)
from .verifier import WormholeVerifier, merkle_verify  # noqa: F401,E402
from .registry import VoterRegistry  # noqa: F401,E402
from .ballot import (AUDIT_STATUS_TEXT, BALLOT_STATUS_TEXT, AuditReport, BallotBox, BallotReceipt,  # noqa: F401,E402
                     BallotResult, audit_log)
from .ledger import (LEDGER_AUDIT_STATUS_TEXT, TRANSFER_STATUS_TEXT, LedgerAuditReport, TransferReceipt,  # noqa: F401,E402
                     TransferResult, WormholeLedger, audit_ledger_log, ledger_log_claims_root, ledger_log_payouts)
from .claims import (CLAIM_CHECK_TEXT, ClaimLeaf, ClaimsCommitment, PayoutClaim, check_claim,  # noqa: F401,E402
                     check_claim_status, claims_times)
from .nullifier_set import (NullifierLeaf, NullifierProof, check_nullifier_proof, nullifier_set_root,  # noqa: F401,E402
                            nullifier_set_tile, nullifier_set_times)
from .screen import INPUT_STATUS_TEXT, InputStatus, screen_inputs  # noqa: F401,E402

__all__ = ["Circuit", "CircuitInputs", "PrivateCircuitInputs", "ProcessedStorageProof", "PublicCircuitInputs",
           "Witness", "VoteCircuitData", "VotePrivateInputs", "VotePublicInputs", "Prover", "ProofWithPublicInputs", "WormholeProver", "Context", "PolynomialBatch", "QpError", "ifft", "lde", "poseidon_permute", "lib", "header_symbols",
           "generate_circuit_binaries", "prover_only_bytes", "AggregatedProof", "CircuitData", "TreeAggregationConfig",
           "WormholeProofAggregator", "aggregate_chunk", "aggregate_level", "aggregate_to_tree", "GateDesc", "gate_desc", "quotient", "FriLayer", "fri_fold", "pow_grind",
           "PermutationData", "opening_set", "fri_initial_poly",
           "WormholeVerifier", "merkle_verify", "VoterRegistry", "BallotBox", "BallotResult", "BallotReceipt",
           "BALLOT_STATUS_TEXT", "AuditReport", "AUDIT_STATUS_TEXT", "audit_log",
           "WormholeLedger", "TransferResult", "TRANSFER_STATUS_TEXT", "TransferReceipt", "LedgerAuditReport",
           "LEDGER_AUDIT_STATUS_TEXT", "audit_ledger_log", "ledger_log_payouts", "INPUT_STATUS_TEXT", "InputStatus", "screen_inputs",
           "NullifierLeaf", "NullifierProof", "check_nullifier_proof", "nullifier_set_root", "nullifier_set_tile",
           "nullifier_set_times", "ledger_log_claims_root", "CLAIM_CHECK_TEXT", "ClaimLeaf", "ClaimsCommitment",
           "PayoutClaim", "check_claim", "check_claim_status", "claims_times"]
