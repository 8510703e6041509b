"""ctypes binding of libqpgpu.so (include/qpgpu.h).

The product path is the HIP library only: if libqpgpu.so is missing or cannot
be loaded this module raises, there is no CPU fallback.
"""
import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QPGPU_LIB") or os.path.join(HERE, "libqpgpu.so")  # QPGPU_LIB: A/B tuning builds
HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "qpgpu.h")

U64P = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
U32P = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
U8P = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
VP = ctypes.c_void_p
PP = ctypes.POINTER(ctypes.c_void_p)

STATUS = {0: "QP_OK", 1: "QP_ERR_ARG", 2: "QP_ERR_HIP", 3: "QP_ERR_OOM", 4: "QP_ERR_STATE",
          5: "QP_ERR_WITNESS", 6: "QP_ERR_FORMAT"}


MAX_GATES = 16
GATE_KINDS = ["noop", "constant", "public_input", "base_sum", "arithmetic", "poseidon", "arithmetic_extension",
              "mul_extension", "random_access", "exponentiation", "reducing", "reducing_extension", "poseidon_mds",
              "coset_interpolation"]  # QP_GATE_* order


class GateDesc(ctypes.Structure):
    """qp_gate_desc: the parts of CommonCircuitData the vanishing polynomial reads."""
    _fields_ = [("num_gates", ctypes.c_uint32), ("kind", ctypes.c_uint32 * MAX_GATES),
                ("param", ctypes.c_uint32 * MAX_GATES), ("param2", ctypes.c_uint32 * MAX_GATES),
                ("param3", ctypes.c_uint32 * MAX_GATES), ("selector_index", ctypes.c_uint32 * MAX_GATES),
                ("num_selectors", ctypes.c_uint32), ("group_lo", ctypes.c_uint32 * MAX_GATES),
                ("group_hi", ctypes.c_uint32 * MAX_GATES), ("num_constants", ctypes.c_uint32),
                ("num_routed_wires", ctypes.c_uint32), ("num_wires", ctypes.c_uint32),
                ("quotient_degree_factor", ctypes.c_uint32), ("num_challenges", ctypes.c_uint32),
                ("num_gate_constraints", ctypes.c_uint32)]

    @classmethod
    def build(cls, gates, groups, num_wires=135, num_routed_wires=80, num_gate_constants=2, rate_bits=3,
              num_gate_constraints=None):
        """gates: [(kind name, params tuple, selector index)], groups: [(lo, hi)]"""
        g = cls()
        g.num_gates = len(gates)
        for i, (kind, params, sel) in enumerate(gates):
            g.kind[i] = GATE_KINDS.index(kind)
            params = tuple(params) + (0, 0, 0)
            g.param[i], g.param2[i], g.param3[i] = params[:3]
            g.selector_index[i] = sel
        g.num_selectors = len(groups)
        for i, (lo, hi) in enumerate(groups):
            g.group_lo[i], g.group_hi[i] = lo, hi
        g.num_constants = len(groups) + num_gate_constants
        g.num_routed_wires, g.num_wires = num_routed_wires, num_wires
        g.quotient_degree_factor, g.num_challenges = 1 << rate_bits, 2
        g.num_gate_constraints = num_gate_constraints or 0
        return g


class WitnessProgram(ctypes.Structure):
    """qp_witness_program: a generator program for the TEST-ONLY qp_debug_witness_program."""
    _fields_ = [("gens", VP), ("ngens", ctypes.c_uint32), ("level_off", VP), ("level_pos", VP),
                ("nlevels", ctypes.c_uint32), ("wslot", VP), ("nrows", ctypes.c_uint32), ("W", ctypes.c_uint32),
                ("nslots", ctypes.c_uint32), ("limbs", ctypes.c_uint32), ("zero_slot", ctypes.c_uint32),
                ("num_consts", ctypes.c_uint32), ("in_slots", VP), ("in_vals", VP), ("nin", ctypes.c_uint32),
                ("B", ctypes.c_uint32), ("form", ctypes.c_uint32), ("wslot_cm", VP), ("pi_slots", VP),
                ("npis", ctypes.c_uint32)]


class QpError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__(f"{STATUS.get(code, code)}: {msg}")


_lib = None


def header_symbols():
    """Function names declared in include/qpgpu.h."""
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\s+\*?\s*(qp_\w+)\s*\(", txt, re.M)))


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(LIB_PATH)
    sig = {
        "qp_version": (ctypes.c_char_p, []),
        "qp_ctx_create": (ctypes.c_int, [ctypes.c_int, PP]),
        "qp_ctx_destroy": (None, [VP]),
        "qp_ctx_last_error": (ctypes.c_char_p, [VP]),
        "qp_ctx_set_stream": (ctypes.c_int, [VP, VP]),
        "qp_ctx_set_priority": (ctypes.c_int, [VP, ctypes.c_int]),
        "qp_ctx_synchronize": (ctypes.c_int, [VP]),
        "qp_commit_values": (ctypes.c_int, [VP, U64P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_uint32, VP, ctypes.c_uint32, VP, U64P, PP]),
        "qp_commit_coeffs": (ctypes.c_int, [VP, U64P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_uint32, VP, ctypes.c_uint32, U64P, PP]),
        "qp_commit_values_dev": (ctypes.c_int, [VP, VP, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                ctypes.c_uint32, ctypes.c_uint32, VP, PP]),
        "qp_batch_open": (ctypes.c_int, [VP, U32P, ctypes.c_uint32, U64P, U64P]),
        "qp_batch_lde": (ctypes.c_int, [VP, U64P]),
        "qp_batch_coeffs": (ctypes.c_int, [VP, U64P]),
        "qp_batch_free": (None, [VP]),
        "qp_ifft": (ctypes.c_int, [VP, U64P, ctypes.c_uint32, ctypes.c_uint32]),
        "qp_lde": (ctypes.c_int, [VP, U64P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                                  U64P]),
        "qp_poseidon_permute": (ctypes.c_int, [VP, U64P, ctypes.c_uint64]),
        "qp_wormhole_circuit_new": (ctypes.c_int, [ctypes.c_int, PP]),
        "qp_circuit_free": (None, [VP]),
        "qp_circuit_info": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_uint32)]),
        "qp_circuit_host_chains": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                                   ctypes.POINTER(ctypes.c_uint32)]),
        "qp_circuit_census": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                              ctypes.POINTER(ctypes.c_uint32)]),
        "qp_circuit_common_data": (ctypes.c_int, [VP, ctypes.c_char_p, ctypes.c_size_t,
                                                  ctypes.POINTER(ctypes.c_size_t)]),
        "qp_circuit_constants_sigmas": (ctypes.c_int, [VP, U64P]),
        "qp_circuit_constants_sigmas_coeffs": (ctypes.c_int, [VP, U64P]),
        "qp_circuit_prover_only_bytes": (ctypes.c_int, [VP, ctypes.c_char_p, ctypes.c_size_t,
                                                        ctypes.POINTER(ctypes.c_size_t)]),
        "qp_wormhole_commit": (ctypes.c_int, [VP, VP, PP, ctypes.c_char_p, ctypes.c_size_t]),
        "qp_voting_circuit_new": (ctypes.c_int, [ctypes.c_int, PP]),
        "qp_voting_commit": (ctypes.c_int, [VP, VP, PP, ctypes.c_char_p, ctypes.c_size_t]),
        "qp_aggregation_circuit_new": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, PP]),
        "qp_aggregation_commit": (ctypes.c_int, [VP, ctypes.c_char_p, ctypes.c_size_t, VP, VP, ctypes.c_uint32,
                                                 VP, PP, ctypes.c_char_p, ctypes.c_size_t]),
        "qp_witness_wires": (ctypes.c_int, [VP, U64P]),
        "qp_witness_public_inputs": (ctypes.c_int, [VP, VP, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
        "qp_witness_free": (None, [VP]),
        "qp_hash_no_pad": (ctypes.c_int, [U64P, ctypes.c_size_t, U64P]),
        "qp_prover_new": (ctypes.c_int, [VP, VP, ctypes.c_uint32, PP]),
        "qp_prover_free": (None, [VP]),
        "qp_prover_proof_size": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_size_t)]),
        "qp_prover_verifier_data": (ctypes.c_int, [VP, ctypes.c_char_p, ctypes.c_size_t,
                                                   ctypes.POINTER(ctypes.c_size_t)]),
        "qp_prover_prove": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_char_p,
                                           ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "qp_prover_prove_wires": (ctypes.c_int, [VP, U64P, U64P, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t,
                                                 ctypes.POINTER(ctypes.c_size_t)]),
        "qp_prover_prove_wires_dev": (ctypes.c_int, [VP, VP, U64P, ctypes.c_uint32, ctypes.c_char_p,
                                                     ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "qp_prover_prove_wormhole_inputs": (ctypes.c_int, [VP, VP, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t,
                                                           ctypes.POINTER(ctypes.c_size_t)]),
        "qp_prover_prove_voting_inputs": (ctypes.c_int, [VP, VP, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t,
                                                         ctypes.POINTER(ctypes.c_size_t)]),
        "qp_wormhole_inputs_screen": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP, VP]),
        "qp_input_status_text": (ctypes.c_char_p, [ctypes.c_uint32]),
        "qp_prover_prove_wormhole_inputs_status": (ctypes.c_int, [VP, VP, ctypes.c_uint32, ctypes.c_char_p,
                                                                  ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                                                  VP, VP]),
        "qp_wormhole_inputs_screen_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double)]),
        "qp_prover_prove_aggregation": (ctypes.c_int, [VP, VP, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t,
                                                       ctypes.POINTER(ctypes.c_size_t)]),
        "qp_registry_new": (ctypes.c_int, [VP, U64P, ctypes.c_uint64, PP]),
        "qp_registry_free": (None, [VP]),
        "qp_registry_root": (ctypes.c_int, [VP, U64P]),
        "qp_registry_size": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]),
        "qp_registry_paths": (ctypes.c_int, [VP, U64P, ctypes.c_uint32, U64P, U32P, U32P]),
        "qp_registry_level": (ctypes.c_int, [VP, ctypes.c_uint32, VP, ctypes.POINTER(ctypes.c_uint64)]),
        "qp_registry_build_times": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_double)]),
        "qp_registry_new_commitments": (ctypes.c_int, [VP, VP, ctypes.c_uint64, ctypes.c_uint64, PP]),
        "qp_registry_append": (ctypes.c_int, [VP, VP, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        "qp_registry_replace": (ctypes.c_int, [VP, VP, VP, ctypes.c_uint32]),
        "qp_registry_reserve": (ctypes.c_int, [VP, ctypes.c_uint64]),
        "qp_registry_state": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "qp_prover_prove_voters": (ctypes.c_int, [VP, VP, U64P, VP, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t,
                                                  ctypes.POINTER(ctypes.c_size_t)]),
        "qp_ballot_box_new": (ctypes.c_int, [VP, U64P, U64P, ctypes.c_uint32, ctypes.c_uint64, PP]),
        "qp_ballot_box_free": (None, [VP]),
        "qp_ballot_box_last_error": (ctypes.c_char_p, [VP]),
        "qp_ballot_box_accept_root": (ctypes.c_int, [VP, U64P]),
        "qp_ballot_box_cast": (ctypes.c_int, [VP, VP, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t),
                                              ctypes.c_uint32, VP]),
        "qp_ballot_box_cast_public": (ctypes.c_int, [VP, VP, VP, ctypes.c_uint32, VP]),
        "qp_ballot_box_reserve": (ctypes.c_int, [VP, ctypes.c_uint64]),
        "qp_ballot_box_tally": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ballot_box_state": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                               ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ballot_box_entries": (ctypes.c_int, [VP, ctypes.c_uint64, ctypes.c_uint64, VP, VP, VP]),
        "qp_ballot_box_recount": (ctypes.c_int, [VP, U64P]),
        "qp_ballot_box_cast_times": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_double)]),
        "qp_ballot_box_find": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP]),
        "qp_ballot_box_commit_log": (ctypes.c_int, [VP, VP, ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ballot_box_receipts": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP, VP, VP, VP, VP,
                                                  ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ballot_box_entries_at": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP, VP, VP]),
        "qp_ballot_receipt_check": (ctypes.c_int, [VP, ctypes.c_uint64, ctypes.c_uint64, VP, ctypes.c_uint64,
                                                   ctypes.c_uint8, VP, ctypes.c_uint32, ctypes.c_uint32]),
        "qp_ballot_log_audit": (ctypes.c_int, [VP, VP, VP, VP, ctypes.c_uint64, VP, VP, VP, VP, ctypes.c_uint32, VP]),
        "qp_ballot_box_roots_at": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP]),
        "qp_ballot_box_restore": (ctypes.c_int, [VP, U64P, U64P, ctypes.c_uint32, ctypes.c_uint64, VP, VP, VP,
                                                 ctypes.c_uint64, ctypes.c_uint64, VP, PP]),
        "qp_ledger_new": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP, ctypes.c_uint64, PP]),
        "qp_ledger_free": (None, [VP]),
        "qp_ledger_last_error": (ctypes.c_char_p, [VP]),
        "qp_ledger_accept_root": (ctypes.c_int, [VP, VP]),
        "qp_ledger_reserve": (ctypes.c_int, [VP, ctypes.c_uint64]),
        "qp_ledger_state": (ctypes.c_int, [VP] + [ctypes.POINTER(ctypes.c_uint64)] * 5),
        "qp_ledger_cast": (ctypes.c_int, [VP, VP, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t),
                                          ctypes.c_uint32, VP]),
        "qp_ledger_cast_public": (ctypes.c_int, [VP, VP, VP, ctypes.c_uint32, VP]),
        "qp_ledger_find": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP]),
        "qp_ledger_entries": (ctypes.c_int, [VP, ctypes.c_uint64, ctypes.c_uint64, VP, VP, VP, VP, VP]),
        "qp_ledger_payouts": (ctypes.c_int, [VP, ctypes.c_uint64, ctypes.c_uint64, VP, VP, VP]),
        "qp_ledger_totals_for": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP, VP]),
        "qp_ledger_recount": (ctypes.c_int, [VP, VP]),
        "qp_ledger_cast_times": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_double)]),
        "qp_ledger_commit_log": (ctypes.c_int, [VP, VP, ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ledger_entries_at": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP, VP, VP, VP, VP]),
        "qp_ledger_receipts": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP, VP, VP, VP, VP,
                                              ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ledger_roots_at": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP]),
        "qp_ledger_receipt_check": (ctypes.c_int, [VP, ctypes.c_uint64, ctypes.c_uint64, VP, ctypes.c_uint64, VP, VP,
                                                   ctypes.c_uint8, VP, ctypes.c_uint32, ctypes.c_uint32]),
        "qp_ledger_log_audit": (ctypes.c_int, [VP, VP, VP, VP, VP, VP, ctypes.c_uint64, VP, VP, VP, VP, VP,
                                               ctypes.c_uint64, VP, VP, ctypes.c_uint32, VP]),
        "qp_ledger_restore": (ctypes.c_int, [VP, VP, ctypes.c_uint32, VP, ctypes.c_uint64, VP, VP, VP, VP, VP,
                                             ctypes.c_uint64, ctypes.c_uint64, VP, PP]),
        "qp_ledger_payouts_between": (ctypes.c_int, [VP, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, VP, VP, VP,
                                                     ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ledger_log_payouts_between": (ctypes.c_int, [VP, VP, VP, VP, ctypes.c_uint64, ctypes.c_uint64,
                                                         ctypes.c_uint64, ctypes.c_uint64, VP, VP, VP,
                                                         ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ballot_box_commit_set": (ctypes.c_int, [VP, VP, ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ledger_commit_set": (ctypes.c_int, [VP, VP, ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ballot_box_set_proofs": (ctypes.c_int, [VP, VP, ctypes.c_uint32] + [VP] * 12 +
                                     [VP, ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ledger_set_proofs": (ctypes.c_int, [VP, VP, ctypes.c_uint32] + [VP] * 12 +
                                 [VP, ctypes.POINTER(ctypes.c_uint64)]),
        "qp_nullifier_set_root": (ctypes.c_int, [VP, VP, VP, ctypes.c_uint64, VP, ctypes.POINTER(ctypes.c_uint64), VP,
                                                 ctypes.POINTER(ctypes.c_uint64)]),
        "qp_nullifier_set_last_error": (ctypes.c_char_p, []),
        "qp_nullifier_set_check": (ctypes.c_int, [VP, ctypes.c_uint64, VP, ctypes.c_uint32, ctypes.c_uint64] +
                                   [VP, ctypes.c_uint64, VP, ctypes.c_uint32, ctypes.c_uint32] * 2),
        "qp_nullifier_set_tile": (ctypes.c_uint32, []),
        "qp_nullifier_set_times": (ctypes.c_uint32, [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]),
        "qp_ledger_commit_claims": (ctypes.c_int, [VP, ctypes.c_uint64, ctypes.c_uint64, VP,
                                                   ctypes.POINTER(ctypes.c_uint64), VP]),
        "qp_ledger_claims": (ctypes.c_int, [VP, ctypes.c_uint64, ctypes.c_uint64, VP, ctypes.c_uint32] + [VP] * 14 +
                             [VP, ctypes.POINTER(ctypes.c_uint64)]),
        "qp_ledger_log_claims_root": (ctypes.c_int, [VP, VP, VP, VP, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                     VP, ctypes.POINTER(ctypes.c_uint64), VP, VP]),
        "qp_ledger_claim_check": (ctypes.c_int, [VP, ctypes.c_uint64, VP, ctypes.c_uint32, ctypes.c_uint64] +
                                  [VP, VP, ctypes.c_uint64, VP, ctypes.c_uint32, ctypes.c_uint32] * 2),
        "qp_ledger_claims_times": (ctypes.c_uint32, [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]),
        "qp_prover_set_timing": (ctypes.c_int, [VP, ctypes.c_int]),
        "qp_prover_debug_force_pow": (ctypes.c_int, [VP, ctypes.c_uint64, ctypes.c_int]),
        "qp_prover_debug_drop_table": (ctypes.c_int, [VP, ctypes.c_char_p]),
        "qp_debug_field_op": (ctypes.c_int, [VP, ctypes.c_uint32, ctypes.c_uint32, U64P, VP, ctypes.c_uint64, U64P]),
        "qp_debug_poseidon_op": (ctypes.c_int, [VP, ctypes.c_uint32, ctypes.c_uint32, VP, ctypes.c_uint64, VP]),
        "qp_debug_witness_program": (ctypes.c_int, [VP, ctypes.POINTER(WitnessProgram), VP, VP, VP, VP]),
        "qp_prover_set_host_threads": (ctypes.c_int, [VP, ctypes.c_uint32]),
        "qp_prover_kernel_stats": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                  ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_int]),
        "qp_prover_stage_times": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_double), ctypes.c_uint32, ctypes.c_int]),
        "qp_circuit_gate_desc": (ctypes.c_int, [VP, ctypes.POINTER(GateDesc)]),
        "qp_quotient": (ctypes.c_int, [VP, VP, VP, VP, ctypes.POINTER(GateDesc), U64P, U64P, U64P, U64P, U64P]),
        "qp_fri_layer_commit": (ctypes.c_int, [VP, U64P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                                               ctypes.c_uint32, ctypes.c_uint32, U64P, PP]),
        "qp_fri_layer_open": (ctypes.c_int, [VP, U32P, ctypes.c_uint32, U64P, U64P]),
        "qp_fri_layer_free": (None, [VP]),
        "qp_fri_fold": (ctypes.c_int, [VP, U64P, ctypes.c_uint32, ctypes.c_uint32, U64P, U64P]),
        "qp_pow_grind": (ctypes.c_int, [VP, U64P, U32P, ctypes.c_uint32, ctypes.c_uint32, U64P]),
        "qp_perm_new": (ctypes.c_int, [VP, U64P, U64P, ctypes.c_uint32, ctypes.c_uint32, PP]),
        "qp_perm_free": (None, [VP]),
        "qp_partial_products_and_zs": (ctypes.c_int, [VP, U64P, ctypes.c_uint32, U64P, U64P, ctypes.c_uint32, U64P]),
        "qp_opening_set": (ctypes.c_int, [VP, VP, VP, VP, VP, ctypes.c_uint32, U64P, U64P]),
        "qp_batch_eval_ext": (ctypes.c_int, [VP, ctypes.c_uint32, ctypes.c_uint32, U64P, ctypes.c_uint32, U64P]),
        "qp_fri_initial_poly": (ctypes.c_int, [VP, VP, VP, VP, VP, ctypes.c_uint32, U64P, U64P, U64P]),
        "qp_verifier_new": (ctypes.c_int, [VP, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                           ctypes.c_uint32, PP]),
        "qp_verifier_free": (None, [VP]),
        "qp_verifier_last_error": (ctypes.c_char_p, [VP]),
        "qp_verifier_verify": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t),
                                              ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
        "qp_verifier_set_host_threads": (ctypes.c_int, [VP, ctypes.c_uint32]),
        "qp_merkle_verify": (ctypes.c_int, [VP, U64P, ctypes.c_uint32, U32P, U64P, ctypes.c_uint32, U64P,
                                            ctypes.c_uint32, ctypes.c_uint32, U8P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


class Context:
    """One HIP stream on one device (qp_ctx)."""

    def __init__(self, device=0):
        L = lib()
        h = ctypes.c_void_p()
        rc = L.qp_ctx_create(device, ctypes.byref(h))
        if rc:
            raise QpError(rc, f"qp_ctx_create(device={device})")
        self.h = h

    def check(self, rc, what=""):
        if rc:
            raise QpError(rc, f"{what}: {lib().qp_ctx_last_error(self.h).decode()}")

    def set_priority(self, high=True):
        """Own stream at the device's greatest (or the default) priority."""
        self.check(lib().qp_ctx_set_priority(self.h, int(bool(high))), "set_priority")

    def close(self):
        if self.h:
            lib().qp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        self.check(lib().qp_ctx_set_stream(self.h, stream_ptr), "set_stream")

    def synchronize(self):
        self.check(lib().qp_ctx_synchronize(self.h), "synchronize")


class PolynomialBatch:
    """Device-resident committed polynomial batch (plonky2 PolynomialBatch)."""

    def __init__(self, ctx, handle, npolys, nsalt, log_n, rate_bits, cap_height, cap, coeffs=None):
        self.ctx, self.h = ctx, handle
        self.npolys, self.nsalt, self.log_n, self.rate_bits, self.cap_height = npolys, nsalt, log_n, rate_bits, cap_height
        self.cap, self.coeffs = cap, coeffs

    @classmethod
    def from_values(cls, ctx, values, rate_bits, cap_height, salt=None, keep=True):
        values = np.ascontiguousarray(values, dtype=np.uint64)
        npolys, n = values.shape
        log_n = n.bit_length() - 1
        nsalt = 0 if salt is None else salt.shape[1]
        salt_c = None if salt is None else np.ascontiguousarray(salt, dtype=np.uint64)
        coeffs = np.zeros_like(values)
        cap = np.zeros(((1 << cap_height), 4), np.uint64)
        h = ctypes.c_void_p()
        rc = lib().qp_commit_values(ctx.h, values, npolys, log_n, rate_bits, cap_height,
                                    None if salt_c is None else salt_c.ctypes.data, nsalt, coeffs.ctypes.data, cap,
                                    ctypes.byref(h) if keep else None)
        ctx.check(rc, "qp_commit_values")
        return cls(ctx, h if keep else None, npolys, nsalt, log_n, rate_bits, cap_height, cap, coeffs)

    @classmethod
    def from_coeffs(cls, ctx, coeffs, rate_bits, cap_height, salt=None, keep=True):
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
        npolys, n = coeffs.shape
        log_n = n.bit_length() - 1
        nsalt = 0 if salt is None else salt.shape[1]
        salt_c = None if salt is None else np.ascontiguousarray(salt, dtype=np.uint64)
        cap = np.zeros(((1 << cap_height), 4), np.uint64)
        h = ctypes.c_void_p()
        rc = lib().qp_commit_coeffs(ctx.h, coeffs, npolys, log_n, rate_bits, cap_height,
                                    None if salt_c is None else salt_c.ctypes.data, nsalt, cap,
                                    ctypes.byref(h) if keep else None)
        ctx.check(rc, "qp_commit_coeffs")
        return cls(ctx, h if keep else None, npolys, nsalt, log_n, rate_bits, cap_height, cap, coeffs)

    def open(self, indices):
        idx = np.ascontiguousarray(indices, dtype=np.uint32)
        W = self.npolys + self.nsalt
        depth = self.log_n + self.rate_bits - self.cap_height
        leaves = np.zeros((len(idx), W), np.uint64)
        sibs = np.zeros((len(idx), depth, 4), np.uint64)
        self.ctx.check(lib().qp_batch_open(self.h, idx, len(idx), leaves, sibs), "qp_batch_open")
        return leaves, sibs

    def eval_ext(self, points, first=0, npolys=None):
        """qp_batch_eval_ext: polynomials [first, first + npolys) at the extension
        points [npts][2]; returns [npts][npolys][2]."""
        pts = _ext_points(points)
        npolys = self.npolys - first if npolys is None else npolys
        if first < 0 or npolys < 1 or first + npolys > self.npolys:
            raise ValueError(f"window [{first}, {first + npolys}) outside the batch's {self.npolys} polynomials")
        out = np.zeros((pts.shape[0], npolys, 2), np.uint64)
        self.ctx.check(lib().qp_batch_eval_ext(self.h, first, npolys, pts, pts.shape[0], out), "qp_batch_eval_ext")
        return out

    def lde(self):
        out = np.zeros((self.npolys, 1 << (self.log_n + self.rate_bits)), np.uint64)
        self.ctx.check(lib().qp_batch_lde(self.h, out), "qp_batch_lde")
        return out

    def free(self):
        if self.h:
            lib().qp_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def ifft(ctx, data):
    a = np.ascontiguousarray(data, dtype=np.uint64).copy()
    ncols, n = a.shape
    ctx.check(lib().qp_ifft(ctx.h, a, ncols, n.bit_length() - 1), "qp_ifft")
    return a


def lde(ctx, coeffs, rate_bits, shift=0xC65C18B67785D900):
    c = np.ascontiguousarray(coeffs, dtype=np.uint64)
    ncols, n = c.shape
    out = np.zeros((ncols, n << rate_bits), np.uint64)
    ctx.check(lib().qp_lde(ctx.h, c, ncols, n.bit_length() - 1, rate_bits, shift, out), "qp_lde")
    return out


def poseidon_permute(ctx, states):
    s = np.ascontiguousarray(states, dtype=np.uint64).copy()
    ctx.check(lib().qp_poseidon_permute(ctx.h, s, s.shape[0]), "qp_poseidon_permute")
    return s


# qp_debug_field_op codes (include/qpgpu.h QP_FOP_*)
(FOP_NT_ADD, FOP_NT_ADD4, FOP_GFN_ADD, FOP_GFN_ADD_C, FOP_PF_ADD_C, FOP_GL_ADD, FOP_NT_SUB, FOP_NT_SUB4, FOP_GL_SUB,
 FOP_NT_REDUCE, FOP_GFN_REDUCE, FOP_GL_REDUCE128, FOP_PF_REDUCE_ROW, FOP_PF_REDUCE_ROW_C, FOP_PF_SUB_SMALL,
 FOP_PF_MUL, FOP_PF_MUL_C, FOP_PF_MULK2, FOP_PF_MULK3, FOP_GL_MUL, FOP_PF_SBOX, FOP_PF_SBOX_C, FOP_NT_MUL_POW2,
 FOP_ACC3, FOP_PF_REDUCE_ROW_WIDE, FOP_COUNT) = range(26)


def debug_field_op(ctx, op, a, b=None, param=0):
    """TEST-ONLY (qp_debug_field_op): the device function `op` on a[i], b[i],
    raw u64 results (one per element; FOP_ACC3: one per group of `param`)."""
    a = np.ascontiguousarray(a, dtype=np.uint64).ravel()
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.uint64).ravel()
        if b.size != a.size:
            raise ValueError("a and b differ in length")
    nout = a.size // param if op == FOP_ACC3 and param and a.size % param == 0 else a.size
    out = np.zeros(nout, np.uint64)
    ctx.check(lib().qp_debug_field_op(ctx.h, int(op), int(param), a, None if b is None else b.ctypes.data, a.size,
                                      out), "qp_debug_field_op")
    return out


# qp_debug_poseidon_op forms (include/qpgpu.h QP_PFORM_*)
(PFORM_PERMUTE_NC, PFORM_PERMUTE_CAPZ, PFORM_ROUNDS1_L7, PFORM_COOP_PERMUTE, PFORM_ROW_PERMUTE, PFORM_MDS_BLOCK,
 PFORM_MDS_K, PFORM_MDS_MADS, PFORM_CAPZ_ROUND0, PFORM_MDS_INIT_SPARSE, PFORM_PARTIAL_GROUP, PFORM_FULL_ROUND_DYN,
 PFORM_PARTIAL_DYN, PFORM_COOP_MDS, PFORM_ROW_MDS, PFORM_DENSE_GROUP, PFORM_COUNT) = range(17)
# forms added after those: PFORM_COUNT stays the first id the forms above reject
PFORM_DENSE_GROUP4 = PFORM_COUNT + 1


def debug_poseidon_op(ctx, form, states, param=0):
    """TEST-ONLY (qp_debug_poseidon_op): the device Poseidon form `form` on
    states[i] (12 words each); raw u64 results, [nstates][12].  states=None
    passes a null pointer (with one state claimed)."""
    if states is None:
        n, src = 1, None
    else:
        s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 12)
        n, src = s.shape[0], s.ctypes.data
    out = np.zeros((n, 12), np.uint64)
    ctx.check(lib().qp_debug_poseidon_op(ctx.h, int(form), int(param), src, n, out.ctypes.data),
              "qp_debug_poseidon_op")
    return out


# qp_debug_witness_program forms (include/qpgpu.h QP_WFORM_*)
(WFORM_PROOF_256, WFORM_PROOF_512, WFORM_LEVEL_ROW, WFORM_LEVEL_WAVE, WFORM_PROOF_256_WAVE, WFORM_PROOF_512_WAVE,
 WFORM_COUNT) = range(7)


def debug_witness_program(ctx, form, gens, level_off, level_pos, wslot, nslots, in_slots, in_vals, limbs=63,
                          zero_slot=0, num_consts=2, wslot_cm=None, pi_slots=None):
    """TEST-ONLY (qp_debug_witness_program): the generator program through the
    production witness kernels under scheduler `form`.  gens [ngens][5] u64
    (DevGen words), level_off [nlevels + 1], level_pos [nlevels][2], wslot
    [nrows][W], in_vals [B][nin].  Returns (vals [B][nslots] raw, err [B]), and
    with wslot_cm ([W][nrows]) also (wires [B][W][nrows], pis [B][npis])."""
    gens = np.ascontiguousarray(gens, dtype=np.uint64).reshape(-1, 5)
    level_off = np.ascontiguousarray(level_off, dtype=np.uint32).ravel()
    level_pos = np.ascontiguousarray(level_pos, dtype=np.uint32).reshape(-1, 2)
    wslot = np.ascontiguousarray(wslot, dtype=np.uint32)
    if wslot.ndim != 2:
        raise ValueError("wslot is [nrows][W]")
    in_slots = np.ascontiguousarray(in_slots, dtype=np.uint32).ravel()
    in_vals = np.ascontiguousarray(in_vals, dtype=np.uint64)
    if in_vals.ndim != 2 or in_vals.shape[1] != in_slots.size:
        raise ValueError("in_vals is [B][nin]")
    if level_off.size != level_pos.shape[0] + 1:
        raise ValueError("level_off holds one entry more than level_pos has levels")
    p = WitnessProgram()
    p.gens, p.ngens = gens.ctypes.data, gens.shape[0]
    p.level_off, p.level_pos, p.nlevels = level_off.ctypes.data, level_pos.ctypes.data, level_pos.shape[0]
    p.wslot, p.nrows, p.W = wslot.ctypes.data, wslot.shape[0], wslot.shape[1]
    p.nslots, p.limbs, p.zero_slot, p.num_consts = int(nslots), int(limbs), int(zero_slot), int(num_consts)
    p.in_slots, p.in_vals, p.nin, p.B = in_slots.ctypes.data, in_vals.ctypes.data, in_slots.size, in_vals.shape[0]
    p.form = int(form)
    B = in_vals.shape[0]
    wires = pis = None
    if wslot_cm is not None:
        wslot_cm = np.ascontiguousarray(wslot_cm, dtype=np.uint32)
        if wslot_cm.shape != wslot.shape[::-1]:
            raise ValueError("wslot_cm is [W][nrows]")
        pi_slots = np.ascontiguousarray([] if pi_slots is None else pi_slots, dtype=np.uint32).ravel()
        p.wslot_cm, p.pi_slots, p.npis = wslot_cm.ctypes.data, pi_slots.ctypes.data, pi_slots.size
        if max(B, 0) * wslot.size <= 1 << 28:  # else left to the library's refusal
            wires = np.zeros((B,) + wslot_cm.shape, np.uint64)
            pis = np.zeros((B, pi_slots.size), np.uint64)
    nv = B * int(nslots) if 0 < B <= 64 and 0 < int(nslots) <= 1 << 20 else 1  # a refused shape: never written
    vals = np.zeros(nv, np.uint64)
    err = np.zeros(max(B, 1), np.uint32)
    ctx.check(lib().qp_debug_witness_program(ctx.h, ctypes.byref(p), vals.ctypes.data, err.ctypes.data,
                                             None if wires is None else wires.ctypes.data,
                                             None if pis is None else pis.ctypes.data), "qp_debug_witness_program")
    vals = vals.reshape(B, int(nslots))
    return (vals, err[:B]) if wslot_cm is None else (vals, err[:B], wires, pis)


def hash_no_pad(values):
    """PoseidonHash::hash_no_pad on the host (libqpgpu host code)."""
    a = np.ascontiguousarray(values, dtype=np.uint64)
    out = np.zeros(4, np.uint64)
    rc = lib().qp_hash_no_pad(a, len(a), out)
    if rc:
        raise QpError(rc, "qp_hash_no_pad")
    return [int(x) for x in out]


# ---- routine-level seams (include/qpgpu.h "routine-level seams") ----------

def gate_desc(circuit):
    """qp_circuit_gate_desc for a built Circuit."""
    g = GateDesc()
    rc = lib().qp_circuit_gate_desc(circuit.h, ctypes.byref(g))
    if rc:
        raise QpError(rc, "qp_circuit_gate_desc")
    return g


def _u64(v, n=None):
    a = np.ascontiguousarray([int(x) for x in v] if not isinstance(v, np.ndarray) else v, dtype=np.uint64)
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} values, got {a.size}")
    return a


def quotient(ctx, cs, wires, zs_pp, gd, betas, gammas, alphas, pi_hash):
    """compute_quotient_polys: returns quotient coefficients [nc * qdf][n]."""
    nc, qdf = gd.num_challenges, gd.quotient_degree_factor
    out = np.zeros((nc * qdf, 1 << cs.log_n), np.uint64)
    ctx.check(lib().qp_quotient(ctx.h, cs.h, wires.h, zs_pp.h, ctypes.byref(gd), _u64(betas, nc), _u64(gammas, nc),
                                _u64(alphas, nc), _u64(pi_hash, 4), out), "qp_quotient")
    return out


class FriLayer:
    """One committed FRI reduction layer (fri_committed_trees)."""

    def __init__(self, ctx, coeffs, log_values, shift, arity_bits, cap_height):
        c = np.ascontiguousarray(coeffs, dtype=np.uint64)
        if c.ndim != 2 or c.shape[0] != 2:
            raise ValueError("coeffs must be [2][2^k] (ext c0 row, c1 row)")
        self.ctx, self.log_values, self.arity_bits, self.cap_height = ctx, log_values, arity_bits, cap_height
        self.cap = np.zeros((1 << cap_height, 4), np.uint64)
        h = ctypes.c_void_p()
        ctx.check(lib().qp_fri_layer_commit(ctx.h, c, c.shape[1].bit_length() - 1, log_values, shift, arity_bits,
                                            cap_height, self.cap, ctypes.byref(h)), "qp_fri_layer_commit")
        self.h = h

    def open(self, indices):
        idx = np.ascontiguousarray(indices, dtype=np.uint32)
        depth = self.log_values - self.arity_bits - self.cap_height
        evals = np.zeros((len(idx), 1 << self.arity_bits, 2), np.uint64)
        sibs = np.zeros((len(idx), depth, 4), np.uint64)
        self.ctx.check(lib().qp_fri_layer_open(self.h, idx, len(idx), evals, sibs), "qp_fri_layer_open")
        return evals, sibs

    def free(self):
        if self.h:
            lib().qp_fri_layer_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def fri_fold(ctx, coeffs, arity_bits, beta):
    c = np.ascontiguousarray(coeffs, dtype=np.uint64)
    out = np.zeros((2, c.shape[1] >> arity_bits), np.uint64)
    ctx.check(lib().qp_fri_fold(ctx.h, c, c.shape[1].bit_length() - 1, arity_bits, _u64(beta, 2), out), "qp_fri_fold")
    return out


def pow_grind(ctx, states, pos, pow_bits):
    """fri_proof_of_work for n duplex states [n][12] with pending-input counts pos[n]."""
    st = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 12)
    p = np.ascontiguousarray(pos, dtype=np.uint32)
    out = np.zeros(st.shape[0], np.uint64)
    ctx.check(lib().qp_pow_grind(ctx.h, st, p, st.shape[0], pow_bits, out), "qp_pow_grind")
    return out


def _ext_points(points):
    """extension points as a uint64 array [npts][2]"""
    pts = np.ascontiguousarray(points, dtype=np.uint64)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 1:
        raise ValueError("points must be [npts][2] (ext c0, c1)")
    return pts


def _cols(a, what, n=None):
    """a column-major uint64 matrix [ncols][2^k] (2^k == n when given)"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1 or a.shape[1] & (a.shape[1] - 1):
        raise ValueError(f"{what} must be [columns][2^k]")
    if n is not None and a.shape[1] != n:
        raise ValueError(f"{what} must have {n} rows per column, got {a.shape[1]}")
    return a


class PermutationData:
    """A circuit's sigma columns and k_is on the device (qp_perm), uploaded once."""

    def __init__(self, ctx, sigmas, k_is):
        s = _cols(sigmas, "sigmas")
        k = np.ascontiguousarray(k_is, dtype=np.uint64)
        if k.ndim != 1 or k.size != s.shape[0]:
            raise ValueError(f"k_is must hold one value per sigma column ({s.shape[0]})")
        self.ctx, self.num_routed, self.n = ctx, s.shape[0], s.shape[1]
        self.h = None
        h = ctypes.c_void_p()
        ctx.check(lib().qp_perm_new(ctx.h, s, k, s.shape[0], s.shape[1].bit_length() - 1, ctypes.byref(h)),
                  "qp_perm_new")
        self.h = h

    def partial_products_and_zs(self, wires, qdf, betas, gammas):
        """wires_permutation_partial_products_and_zs: wires [>= num_routed][n] ->
        [nc * nchunks][n], all Zs first, then the partial products per challenge."""
        w = _cols(wires, "wires", self.n)
        if w.shape[0] < self.num_routed:
            raise ValueError(f"wires must hold the {self.num_routed} routed columns")
        b, g = _u64(betas), _u64(gammas)
        if b.ndim != 1 or b.size < 1 or b.size != g.size:
            raise ValueError("betas and gammas must hold one value per challenge")
        qdf = int(qdf)
        if qdf < 1:
            raise ValueError("quotient_degree_factor must be positive")
        nchunks = (self.num_routed + qdf - 1) // qdf
        out = np.zeros((b.size * nchunks, self.n), np.uint64)
        self.ctx.check(lib().qp_partial_products_and_zs(self.h, w, qdf, b, g, b.size, out),
                       "qp_partial_products_and_zs")
        return out

    def free(self):
        if self.h:
            lib().qp_perm_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def opening_set(ctx, cs, wires, zs_pp, quotient, nc, zeta):
    """OpeningSet::new: every polynomial of the four batches at zeta in oracle order,
    then the nc Zs at g*zeta: [(sum of npolys) + nc][2]."""
    z = _u64(zeta, 2)
    out = np.zeros((cs.npolys + wires.npolys + zs_pp.npolys + quotient.npolys + int(nc), 2), np.uint64)
    ctx.check(lib().qp_opening_set(ctx.h, cs.h, wires.h, zs_pp.h, quotient.h, int(nc), z, out), "qp_opening_set")
    return out


def fri_initial_poly(ctx, cs, wires, zs_pp, quotient, nc, alpha, zeta):
    """The polynomial PolynomialBatch::prove_openings hands to FRI: ext coefficients
    [2][n] (c0 row, c1 row), the layout FriLayer takes."""
    a, z = _u64(alpha, 2), _u64(zeta, 2)
    out = np.zeros((2, 1 << cs.log_n), np.uint64)
    ctx.check(lib().qp_fri_initial_poly(ctx.h, cs.h, wires.h, zs_pp.h, quotient.h, int(nc), a, z, out),
              "qp_fri_initial_poly")
    return out
