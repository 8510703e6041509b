"""The native verifier's host path (device=None, no GPU) at the FRI shapes
new_from_bytes accepts beyond the fixtures' ConstantArityBits(4, 5) at cap height
4 with 28 queries: arities 2..64 in any mix, 0..8 layers, cap heights 0..4 of a
2^11 tree, 1..64 query rounds (fri_shapes.SHAPES).  The oracle proves the voting
circuit under each shape and is the checker on every tampered variant; a
plain-integer model of the fold checks the oracle's own proofs, since away from
arity 16 its prover and verifier otherwise vouch only for each other; the
shapes check_supported refuses are refused with their reason."""
import struct

import numpy as np
import pytest

import fri_shapes as fs
import verifier_cases as vc
from oracle_lib import P, lib as olib
from test_verifier import _new, host_verifier

SHAPES = pytest.mark.parametrize("shape", fs.SHAPES, ids=fs.shape_id)


def test_patch_common_roundtrip():
    cb = fs.voting_common()
    d = vc.parse_common(cb)
    assert (d["degree_bits"], d["rate_bits"], d["cap_h"], d["nq"], d["arity"]) == (8, 3, 4, 28, [4])
    assert fs.patch_common(cb, d["arity"]) == cb
    assert fs.patch_common(fs.patch_common(cb, [1] * 8, 0, 63, 8), [4], 4, 28, struct.unpack_from("<I", cb, 74)[0]) == cb
    assert len(fs.patch_common(cb, [])) == len(cb) - 8


def test_fixture_tamper_cases_unchanged():
    """tamper_set on the three reference proofs: the labels in their order (test_batch_semantics
    picks cases by position), no duplicate, and each variant differing from the proof."""
    for name, (vo, cb, cases) in vc.reference_cases().items():
        labels = [lab for lab, _, _ in cases]
        nl = len(vc.Layout(cb).layers)
        want = ["intact", "wires cap", "constants opening", "wires opening", "quotient opening", "public input",
                "pow witness"]
        want += [f"q{q} tree{o} {what}" for q in (0, 14, 27) for o in range(4) for what in ("leaf", "sibling")]
        want += [f"layer{l} {what}" for l in range(nl) for what in ("queried element", "other element", "sibling")]
        want += ["final poly", "truncated", "extra byte", "sibling count", "element = p"]
        assert labels == want, name
        assert len({pf for _, pf, _ in cases}) == len(cases)


@SHAPES
def test_host_verdicts_equal_the_oracles(shape):
    """Every case of verifier_cases.tamper_set on the oracle's proof under `shape`: the host
    path's status equals the oracle's code (fri/verifier.rs verify_fri_proof,
    fri_verifier_query_round, fri_verify_initial_proof, compute_evaluation;
    hash/merkle_proofs.rs verify_merkle_proof_to_cap), and the codes cover every stage a byte
    tamper can reach (fri_shapes.status_floor).  Code 8 (final polynomial) is out of reach: the
    final polynomial is observed before PoW and the query indices, so a changed coefficient
    fails PoW first."""
    vo, cb, pf = fs.oracle_case(shape)
    cases = fs.tamper_cases(shape)
    assert cases[0][0] == "intact" and cases[0][2] == 0
    assert len({p for _, p, _ in cases}) == len(cases)
    v = host_verifier(vo, cb, max_batch=64)
    got = v.verify_batch([p for _, p, _ in cases])
    v.verify(pf)
    v.close()
    bad = [(lab, st, rc) for (lab, _, rc), st in zip(cases, got) if st != vc.expect(rc)]
    assert not bad, bad
    assert fs.status_floor(shape) <= set(got), sorted(set(got))


@pytest.mark.parametrize("shape", [fs.SHAPES[10], fs.SHAPES[11], fs.SHAPES[9]], ids=fs.shape_id)
def test_host_odd_lane_chunks(shape):
    """max_batch = 3 over 7 proofs (chunks of 3, 3, 1) at odd nq: every chunk has an odd lane
    count, so each class's u32 index array ends in a padded word (make_layout).  Statuses equal
    each proof verified alone; see fri_shapes.chunk_pick for the pattern."""
    assert shape[2] % 2 == 1
    vo, cb, _ = fs.oracle_case(shape)
    proofs, valid = fs.chunk_pick(shape)
    assert [p == proofs[0] for p in proofs] == valid
    one = host_verifier(vo, cb, max_batch=1)
    alone = [one.verify_batch([p])[0] for p in proofs]
    one.close()
    assert [st == 0 for st in alone] == valid
    v = host_verifier(vo, cb, max_batch=3)
    assert v.verify_batch(proofs) == alone
    v.close()


# ---- a plain-integer model of the fold, over F_p[X] / (X^2 - 7)

def x_mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def x_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def rev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


GEN = 14293326489335486720  # Goldilocks MULTIPLICATIVE_GROUP_GENERATOR, the coset shift of the LDE
TWO_ADIC_GEN = 7277203076849721926  # Goldilocks POWER_OF_TWO_GENERATOR, of order 2^32


def omega(bits):
    """The primitive 2^bits-th root of unity, as Field::primitive_root_of_unity squares it down."""
    return pow(TWO_ADIC_GEN, 1 << (32 - bits), P)


def lagrange_at(xs, ys, beta):
    """The polynomial through (xs[i], ys[i]), xs in the base field, at the extension point beta."""
    acc = (0, 0)
    for i, (xi, yi) in enumerate(zip(xs, ys)):
        num, den = yi, 1
        for j, xj in enumerate(xs):
            if j != i:
                num = x_mul(num, ((beta[0] - xj) % P, beta[1]))
                den = den * (xi - xj) % P
        inv = pow(den, P - 2, P)
        acc = x_add(acc, (num[0] * inv % P, num[1] * inv % P))
    return acc


def test_model_field_constants():
    assert pow(TWO_ADIC_GEN, 1 << 31, P) == P - 1
    assert P - 1 == (1 << 32) * 3 * 5 * 17 * 257 * 65537
    assert all(pow(GEN, (P - 1) // f, P) != 1 for f in (2, 3, 5, 17, 257, 65537))
    assert olib().ora_root_of_unity(11) == omega(11) and pow(omega(6), 32, P) == P - 1
    assert x_mul((0, 1), (0, 1)) == (7, 0)
    assert [rev(i, 3) for i in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7] and rev(1, 1) == 1 and rev(0, 0) == 0


@pytest.mark.parametrize("shape", [s for s in fs.SHAPES if s[0]], ids=fs.shape_id)
def test_fold_model(shape):
    """The oracle's valid proof against Python integers, independent of both C implementations
    (fri/verifier.rs fri_verifier_query_round and compute_evaluation, fri/reduction_strategies.rs
    for the arity list): for every query and layer the 2^ab opened values, Lagrange-interpolated
    at beta_l over the points s w_ab^rev_ab(j), give the next layer's opened element at that
    layer's position, and after the last layer the final polynomial at the folded point.

    The point of opened value j is read off the layer's domain directly, position
    (coset << ab | j) of the bit-reversed coset g^(2^folded) <w_lg>; s, the first of them, must
    equal what compute_evaluation derives from the queried point x = g w_N^rev(x_index):
    x^(2^folded) w_ab^(arity - rev_ab(x_index_within_coset)).  beta_l and the query indices are
    ora_challenges'; the cosets and the final polynomial are the proof's bytes at
    verifier_cases.Layout's offsets.  The initial combine is out of this model's scope, so a
    shape without layers has nothing to assert here."""
    arity, cap_h, nq = shape
    vo, cb, pf = fs.oracle_case(shape)
    lay = vc.Layout(cb)
    assert [a for a, _ in lay.layers] == list(arity) and lay.log_N == 11 and lay.d["nq"] == nq
    ch = np.zeros(256, np.uint64)
    n = olib().ora_challenges(vo + cb, len(vo + cb), pf, len(pf), ch)
    nc = lay.d["nc"]
    assert n == 3 * nc + 4 + 2 * len(arity) + 1 + nq
    betas = [(int(ch[3 * nc + 4 + 2 * l]), int(ch[3 * nc + 5 + 2 * l])) for l in range(len(arity))]
    qidx = [int(x) for x in ch[n - nq:n]]
    assert all(x < 1 << lay.log_N for x in qidx)
    ext_at = lambda off, k: struct.unpack_from("<QQ", pf, off + 16 * k)  # noqa: E731
    final = [ext_at(lay.final_poly, k) for k in range(lay.final_len)]
    assert lay.final_len == 1 << (8 - sum(arity))
    for q, x_index in enumerate(qidx):
        x = GEN * pow(omega(lay.log_N), rev(x_index, lay.log_N), P) % P
        lg, folded, carried = lay.log_N, 0, None
        for l, ab in enumerate(arity):
            ev = [ext_at(lay.layer(q, l)[0], j) for j in range(1 << ab)]
            index = x_index >> folded
            coset, within = index >> ab, index & ((1 << ab) - 1)
            if carried is not None:
                assert ev[within] == carried, (q, l)
            shift = pow(GEN, 1 << folded, P)
            pts = [shift * pow(omega(lg), rev(coset << ab | j, lg), P) % P for j in range(1 << ab)]
            s = pts[0]
            assert s == pow(x, 1 << folded, P) * pow(omega(ab), (1 << ab) - rev(within, ab), P) % P
            assert pts == [s * pow(omega(ab), rev(j, ab), P) % P for j in range(1 << ab)]
            carried = lagrange_at(pts, ev, betas[l])
            lg -= ab
            folded += ab
        at = pow(GEN, 1 << folded, P) * pow(omega(lg), rev(x_index >> folded, lg), P) % P
        fx = (0, 0)
        for c in reversed(final):
            fx = x_add((fx[0] * at % P, fx[1] * at % P), c)
        assert fx == carried, q


# ---- the shapes check_supported refuses

REFUSED = [
    (([0], 4, 28), "unsupported FRI reduction"),
    (([7], 4, 28), "unsupported FRI reduction"),
    (([4, 4], 4, 28), "unsupported FRI reduction"),     # the last layer's tree is below the cap
    (([4, 4, 1], 0, 28), "unsupported FRI reduction"),  # the reduction runs past the degree
    (([1] * 9, 0, 28), "too many FRI layers"),
    (([4], 4, 0), "unsupported query round count"),
    (([4], 4, 65), "unsupported query round count"),
    (([4], 12, 28), "cap height exceeds the tree"),
    (([4], 17, 28), "cap height exceeds the tree"),
]


@pytest.mark.parametrize("shape,reason", REFUSED, ids=[fs.shape_id(s) for s, _ in REFUSED])
def test_refused_shapes(shape, reason):
    """rc 6 (QP_ERR_FORMAT) with check_supported's reason, and a handle that verifies nothing
    (_new asserts it)."""
    arity, cap_h, nq = shape
    cb = fs.patch_common(fs.voting_common(), arity, cap_h, nq, fs.POW_BITS)
    vo = struct.pack("<Q", cap_h) + bytes(32 << cap_h) + bytes(32)
    rc, msg = _new(vo, cb)
    assert rc == 6 and msg == "common circuit data: " + reason, (rc, msg)


def test_refusal_boundaries_are_accepted():
    """The accepted side of each refusal: 8 layers at cap height 3 with one query, arity 64,
    64 queries, a last layer whose tree is exactly the cap, and a cap as high as the tree."""
    for arity, cap_h, nq in (([1] * 8, 3, 1), ([6], 4, 64), ([4, 3], 4, 28), ([], 11, 28)):
        cb = fs.patch_common(fs.voting_common(), arity, cap_h, nq, fs.POW_BITS)
        vo = struct.pack("<Q", cap_h) + bytes(32 << cap_h) + bytes(32)
        assert _new(vo, cb) == (0, ""), (arity, cap_h, nq)
