"""plonky2's prove() composed from the routine-level seams alone (INTEGRATION.md
binding A): tests/seam_prover.py with its three host stand-ins replaced by the
seams that move them to the device,

    PermutationData.partial_products_and_zs   wires_permutation_partial_products_and_zs
    opening_set                               OpeningSet::new
    fri_initial_poly                          PolynomialBatch::prove_openings' initial polynomial

so the oracle supplies only the transcript's Poseidon permutation.  stages="host"
runs the oracle stand-ins instead (the same code path as seam_prover.prove), and
`times` collects the wall time of each of the three stages either way
(tools/seam_stages.py).  Also the plain-integer reference of the permutation
products for shapes no circuit has.

TEST INFRASTRUCTURE, like seam_prover.py."""
import struct
import time

import numpy as np

from oracle_lib import P, hash_no_pad
from seam_prover import GEN, Challenger, _bind, _ext_mul, _root, evals_ext, fri_arities


def k_is(num_routed):
    """plonky2 get_unique_coset_shifts: g^i of the multiplicative generator."""
    return np.array([pow(GEN, i, P) for i in range(num_routed)], np.uint64)


def root_of_unity(log_n):
    return _root(log_n)


def ref_partial_products_and_zs(wires, sigmas, kis, qdf, betas, gammas):
    """wires_permutation_partial_products_and_zs with Python integers: per row the
    quotients (w + beta k_j x + gamma) / (w + beta sigma + gamma), chunk products of
    qdf, Z the running product over rows from 1, partial products Z times the chunk
    prefix products without the last.  Returns ([nc * nchunks][n], no zero denominator)."""
    R, n = len(sigmas), len(sigmas[0])
    nchunks = (R + qdf - 1) // qdf
    nc = len(betas)
    g = _root(n.bit_length() - 1)
    zs = [[0] * n for _ in range(nc)]
    pps = [[[0] * n for _ in range(nchunks - 1)] for _ in range(nc)]
    dens_ok = True
    for c in range(nc):
        beta, gamma = int(betas[c]), int(gammas[c])
        z, x = 1, 1
        for i in range(n):
            zs[c][i] = z
            run = z
            for k in range(nchunks):
                num = den = 1
                for j in range(k * qdf, min((k + 1) * qdf, R)):
                    w = int(wires[j][i])
                    num = num * ((w + beta * int(kis[j]) % P * x + gamma) % P) % P
                    d = (w + beta * int(sigmas[j][i]) + gamma) % P
                    dens_ok = dens_ok and d != 0
                    den = den * d % P
                run = run * num % P * pow(den, P - 2, P) % P
                if k < nchunks - 1:
                    pps[c][k][i] = run
            z = run
            x = x * g % P
    rows = zs + [pp for c in range(nc) for pp in pps[c]]
    return np.array(rows, dtype=np.uint64).reshape(nc * nchunks, n), dens_ok


def prove(ctx, circuit, wires, pis, stages="seam", times=None, gate_desc=None, cap_h=4, rate_bits=3, num_queries=28,
          pow_bits=16):
    """One proof of `circuit` for the witness `wires` [num_wires][n] and public inputs `pis`.
    stages="seam": everything but the transcript through the C ABI; "host": the three
    stages through the oracle's C as in seam_prover.prove.  times: dict of lists, seconds
    per stage ("zs", "openings", "fri_initial") appended."""
    import qp_wormhole as q
    L = _bind()
    assert stages in ("seam", "host")
    seam = stages == "seam"

    def lap(name, t0):
        if times is not None:
            times.setdefault(name, []).append(time.perf_counter() - t0)

    common = circuit.common_data()
    n = circuit.n
    log_n = circuit.degree_bits
    logN = log_n + rate_bits
    N = 1 << logN
    g = gate_desc or q.gate_desc(circuit)
    arity_bits, final_len = fri_arities(log_n, rate_bits, cap_h)
    nc, qdf, R = g.num_challenges, g.quotient_degree_factor, g.num_routed_wires
    cs_vals = circuit.constants_sigmas()
    wires = np.ascontiguousarray(wires, np.uint64)
    # preprocessing (build_prover): constants || sigmas commitment, circuit digest, permutation data
    cs = q.PolynomialBatch.from_values(ctx, cs_vals, rate_bits, cap_h)
    perm = q.PermutationData(ctx, cs_vals[cs_vals.shape[0] - R:], k_is(R)) if seam else None
    empty = np.zeros(4, np.uint64)
    L.ora_hash_pad(np.zeros(1, np.uint64), 0, empty)
    digest = hash_no_pad(np.concatenate([cs.cap.reshape(-1), empty, np.array([log_n], np.uint64)]))
    pih = hash_no_pad(np.asarray(pis, np.uint64))
    t = Challenger()
    t.observe(digest)
    t.observe(pih)
    w = q.PolynomialBatch.from_values(ctx, wires, rate_bits, cap_h)
    t.observe(w.cap)
    betas = [t.get() for _ in range(nc)]
    gammas = [t.get() for _ in range(nc)]
    # partial products and Z
    nchunks = (R + qdf - 1) // qdf
    t0 = time.perf_counter()
    if seam:
        zs_vals = perm.partial_products_and_zs(wires, qdf, betas, gammas)
    else:
        zs_vals = np.zeros((nc * nchunks, n), np.uint64)
        assert L.ora_zs_values(common, len(common), cs_vals, wires, np.array(betas, np.uint64),
                               np.array(gammas, np.uint64), zs_vals) == 0
    lap("zs", t0)
    z = q.PolynomialBatch.from_values(ctx, zs_vals, rate_bits, cap_h)
    t.observe(z.cap)
    alphas = [t.get() for _ in range(nc)]
    qc = q.quotient(ctx, cs, w, z, g, betas, gammas, alphas, pih)
    qb = q.PolynomialBatch.from_coeffs(ctx, qc, rate_bits, cap_h)
    t.observe(qb.cap)
    zeta = t.get_ext()
    # openings
    batches = [cs, w, z, qb]
    zeta_next = _ext_mul(zeta, (_root(log_n), 0))
    t0 = time.perf_counter()
    if seam:
        o = q.opening_set(ctx, cs, w, z, qb, nc, zeta)
        cuts = np.cumsum([0] + [b.npolys for b in batches])
        op = [o[cuts[i]:cuts[i + 1]] for i in range(4)]
        z_next = o[cuts[4]:]
    else:
        op = [evals_ext(b.coeffs, zeta) for b in batches]
        z_next = evals_ext(z.coeffs[:nc], zeta_next)
    lap("openings", t0)
    npp = nc * (nchunks - 1)
    for o_ in (op[0], op[1], op[2][:nc], op[2][nc:nc + npp], op[3], z_next):
        t.observe(o_)
    # FRI: initial polynomial, then one seam call per reduction layer
    alpha = t.get_ext()
    t0 = time.perf_counter()
    if seam:
        coeffs = q.fri_initial_poly(ctx, cs, w, z, qb, nc, alpha, zeta)  # [2][n]: qp_fri_layer_commit's layout
    else:
        fin = np.zeros((n, 2), np.uint64)
        L.ora_fri_initial(cs.coeffs, cs.npolys, w.coeffs, w.npolys, z.coeffs, z.npolys, qb.coeffs, qb.npolys, nc,
                          log_n, np.array(alpha, np.uint64), np.array(zeta, np.uint64),
                          np.array(zeta_next, np.uint64), fin)
        coeffs = np.ascontiguousarray(fin.T)
    lap("fri_initial", t0)
    shift, lg = GEN, logN
    layers, layer_caps = [], []
    for ab in arity_bits:
        layer = q.FriLayer(ctx, coeffs, lg, shift, ab, cap_h)
        layers.append(layer)
        layer_caps.append(layer.cap)
        t.observe(layer.cap)
        beta = t.get_ext()
        coeffs = q.fri_fold(ctx, coeffs, ab, beta)
        shift = pow(shift, 1 << ab, P)
        lg -= ab
    final = coeffs[:, :final_len].T.copy()
    t.observe(final)
    st, pos = t.pending_state()
    pw = int(q.pow_grind(ctx, st[None, :], [pos], pow_bits)[0])
    t.observe([pw])
    t.get()
    queries = []
    for _ in range(num_queries):
        xi = t.get() % N
        init = [b.open([xi]) for b in batches]
        steps = []
        for layer, ab in zip(layers, arity_bits):
            li = xi >> ab
            ev, sib = layer.open([li])
            steps.append((ev[0], sib[0]))
            xi = li
        queries.append((init, steps))
    # ProofWithPublicInputs::to_bytes
    out = bytearray()

    def u64s(a):
        out.extend(np.ascontiguousarray(a, dtype=np.uint64).tobytes())
    for b in (w, z, qb):
        u64s(b.cap)
    for o_ in (op[0], op[1], op[2][:nc], z_next, op[2][nc:nc + npp], op[3]):
        u64s(o_)
    for c in layer_caps:
        u64s(c)
    for init, steps in queries:
        for leaves, sibs in init:
            u64s(leaves[0])
            out.append(sibs.shape[1])
            u64s(sibs[0])
        for ev, sib in steps:
            u64s(ev)
            out.append(sib.shape[0])
            u64s(sib)
    u64s(final)
    out.extend(struct.pack("<QQ", pw, len(pis)))
    u64s(np.asarray(pis, np.uint64))
    for layer in layers:
        layer.free()
    if perm is not None:
        perm.free()
    for b in batches:
        b.free()
    return bytes(out)
