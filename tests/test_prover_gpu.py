"""`Prover::prove_with_preprocessed` end to end on the device (ark_plonk_amd/prover.py: every O(n) step through the C ABI, the
library's merlin transcript, the library's proof serialisation) against the reference VERIFIER restated on integers
(oracle/verifier_oracle.py: proof.rs:110-611 with the pairing replaced by the same equation on discrete logarithms, which the test
can do because it knows tau).

The circuit is a real satisfied one: arithmetic gates with every selector in play, public inputs, copy constraints that move
values between wires and rows (so z is not constant), lookup gates into a padded four-column table and -- from 128 rows up -- runs of
every other gate the reference has: range (base-4 accumulator chains, widget/range.rs), logic (AND and XOR quads, widget/logic.rs),
curve addition and fixed-base scalar multiplication steps over a twisted Edwards curve with random coefficients (widget/ecc/*.rs).
At 32 rows those four selectors are all-zero (their commitments are the point at infinity).  A witness with ONE wrong cell must fail."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ark_plonk_amd as zk  # noqa: E402
from ark_plonk_amd import linearisation, prover, transcript  # noqa: E402
from ark_plonk_amd.curves import fr_from_mont, fr_to_mont  # noqa: E402
from oracle import bigint_oracle as bo  # noqa: E402
from oracle import verifier_oracle as vo  # noqa: E402
from oracle import wire_oracle as wo  # noqa: E402
from tests.conftest import TAU, assert_is_scalar_times_g, srs_from_powers, tau_powers  # noqa: E402

pytestmark = pytest.mark.gpu
K = (1, 7, 13, 17)


def dev(cid, ints):
    import torch
    return torch.from_numpy(np.ascontiguousarray(fr_to_mont(cid, ints)).view(np.int64).reshape(-1, 4)).cuda()


def add_gadgets(cv, base, sel, a, b, c, d, rnd, ca, cd):
    """Runs of range / logic / curve-addition / fixed-base rows starting at row `base`, each followed by an ordinary arithmetic row
    that absorbs the run's "next row" values in its a, b, d wires (its c is computed later).  Returns the rows that are NOT free
    arithmetic rows (the gadget rows) and the terminal rows."""
    p = cv.r
    inv = lambda x: pow(x % p, -1, p)  # noqa: E731
    quads = [int(v % 4) for v in rnd(64, 90)]
    gadget, terminal = [], []
    r = base
    # -- range (widget/range.rs:47-63): c - 4d, b - 4c, a - 4b, d_next - 4a in {0,1,2,3}
    acc = rnd(1, 91)[0]
    for k in range(6):
        d[r] = acc
        c[r] = (4 * d[r] + quads[4 * k]) % p
        b[r] = (4 * c[r] + quads[4 * k + 1]) % p
        a[r] = (4 * b[r] + quads[4 * k + 2]) % p
        acc = (4 * a[r] + quads[4 * k + 3]) % p
        sel["q_range"][r] = 1
        gadget.append(r)
        r += 1
    d[r] = acc
    terminal.append(r)
    r += 1
    # -- logic (widget/logic.rs:65-133): q_c = 1 is AND, q_c = -1 is XOR on base-4 digits; c holds the product of the two digits
    xa, xb, xd = rnd(3, 92)
    for k in range(6):
        qa, qb = quads[24 + 2 * k], quads[25 + 2 * k]
        is_and = k % 2 == 0
        a[r], b[r], d[r] = xa, xb, xd
        c[r] = qa * qb
        xa, xb = (4 * xa + qa) % p, (4 * xb + qb) % p
        xd = (4 * xd + ((qa & qb) if is_and else (qa ^ qb))) % p
        sel["q_logic"][r] = 1
        sel["q_c"][r] = 1 if is_and else p - 1
        gadget.append(r)
        r += 1
    a[r], b[r], d[r] = xa, xb, xd
    terminal.append(r)
    r += 1
    # -- curve addition (widget/ecc/curve_addition.rs:62-97): (x1, y1) + (x2, y2) by the twisted Edwards formulas with coefficients ca, cd;
    #    the row after it holds the sum in a, b and x1 * y2 in d
    for k in range(4):
        x1, y1, x2, y2 = rnd(4, 94 + k)
        a[r], b[r], c[r], d[r] = x1, y1, x2, y2
        x1y2, y1x2 = x1 * y2 % p, y1 * x2 % p
        x3 = (x1y2 + y1x2) * inv(1 + cd * x1y2 % p * y1x2) % p
        y3 = (y1 * y2 - ca * x1 * x2) * inv(1 - cd * x1y2 % p * y1x2) % p
        sel["q_variable_group_add"][r] = 1
        gadget.append(r)
        r += 1
        a[r], b[r], d[r] = x3, y3, x1y2
        terminal.append(r)
        r += 1
    # -- fixed-base scalar multiplication step (widget/ecc/fixed_base_scalar_mul.rs:88-156): bit = d_next - 2d in {-1, 0, 1}
    ax, ay, ad = rnd(3, 110)
    for k, bit in enumerate((1, 0, p - 1, 1, p - 1)):
        xb, yb, xyb = rnd(3, 111 + k)
        sel["q_l"][r], sel["q_r"][r], sel["q_c"][r] = xb, yb, xyb
        sel["q_fixed_group_add"][r] = 1
        a[r], b[r], d[r] = ax, ay, ad
        c[r] = bit * xyb % p                                       # xy_alpha
        x_alpha, y_alpha = xb * bit % p, (bit * bit * (yb - 1) + 1) % p
        t = cd * c[r] % p * ax % p * ay % p
        ax, ay = (x_alpha * ay + y_alpha * ax) * inv(1 + t) % p, (y_alpha * ay - ca * x_alpha * ax) * inv(1 - t) % p
        ad = (2 * ad + bit) % p
        gadget.append(r)
        r += 1
    a[r], b[r], d[r] = ax, ay, ad
    terminal.append(r)
    r += 1
    return gadget, terminal, r


def build_circuit(cv, log_n, seed, break_cell=False, coeffs=(0, 0)):
    """Selector / sigma / table / wire columns of a satisfied circuit as integer lists, and its public inputs."""
    p, n = cv.r, 1 << log_n
    rng = np.random.default_rng(seed)
    rnd = lambda k, s: bo.seeded_scalars(cv, seed * 1000 + s, k)  # noqa: E731
    used = n - 5                                                     # a few all-zero padding rows at the end
    sel = {name: [0] * n for name in prover.SELECTORS}
    a, b, c, d = ([0] * n for _ in range(4))
    gadget_rows, terminal_rows = set(), set()
    g_base = used - 48
    # the table: n/4 distinct rows, padded with its first row
    rows = max(n // 4, 2)
    tcols = [rnd(rows, 10 + k) for k in range(4)]
    table = [[col[i] if i < rows else col[0] for i in range(n)] for col in tcols]
    ra, rb, rd = rnd(n, 1), rnd(n, 2), rnd(n, 3)
    qs = {name: rnd(n, 20 + k) for k, name in enumerate(("q_m", "q_l", "q_r", "q_4", "q_c"))}
    reserved = set(range(g_base, used)) if n >= 128 else set()       # rows of the gadget runs: neither lookups nor random arithmetic
    is_lookup = [bool(rng.integers(0, 3) == 0) and 0 < i < used and i not in reserved for i in range(n)]
    pub = {1: rnd(1, 40)[0], 3: rnd(1, 41)[0]}
    for i in range(used):
        if is_lookup[i]:
            j = int(rng.integers(0, rows))
            a[i], b[i], c[i], d[i] = (tcols[k][j] for k in range(4))
            sel["q_lookup"][i] = 1
        else:
            a[i], b[i], d[i] = ra[i], rb[i], rd[i]
    # copy constraints before the outputs are computed: cell (wire, row) pairs that must hold one value
    sigma = [[K[k] * pow(cv.root_of_unity(log_n), i, p) % p for i in range(n)] for k in range(4)]
    free = [i for i in range(5, used) if not is_lookup[i]]
    for t in range(0, min(len(free) - 1, 12), 2):
        i, j = free[t], free[t + 1]
        (w1, r1), (w2, r2) = ((0, i), (1, j)) if t % 4 == 0 else ((3, i), (0, j))      # a_i = b_j, then d_i = a_j
        cols = (a, b, c, d)
        cols[w2][r2] = cols[w1][r1]
        sigma[w1][r1], sigma[w2][r2] = sigma[w2][r2], sigma[w1][r1]                    # a 2-cycle
    if n >= 128:
        g, t, end = add_gadgets(cv, g_base, sel, a, b, c, d, rnd, coeffs[0], coeffs[1])
        assert end <= used
        gadget_rows, terminal_rows = set(g), set(t)
    for i in range(used):
        if i in gadget_rows:
            continue
        if not is_lookup[i]:
            for name in qs:
                sel[name][i] = qs[name][i]
            sel["q_o"][i] = p - 1
            sel["q_arith"][i] = 1
            c[i] = (sel["q_m"][i] * a[i] * b[i] + sel["q_l"][i] * a[i] + sel["q_r"][i] * b[i] + sel["q_4"][i] * d[i] + sel["q_c"][i]
                    + pub.get(i, 0)) % p
    pub = {i: v for i, v in pub.items() if not is_lookup[i]}
    if break_cell:
        c[free[3]] = (c[free[3]] + 1) % p
    return sel, sigma, table, [a, b, c, d], pub


def run_case(cid, log_n, ctx, oracle_cpu, break_cell=False):
    cv = bo.CURVES[cid]
    n = 1 << log_n
    ca, cd = bo.seeded_scalars(cv, 0x51, 2)                                  # the embedded curve's coefficients: any two field elements
    sel, sigma, table, wires, pub = build_circuit(cv, log_n, 7 + log_n + cid, break_cell, (ca, cd))
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    dom4 = zk.Radix2EvaluationDomain.new(4 * n, cid, ctx)
    pk = prover.ProverKey(dom, dom4, {k: dev(cid, v) for k, v in sel.items()}, [dev(cid, s) for s in sigma], [dev(cid, t) for t in table])
    pw_canon, _ = tau_powers(oracle_cpu, cid, n + 8)
    ck = zk.CommitterKey(srs_from_powers(ctx, cid, pw_canon), cid, ctx)
    vk = pk.verifier_key(ck)                                                 # preprocess.rs:351-374: the 20 commitments of the key
    pre = transcript.seed_transcript(transcript.Transcript(b"end to end", cid), vk, n)      # widget/mod.rs:252-278
    proof = prover.prove(pk, ck, [dev(cid, w) for w in wires], {i: fr_to_mont(cid, [v])[0] for i, v in pub.items()}, pre,
                         fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0])
    proof.vk = vk
    return cv, pk, ck, proof, pub, (ca, cd), wires


def oracle_points(cid, vk):
    """The verifier key's commitments as the oracle's affine integer points, under the oracle's names."""
    from ark_plonk_amd.curves import fq_from_mont
    names = dict(KEY, sigma0="left_sigma", sigma1="right_sigma", sigma2="out_sigma", sigma3="fourth_sigma",
                 table_1="table_1", table_2="table_2", table_3="table_3", table_4="table_4")
    out = {}
    for k, v in names.items():
        pt = vk[v]
        out[k] = None if pt.infinity else (fq_from_mont(cid, pt.x.reshape(1, -1))[0], fq_from_mont(cid, pt.y.reshape(1, -1))[0])
    return out


KEY = {"q_m": "q_m", "q_l": "q_l", "q_r": "q_r", "q_o": "q_o", "q_4": "q_4", "q_c": "q_c", "q_arith": "q_arith", "q_range": "q_range",
       "q_logic": "q_logic", "q_fixed": "q_fixed_group_add", "q_var": "q_variable_group_add", "q_lookup": "q_lookup"}


def dlogs(cid, ctx, pk, proof):
    """polynomial(tau) for every commitment of the verifier key and of the proof, from the device-resident polynomials
    (zk_poly_evaluate_dev).  The opening witnesses are canonical scalars: read as Montgomery values they are off by the factor R."""
    cv = bo.CURVES[cid]
    polys = {k: pk.polys[v] for k, v in KEY.items()}
    polys.update({f"sigma{k}": pk.sigma_polys[k] for k in range(4)})
    polys.update({f"table_{k + 1}": pk.domain.ifft(pk.table_cols[k]) for k in range(4)})
    polys.update(proof.polys)
    names = list(polys)
    tau_m = fr_to_mont(cid, [TAU])
    vals = fr_from_mont(cid, linearisation.evaluate_batch([polys[k] for k in names], np.repeat(tau_m, len(names), axis=0), cid, ctx))
    d = dict(zip(names, vals))
    for k in ("aw", "saw"):
        d[f"{k}_opening"] = d.pop(f"{k}_witness") * (1 << 256) % cv.r
    return d


@pytest.mark.parametrize("cid,log_n", [(0, 5), (0, 10), (0, 14), (1, 7)])
def test_device_prover_satisfies_the_reference_verifier(cid, log_n, ctx, oracle_cpu):
    import torch
    cv, pk, ck, proof, pub, (ca, cd), wires = run_case(cid, log_n, ctx, oracle_cpu)
    n = 1 << log_n
    data = proof.to_bytes()
    # -- the logarithm of every commitment: its polynomial at tau, bound to the proof's points by scalar multiplication
    ch = proof.challenges
    dlog = dlogs(cid, ctx, pk, proof)
    for k in vo.COMMITMENTS:
        assert_is_scalar_times_g(proof.commitments[k], dlog[k], cid)
    assert_is_scalar_times_g(proof.aw_opening, dlog["aw_opening"], cid)
    assert_is_scalar_times_g(proof.saw_opening, dlog["saw_opening"], cid)
    # -- the verifier
    vk_pts = oracle_points(cid, proof.vk)
    for k, pt in vk_pts.items():                       # the key's commitments are its polynomials at tau times G
        assert pt == bo.ec_mul(cv, dlog[k], (cv.gx, cv.gy)), k
    t = vo.seed_transcript(cv, wo.PlonkTranscript(b"end to end", cv), vk_pts, n)
    ok, vch, det = vo.verify_with_trapdoor(cv, log_n, data, t, pub, dlog, TAU, ca, cd)
    assert ok, det
    # the library's transcript and the independent one agree on every challenge
    mine = {k: fr_from_mont(cid, np.asarray(v).reshape(1, 4))[0] for k, v in ch.items()}
    for a, b in (("zeta", "zeta"), ("beta", "beta"), ("gamma", "gamma"), ("delta", "delta"), ("epsilon", "epsilon"), ("alpha", "alpha"),
                 ("range", "range_challenge"), ("logic", "logic_challenge"), ("fixed", "fixed_base_challenge"), ("var", "var_base_challenge"),
                 ("lookup", "lookup_challenge"), ("z", "z_challenge"), ("aw", "aw_challenge"), ("saw", "saw_challenge")):
        assert vch[a] == mine[b], a
    # the bytes are the reference layout: the independent serialiser rebuilds them from the parsed proof
    pr = det["proof"]
    assert wo.proof_bytes(cv, [pr["commitments"][k] for k in vo.COMMITMENTS], [pr["aw_opening"], pr["saw_opening"]],
                          [pr["evals"][k] for k in vo.EVALS], pr["custom"]) == data
    # all-zero selectors commit to the point at infinity and z is not the constant 1
    assert pr["commitments"]["z_comm"] != (cv.gx, cv.gy)
    if n < 128:                                       # no gadget runs: the four selectors are zero polynomials
        assert torch.count_nonzero(pk.polys["q_range"]).item() == 0 and pr["commitments"]["z_comm"] is not None
    else:                                             # every widget contributes to this proof
        for name in ("q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add", "q_lookup", "q_arith"):
            assert torch.count_nonzero(pk.polys[name]).item() > 0, name


def test_wrong_witness_does_not_verify(ctx, oracle_cpu):
    """One output cell off by one: the prover still runs (the quotient is no longer a polynomial of degree < 4n, its coset iFFT is
    just some vector) and the aggregate opening at z fails the verifier's equation."""
    cid, log_n = 0, 6
    cv, pk, ck, proof, pub, (ca, cd), wires = run_case(cid, log_n, ctx, oracle_cpu, break_cell=True)
    dlog = dlogs(cid, ctx, pk, proof)
    t = vo.seed_transcript(cv, wo.PlonkTranscript(b"end to end", cv), oracle_points(cid, proof.vk), 1 << log_n)
    ok, _, det = vo.verify_with_trapdoor(cv, log_n, proof.to_bytes(), t, pub, dlog, TAU, ca, cd)
    assert not ok and not det["aw"]


def test_full_size_proof_verifies(ctx, oracle_cpu):
    """n = 2^20 (BASELINE config 2): a satisfied circuit built on the device (prover.example_circuit), proved on the device, its
    proof bytes checked by the restated verifier.  Prints the prover's wall time (all five rounds, every O(n) step on the device)."""
    import time
    import torch
    cid, log_n = 0, 20
    n = 1 << log_n
    cv = bo.CURVES[cid]
    ca, cd = bo.seeded_scalars(cv, 0x51, 2)
    pk, wires, pub_m = prover.example_circuit(log_n, cid, ctx, coeffs=(ca, cd))
    pub = {i: fr_from_mont(cid, v.reshape(1, 4))[0] for i, v in pub_m.items()}
    for name in ("q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add", "q_lookup", "q_arith"):
        assert torch.count_nonzero(pk.polys[name]).item() > 0, name          # every widget is in this circuit
    pw_canon, _ = tau_powers(oracle_cpu, cid, n)
    ck = zk.CommitterKey(srs_from_powers(ctx, cid, pw_canon), cid, ctx)
    ck.precompute()
    vk = pk.verifier_key(ck)
    pre = transcript.seed_transcript(transcript.Transcript(b"end to end", cid), vk, n)
    args = (pk, ck, wires, pub_m, pre, fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0])
    prover.prove(*args)                                           # warm-up (twiddle tables, buffers)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    proof = prover.prove(*args)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    data = proof.to_bytes()
    print(f"\nfull proof at n = 2^{log_n}: {dt * 1e3:.1f} ms, {len(data)} bytes")
    dlog = dlogs(cid, ctx, pk, proof)
    for k in ("a_comm", "z_comm", "z_2_comm", "t_3_comm"):
        assert_is_scalar_times_g(proof.commitments[k], dlog[k], cid)
    assert_is_scalar_times_g(proof.aw_opening, dlog["aw_opening"], cid)
    t = vo.seed_transcript(cv, wo.PlonkTranscript(b"end to end", cv), oracle_points(cid, vk), n)
    ok, _, det = vo.verify_with_trapdoor(cv, log_n, data, t, pub, dlog, TAU, ca, cd)
    assert ok, (det["aw"], det["saw"])
    assert prover.check_identity(pk, proof, pub_m)              # the product-side self check agrees
    t0 = time.perf_counter()
    lean = prover.prove(*args, lean=True)                       # 15 MSMs instead of 29: the same bytes
    torch.cuda.synchronize()
    print(f"lean: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    assert lean.to_bytes() == data
    assert dt < 1.0


@pytest.mark.parametrize("cid,log_n", [(0, 5), (0, 7), (1, 7)])
def test_proof_bytes_equal_the_cpu_restatement(cid, log_n, ctx, oracle_cpu):
    """Bit-exact end to end: the device-resident prover and oracle/prover_oracle.py -- `Prover::prove_with_preprocessed` restated
    on integers from the oracle's own pieces (its transforms, grand products, quotient, linearisation, multisets, merlin,
    serialiser; the C++ restatement's Pippenger for the commitments) -- produce the SAME proof bytes for the same circuit,
    including every gate type at 128 rows.  Challenges are compared too, so a difference would be located by round."""
    assert_proof_bytes_equal_the_cpu_restatement(cid, log_n, ctx, oracle_cpu)


def assert_proof_bytes_equal_the_cpu_restatement(cid, log_n, ctx, oracle_cpu):
    """The comparison of the test above, for callers that run it under another setting of the ctx (tests/test_ntt_pass_shapes_gpu.py)."""
    from oracle import prover_oracle as po
    cv, pk, ck, proof, pub, (ca, cd), wires = run_case(cid, log_n, ctx, oracle_cpu)
    n = 1 << log_n
    sel, sigma, table, wires2, pub2 = build_circuit(cv, log_n, 7 + log_n + cid, False, (ca, cd))
    assert wires2 == wires and pub2 == pub
    pw_canon, _ = tau_powers(oracle_cpu, cid, n + 8)
    srs = srs_from_powers(ctx, cid, pw_canon).cpu().numpy().view(np.uint64)
    t = vo.seed_transcript(cv, wo.PlonkTranscript(b"end to end", cv), oracle_points(cid, proof.vk), n)
    osel = {k: sel[v] for k, v in KEY.items()}
    data, och, _ = po.prove(cv, log_n, osel, sigma, table, wires, pub, t, po.cpp_committer(oracle_cpu, cid, cv, srs), ca, cd)
    mine = {k: fr_from_mont(cid, np.asarray(v).reshape(1, 4))[0] for k, v in proof.challenges.items()}
    for a, b in (("zeta", "zeta"), ("beta", "beta"), ("epsilon", "epsilon"), ("alpha", "alpha"), ("lookup", "lookup_challenge"),
                 ("z", "z_challenge"), ("aw", "aw_challenge"), ("saw", "saw_challenge")):
        assert och[a] == mine[b], a
    assert proof.to_bytes() == data
