"""The batch verifier on the device (ark_plonk_amd/verifier.py, csrc/verify.hip) against the integer restatement of the reference
verifier (oracle/verifier_oracle.py), stage by stage: the point decode against `wire_oracle.de_g1`, the per-proof scalar rows against
the oracle's (commitment, value) lists expanded over the bases with Python integers, the fold against the definition computed with the
big-int group law, and -- the synthetic SRS has a known tau -- the pairing equation as tau L == R.  Every comparison is exact."""
import os
import sys
from collections import defaultdict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ark_plonk_amd as zk  # noqa: E402
from ark_plonk_amd import prover, transcript, verifier  # noqa: E402
from ark_plonk_amd.curves import fq_from_mont, fq_to_mont, fr_to_mont, limbs_to_ints  # noqa: E402
from oracle import bigint_oracle as bo  # noqa: E402
from oracle import verifier_oracle as vo  # noqa: E402
from oracle import wire_oracle as wo  # noqa: E402
from tests.conftest import TAU, srs_from_powers, tau_powers  # noqa: E402
from tests.test_prover_gpu import build_circuit, dev, dlogs, oracle_points, run_case  # noqa: E402

pytestmark = pytest.mark.gpu
LABEL = b"end to end"                                       # the label run_case seeds its transcript under
ORACLE_KEY = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_range", "q_logic", "q_fixed", "q_var", "q_lookup", "sigma0", "sigma1", "sigma2",
              "sigma3", "table_1", "table_2", "table_3", "table_4")
PROOF_NAMES = vo.COMMITMENTS + ("aw_opening", "saw_opening")
ERROR_CLASS = {"invalid flags": verifier.G1_BAD_FLAGS, "x not reduced": verifier.G1_X_NOT_REDUCED, "not on curve": verifier.G1_NOT_ON_CURVE,
               "not in the subgroup": verifier.G1_NOT_IN_SUBGROUP}


# ------------------------------------------------------------------------------------------------------------------ stage 1
def encodings(cv):
    """67 encodings: the edge cases first, valid multiples of G after them"""
    g = wo.fq_flag_bytes(cv)
    G = (cv.gx, cv.gy)

    def enc(x, flags=0):
        b = bytearray(x.to_bytes(g, "little"))
        b[-1] |= flags
        return bytes(b)

    out = [wo.ser_g1(cv, G)]
    for k in (2, 3, 5):
        P = bo.ec_mul(cv, k, G)
        e = bytearray(wo.ser_g1(cv, P))
        out.append(bytes(e))
        e[-1] ^= 0x80                                       # the other root: -P, as valid as P
        out.append(bytes(e))
    out += [wo.ser_g1(cv, None), enc(5, 0x40), enc(cv.q - 1, 0x40), enc(cv.q, 0x40), enc(1, 0xC0), enc(0, 0xC0), enc(cv.q), enc(cv.q - 1),
            enc(cv.q - 1, 0x80), enc((1 << (8 * g - 2)) - 1)]
    xs = (1, 2, 0, 4, 5) if cv.q.bit_length() > 300 else (0, 4, 1)
    for x in xs:
        out += [enc(x), enc(x, 0x80)]
    k = 7
    while len(out) < 67:
        out.append(wo.ser_g1(cv, bo.ec_mul(cv, k * 0x9E3779B97F4A7C15 % cv.r, G)))
        k += 1
    return out


def oracle_decode(cv, e):
    try:
        return 0, wo.de_g1(cv, e)
    except ValueError as err:
        return ERROR_CLASS[str(err)], None


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("n", [1, 67])
def test_decode_matches_the_oracle(cid, n, ctx):
    import torch
    cv = bo.CURVES[cid]
    L = zk.get_curve(cid).fq_limbs
    encs = encodings(cv)[:n]
    assert len(encs) == n
    pts, inf, st = verifier.decompress_batch(np.frombuffer(b"".join(encs), dtype=np.uint8), cid, ctx)
    torch.cuda.synchronize()
    pts, inf, st = pts.cpu().numpy().view(np.uint64), inf.cpu().numpy(), st.cpu().numpy()
    want = [oracle_decode(cv, e) for e in encs]
    assert st.tolist() == [w[0] for w in want]
    if n > 1:                                               # every class of the oracle occurs (the subgroup one only where the cofactor is not 1)
        assert set(st.tolist()) == ({0, 1, 2, 3, 4} if cid == 0 else {0, 1, 2, 3})
    one = fq_to_mont(cid, [1])[0]
    for i, (code, P) in enumerate(want):
        if code:
            assert not pts[i].any() and inf[i] == 0, i
        elif P is None:
            assert inf[i] == 1 and not pts[i, :L].any() and np.array_equal(pts[i, L:], one), i
        else:
            assert inf[i] == 0 and np.array_equal(pts[i], fq_to_mont(cid, list(P)).reshape(-1)), i


# ------------------------------------------------------------------------------------------------------------------ real proofs
class Real:
    """proofs of one circuit with their verifier, and the oracle's view of them"""

    def __init__(self, cid, log_n, ctx, vk, coeffs, proofs):
        self.cid, self.log_n, self.cv, self.ctx, self.vk = cid, log_n, bo.CURVES[cid], ctx, vk
        self.ca, self.cd = coeffs
        self.proofs = proofs                                 # [(bytes, {position: int})]
        self.vk_pts = oracle_points(cid, vk)
        self.bv = self.verifier_for(self.ca)
        self._exp = {}

    def seeded(self):
        return transcript.seed_transcript(transcript.Transcript(LABEL, self.cid), self.vk, 1 << self.log_n)

    def verifier_for(self, ca):
        m = lambda v: fr_to_mont(self.cid, [v])[0]          # noqa: E731
        return zk.BatchVerifier(self.vk, 1 << self.log_n, self.seeded(), m(ca), m(self.cd), self.cid, self.ctx)

    def pi(self, pub):
        return {i: fr_to_mont(self.cid, [v])[0] for i, v in pub.items()}

    def expansion(self, k):
        """proof k's two openings as the oracle forms them: [(combination of named bases, value)] each, chi, the point"""
        if k in self._exp:
            return self._exp[k]
        cv, p = self.cv, self.cv.r
        data, pub = self.proofs[k]
        proof = vo.parse_proof(cv, data)
        ev = proof["evals"]
        t = vo.seed_transcript(cv, wo.PlonkTranscript(LABEL, cv), self.vk_pts, 1 << self.log_n)
        ch = vo.replay_transcript(cv, t, proof, pub)
        ch.update(coeff_a=self.ca, coeff_d=self.cd)
        r0 = vo.compute_r0(cv, self.log_n, ev, ch, pub)
        lin = vo.linearisation_terms(cv, self.log_n, ev, ch)
        ze = ch["zeta"]
        table = [("table_1", 1), ("table_2", ze), ("table_3", ze * ze % p), ("table_4", ze * ze * ze % p)]
        C = lambda name: [(name, 1)]                        # noqa: E731
        aw = [(lin, -r0 % p), (C("sigma0"), ev["left_sigma_eval"]), (C("sigma1"), ev["right_sigma_eval"]), (C("sigma2"), ev["out_sigma_eval"]),
              (C("f_comm"), ev["f_eval"]), (C("h_2_comm"), ev["h2_eval"]), (table, ev["table_eval"]), (C("a_comm"), ev["a_eval"]),
              (C("b_comm"), ev["b_eval"]), (C("c_comm"), ev["c_eval"]), (C("d_comm"), ev["d_eval"])]
        saw = [(C("z_comm"), ev["permutation_eval"]), (C("a_comm"), ev["a_next_eval"]), (C("b_comm"), ev["b_next_eval"]),
               (C("d_comm"), ev["d_next_eval"]), (C("h_1_comm"), ev["h1_next_eval"]), (C("z_2_comm"), ev["z2_next_eval"]),
               (table, ev["table_next_eval"])]
        z = ch["z"]
        pts = dict(proof["commitments"], aw_opening=proof["aw_opening"], saw_opening=proof["saw_opening"])
        self._exp[k] = (aw, saw, ch["aw"], ch["saw"], z, z * cv.root_of_unity(self.log_n) % p, pts)
        return self._exp[k]

    def rows(self, k, u, v):
        """the 20 + 15 + 2 scalars of proof k under the weights (u, v), by expanding the lists"""
        p = self.cv.r
        aw, saw, chi, chj, z, zw, _ = self.expansion(k)
        acc = defaultdict(int)
        for pairs, c, w, point, opening in ((aw, chi, u, z, "aw_opening"), (saw, chj, v, zw, "saw_opening")):
            pw = w
            for comb, val in pairs:
                for name, s in comb:
                    acc[name] += pw * s
                acc["G"] -= pw * val
                pw = pw * c % p
            acc[opening] += w * point
        return [acc[k] % p for k in ORACLE_KEY + ("G",)], [acc[k] % p for k in PROOF_NAMES], [u % p, v % p]

    def definition(self, ks, weights):
        """(L, R) of the proofs ks from the definition, with the big-int group law"""
        cv = self.cv
        L = R = None
        for k, (u, v) in zip(ks, weights):
            key, prf, _ = self.rows(k, u, v)
            pts = self.expansion(k)[6]
            bases = [self.vk_pts[nm] for nm in ORACLE_KEY] + [(cv.gx, cv.gy)] + [pts[nm] for nm in PROOF_NAMES]
            for s, P in zip(key + prf, bases):
                if P is not None:
                    R = bo.ec_add(cv, R, bo.ec_mul(cv, s, P))
            for s, nm in ((u, "aw_opening"), (v, "saw_opening")):
                if pts[nm] is not None:
                    L = bo.ec_add(cv, L, bo.ec_mul(cv, s % cv.r, pts[nm]))
        return L, R


def point(cid, P):
    return None if P.infinity else (fq_from_mont(cid, P.x.reshape(1, -1))[0], fq_from_mont(cid, P.y.reshape(1, -1))[0])


def tau_relation(real, L, R):
    """e(L, [tau]H) == e(R, H) for the synthetic SRS: tau L == R"""
    return bo.ec_mul(real.cv, TAU, point(real.cid, L)) == point(real.cid, R)


def weights_for(B, seed):
    rng = np.random.default_rng(seed)
    return [tuple(int.from_bytes(rng.bytes(16), "little") | 1 for _ in range(2)) for _ in range(B)]


@pytest.fixture(scope="module")
def reals(ctx, oracle_cpu):
    out = {}
    for cid, log_n in ((0, 5), (0, 7), (1, 7)):
        cv, pk, ck, proof, pub, coeffs, wires = run_case(cid, log_n, ctx, oracle_cpu)
        out[(cid, log_n)] = Real(cid, log_n, ctx, proof.vk, coeffs, [(proof.to_bytes(), pub)])
        out[(cid, log_n)].dlog = dlogs(cid, ctx, pk, proof)             # polynomial(tau) behind every commitment: the oracle's verdict
    out["pi"] = pi_case(ctx, oracle_cpu)
    out["tamper"] = tamper_case(ctx, oracle_cpu)
    return out


def tamper_case(ctx, oracle_cpu):
    """The one proof of the tamper tests: 32 rows, and every input of the verifier reaches it.  build_circuit's 32-row circuit has no
    row of the two widgets that read the embedded curve's coefficients, so their selectors commit to the point at infinity and a
    verifier cannot tell one coeff_a from another there.  This is that circuit with one curve addition (widget/ecc/curve_addition.rs:
    62-97) in two of its all-zero padding rows: (x1, y1) + (x2, y2) in row n - 5, the sum and x1 y2 in the a, b, d wires of row n - 4,
    which has no selector of its own."""
    cid, log_n = 0, 5
    cv = bo.CURVES[cid]
    p, n = cv.r, 1 << log_n
    ca, cd = bo.seeded_scalars(cv, 0x51, 2)
    sel, sigma, table, wires, pub = build_circuit(cv, log_n, 7 + log_n + cid, False, (ca, cd))
    a, b, c, d = wires
    r = n - 5
    assert not any(sel[k][i] for k in sel for i in (r, r + 1)) and not any(w[i] for w in wires for i in (r, r + 1))
    x1, y1, x2, y2 = bo.seeded_scalars(cv, 0x77, 4)
    inv = lambda x: pow(x % p, -1, p)                          # noqa: E731
    x1y2, y1x2 = x1 * y2 % p, y1 * x2 % p
    a[r], b[r], c[r], d[r] = x1, y1, x2, y2
    a[r + 1] = (x1y2 + y1x2) * inv(1 + cd * x1y2 % p * y1x2) % p
    b[r + 1] = (y1 * y2 - ca * x1 * x2) * inv(1 - cd * x1y2 % p * y1x2) % p
    d[r + 1] = x1y2
    sel["q_variable_group_add"][r] = 1
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    dom4 = zk.Radix2EvaluationDomain.new(4 * n, cid, ctx)
    pk = prover.ProverKey(dom, dom4, {k: dev(cid, v) for k, v in sel.items()}, [dev(cid, s) for s in sigma], [dev(cid, t) for t in table])
    pw_canon, _ = tau_powers(oracle_cpu, cid, n + 8)
    ck = zk.CommitterKey(srs_from_powers(ctx, cid, pw_canon), cid, ctx)
    vk = pk.verifier_key(ck)
    pre = transcript.seed_transcript(transcript.Transcript(LABEL, cid), vk, n)
    proof = prover.prove(pk, ck, [dev(cid, w) for w in wires], {i: fr_to_mont(cid, [v])[0] for i, v in pub.items()}, pre,
                         fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0])
    real = Real(cid, log_n, ctx, vk, (ca, cd), [(proof.to_bytes(), pub)])
    real.dlog = dlogs(cid, ctx, pk, proof)
    assert real.vk_pts["q_var"] is not None
    return real


PI_LOG_N, PI_COUNTS = 8, (0, 1, 2, 65, 62, 63, 64)


def pi_case(ctx, oracle_cpu):
    """One circuit with 65 public-input rows -- rows 0 and n - 1 among them -- and proofs of it whose public inputs are non-zero at 0, 1, 2
    and 65 of those rows (the first four proofs), then at 62, 63 and 64 (a zero value is no entry of the reference's map).  build_circuit's circuit with its own public
    inputs taken out; the output wire c is in no copy constraint, so adding a public value to an arithmetic row only moves its c."""
    cid, log_n = 0, PI_LOG_N
    cv = bo.CURVES[cid]
    p, n = cv.r, 1 << log_n
    ca, cd = bo.seeded_scalars(cv, 0x51, 2)
    sel, sigma, table, wires, pub0 = build_circuit(cv, log_n, 99, False, (ca, cd))
    a, b, c, d = wires
    for i, v in pub0.items():
        c[i] = (c[i] - v) % p
    assert sel["q_arith"][0] == 1 and sel["q_arith"][n - 1] == 0
    sel["q_arith"][n - 1], sel["q_o"][n - 1] = 1, p - 1       # the last row: -c + pi = 0
    rows = [0] + [i for i in range(1, n - 1) if sel["q_arith"][i] == 1][:63] + [n - 1]
    assert len(rows) == 65
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    dom4 = zk.Radix2EvaluationDomain.new(4 * n, cid, ctx)
    pk = prover.ProverKey(dom, dom4, {k: dev(cid, v) for k, v in sel.items()}, [dev(cid, s) for s in sigma], [dev(cid, t) for t in table])
    pw_canon, _ = tau_powers(oracle_cpu, cid, n + 8)
    ck = zk.CommitterKey(srs_from_powers(ctx, cid, pw_canon), cid, ctx)
    vk = pk.verifier_key(ck)
    pre = transcript.seed_transcript(transcript.Transcript(LABEL, cid), vk, n)
    vals = bo.seeded_scalars(cv, 0x1234, 65)
    proofs = []
    for count in PI_COUNTS:
        chosen = {1: [0], 2: [0, 64]}.get(count, list(range(count)))        # indices into rows: 0 -> row 0, 64 -> row n - 1
        pub = {rows[k]: vals[k] for k in chosen}
        c2 = list(c)
        for i, v in pub.items():
            c2[i] = (c2[i] + v) % p
        pr = prover.prove(pk, ck, [dev(cid, w) for w in (a, b, c2, d)], {i: fr_to_mont(cid, [v])[0] for i, v in pub.items()}, pre,
                          fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0])
        proofs.append((pr.to_bytes(), pub))
    return Real(cid, log_n, ctx, vk, (ca, cd), proofs)


# ------------------------------------------------------------------------------------------------------------------ stage 3
@pytest.mark.parametrize("which", [(0, 5), (0, 7), (1, 7), "pi"])
@pytest.mark.parametrize("B", [1, 3, 65, 130])
def test_scalar_rows_match_the_expanded_oracle(which, B, reals):
    import torch
    real = reals[which]
    ks = [j % len(real.proofs) for j in range(B)]
    if which == "pi":
        ks = [(j + 3) % 4 for j in range(B)]                 # B = 1 takes the proof with 65 public inputs
    ws = weights_for(B, 1000 + B)
    st = real.bv.prepare([real.proofs[k][0] for k in ks], [real.pi(real.proofs[k][1]) for k in ks], ws)
    torch.cuda.synchronize()
    assert not st.any()
    key, prf, opn = (limbs_to_ints(t.cpu().numpy().view(np.uint64).reshape(-1, 4)) for t in real.bv.rows())
    for j, (k, (u, v)) in enumerate(zip(ks, ws)):
        wk, wp, wo_ = real.rows(k, u, v)
        assert key[20 * j:20 * j + 20] == wk, (j, "key")
        assert prf[15 * j:15 * j + 15] == wp, (j, "proof")
        assert opn[2 * j:2 * j + 2] == wo_, (j, "openings")
    if which == "pi":
        assert sorted({len(real.proofs[k][1]) for k in ks}) == sorted(set(PI_COUNTS[(j + 3) % 4] for j in range(B)))
        n = 1 << real.log_n
        assert all(0 in real.proofs[k][1] for k in (1, 2, 3)) and all(n - 1 in real.proofs[k][1] for k in (2, 3))


def test_scalar_rows_at_the_edges_of_an_inversion_round(reals):
    """verify_scalars inverts a proof's n_pi + 1 denominators in rounds of 64 with one inversion each (csrc/block_inverse.cuh): 0, 62 and
    63 public inputs are one round (63: every lane has an item), 64 and 65 go through the loop a second time and write the same LDS
    again.  One batch that mixes the counts, each of them twice; every row against the expanded oracle, exactly."""
    import torch
    real = reals["pi"]
    counts = (0, 62, 63, 64, 65, 64, 0, 65, 63, 62)
    ks = [PI_COUNTS.index(c) for c in counts]
    assert [len(real.proofs[k][1]) for k in ks] == list(counts)
    ws = weights_for(len(ks), 77)
    st = real.bv.prepare([real.proofs[k][0] for k in ks], [real.pi(real.proofs[k][1]) for k in ks], ws)
    torch.cuda.synchronize()
    assert not st.any()
    key, prf, opn = (limbs_to_ints(t.cpu().numpy().view(np.uint64).reshape(-1, 4)) for t in real.bv.rows())
    for j, (k, (u, v)) in enumerate(zip(ks, ws)):
        wk, wp, wo_ = real.rows(k, u, v)
        assert (key[20 * j:20 * j + 20], prf[15 * j:15 * j + 15], opn[2 * j:2 * j + 2]) == (wk, wp, wo_), (j, counts[j])


def test_a_challenge_on_the_domain_is_a_status(reals, ctx):
    """inverse(0) = 0 here: z = w^pos for a public input's position (or z = 1) would give a wrong sum without a word.  Stage 3 called on
    rows whose z is put on the domain reports it and zeroes the rows."""
    import torch
    real = reals[(0, 5)]
    data, pub = real.proofs[0]
    ch, ev, st = verifier.replay_batch(real.seeded(), [data] * 3, [real.pi(pub)] * 3, real.cid)
    w = real.cv.root_of_unity(real.log_n)
    ch[0, 11] = fr_to_mont(real.cid, [1])[0]                                   # z = 1: l_1's denominator
    ch[1, 11] = fr_to_mont(real.cid, [pow(w, 3, real.cv.r)])[0]                # z = w^3, a position of the extra public input below
    pis = [real.pi(pub), {**real.pi(pub), 3: fr_to_mont(real.cid, [5])[0]}, real.pi(pub)]
    m = lambda v: fr_to_mont(real.cid, [v])[0]                                  # noqa: E731
    key, prf, opn, st = verifier.scalar_rows(real.log_n, ch, ev, pis, m(real.ca), m(real.cd), weights_for(3, 5), None, None, real.cid, ctx)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [verifier.VERIFY_Z_ON_DOMAIN, verifier.VERIFY_Z_ON_DOMAIN, 0]
    assert not key[:2].any() and not prf[:2].any() and not opn[:2].any() and key[2].any()


# ------------------------------------------------------------------------------------------------------------------ stage 4
def fold_points(real, ks, ws, **kw):
    L, R, st = real.bv.fold([real.proofs[k][0] for k in ks], [real.pi(real.proofs[k][1]) for k in ks], ws, **kw)
    return L, R, st


@pytest.mark.parametrize("which,ks", [((0, 5), [0]), ("pi", [0, 3]), ((1, 7), [0])])
def test_fold_equals_the_definition(which, ks, reals):
    real = reals[which]
    ws = weights_for(len(ks), 77)
    L, R, st = fold_points(real, ks, ws)
    assert not st.any()
    wL, wR = real.definition(ks, ws)
    assert point(real.cid, L) == wL and point(real.cid, R) == wR
    assert wL is not None and bo.ec_mul(real.cv, TAU, wL) == wR          # ... and the proofs are valid


def test_fold_of_65_proofs_satisfies_the_pairing_equation(reals):
    real = reals["pi"]
    ks = [j % 4 for j in range(65)]
    L, R, st = fold_points(real, ks, None)                               # weights from the operating system
    assert not st.any() and not L.infinity and tau_relation(real, L, R)
    L2, R2, _ = fold_points(real, ks, None)
    assert L2 != L and R2 != R                                           # ... and never the same twice


def test_fold_of_a_range_equals_the_fold_of_the_sublist(reals):
    real = reals["pi"]
    ks = [0, 1, 2, 3, 2, 1, 0]
    ws = weights_for(len(ks), 31)
    for lo, hi in ((2, 5), (0, 1), (6, 7), (0, 7)):
        L, R, _ = fold_points(real, ks, ws, lo=lo, hi=hi)
        L2, R2, _ = fold_points(real, ks[lo:hi], ws[lo:hi])
        assert L == L2 and R == R2 and tau_relation(real, L, R), (lo, hi)
    L, R = real.bv.fold_range(3, 3)
    assert L.infinity and R.infinity


# ------------------------------------------------------------------------------------------------------------------ tampering
def eval_plus_one(real, data, i):
    cv = real.cv
    g, f = wo.fq_flag_bytes(cv), wo.fr_bytes(cv)
    o = 15 * g + 2 + i * f
    v = (int.from_bytes(data[o:o + f], "little") + 1) % cv.r
    return data[:o] + v.to_bytes(f, "little") + data[o + f:]


def point_replaced(real, data, i, enc=None):
    cv = real.cv
    g = wo.fq_flag_bytes(cv)
    o = i * g + (1 if i == 14 else 0)
    enc = enc or wo.ser_g1(cv, (cv.gx, cv.gy))
    return data[:o] + enc + data[o + g:]


def rejected(real, data, pub, ws=None, bv=None):
    bv = bv or real.bv
    L, R, st = bv.fold([data], [real.pi(pub)], ws or weights_for(1, 9))
    return bool(st[0]) or not tau_relation(real, L, R)


def test_tamper_valid_proof_is_accepted(reals):
    real = reals["tamper"]
    data, pub = real.proofs[0]
    assert not rejected(real, data, pub)


def test_tamper_each_evaluation_plus_one(reals):
    real = reals["tamper"]
    data, pub = real.proofs[0]
    got = [rejected(real, eval_plus_one(real, data, i), pub) for i in range(16)]
    print("\nevaluation + 1 rejected:", dict(zip(vo.EVALS, got)))
    for i in range(16):
        assert got[i], ("evaluation", vo.EVALS[i])


def test_verdicts_on_changed_evaluations_are_the_oracles(reals):
    """The oracle is the definition: for each of the sixteen evaluations plus 1 the fold's verdict is the restated verifier's."""
    real = reals["tamper"]
    data, pub = real.proofs[0]
    for i in range(16):
        bad = eval_plus_one(real, data, i)
        t = vo.seed_transcript(real.cv, wo.PlonkTranscript(LABEL, real.cv), real.vk_pts, 1 << real.log_n)
        ok = vo.verify_with_trapdoor(real.cv, real.log_n, bad, t, pub, real.dlog, TAU, real.ca, real.cd)[0]
        assert rejected(real, bad, pub) == (not ok), vo.EVALS[i]


def test_tamper_each_point_replaced_by_the_generator(reals):
    real = reals["tamper"]
    data, pub = real.proofs[0]
    for i in range(15):
        assert point_replaced(real, data, i) != data
        assert rejected(real, point_replaced(real, data, i), pub), ("point", i)


def test_tamper_public_input_plus_one(reals):
    real = reals["tamper"]
    data, pub = real.proofs[0]
    assert pub
    k = sorted(pub)[0]
    assert rejected(real, data, {**pub, k: (pub[k] + 1) % real.cv.r})


def test_tamper_wrong_coeff_a(reals):
    """The same 32-row proof verified under coeff_a + 1.  coeff_a enters Proof::verify through the scalars of q_fixed_group_add and
    q_variable_group_add alone (proof.rs:488-611), so the proof's circuit must have a row of one of them: tamper_case puts a curve
    addition there.  (On a circuit with neither, both commitments are the point at infinity and no verifier can see coeff_a.)"""
    real = reals["tamper"]
    data, pub = real.proofs[0]
    assert real.log_n == 5 and real.vk_pts["q_var"] is not None
    bv = real.verifier_for((real.ca + 1) % real.cv.r)
    try:
        got = rejected(real, data, pub, bv=bv)
    finally:
        bv.close()
    print("\nwrong coeff_a rejected at 32 rows:", got)
    assert got


def test_tamper_wrong_coeff_a_where_the_circuit_has_the_widgets(reals):
    """coeff_a enters through the fixed-base and curve-addition widgets alone; the circuit of 128 rows has both."""
    real = reals[(0, 7)]
    data, pub = real.proofs[0]
    assert not rejected(real, data, pub)
    assert real.vk_pts["q_fixed"] is not None and real.vk_pts["q_var"] is not None
    bv = real.verifier_for((real.ca + 1) % real.cv.r)
    try:
        assert rejected(real, data, pub, bv=bv)
    finally:
        bv.close()


def test_tamper_weights_of_the_wrong_proof(reals):
    """u and u' of a pair exchanged between the two proofs: L under the weights (w0, w1) against R under (w1, w0) and the reverse"""
    real = reals["pi"]
    ws = weights_for(2, 3)
    two = [real.proofs[0], real.proofs[3]]
    args = ([d for d, _ in two], [real.pi(p) for _, p in two])
    L, R, _ = real.bv.fold(*args, ws)
    Ls, Rs, _ = real.bv.fold(*args, ws[::-1])
    assert tau_relation(real, L, R) and tau_relation(real, Ls, Rs)
    assert not tau_relation(real, L, Rs) and not tau_relation(real, Ls, R)


def off_curve(real):
    cv = real.cv
    g = wo.fq_flag_bytes(cv)
    enc = (1).to_bytes(g, "little")                                      # BLS12-381: x = 1 has no point
    assert oracle_decode(cv, enc)[0] == verifier.G1_NOT_ON_CURVE
    return enc


def test_mixed_batch_is_bisected(reals):
    real = reals[(0, 5)]
    data, pub = real.proofs[0]
    B = 9
    datas = [data] * B
    datas[0] = point_replaced(real, data, 5, off_curve(real))
    datas[4] = eval_plus_one(real, data, 2)
    datas[8] = eval_plus_one(real, data, 13)
    pis = [real.pi(pub)] * B
    ws = weights_for(B, 41)
    L, R, st = real.bv.fold(datas, pis, ws)
    assert not tau_relation(real, L, R)
    assert st.tolist() == [verifier.VERIFY_BAD_POINT + verifier.G1_NOT_ON_CURVE] + [0] * 8
    calls = []

    def accepts(L, R):
        calls.append(1)
        return tau_relation(real, L, R)

    assert real.bv.locate_invalid(datas, pis, accepts, ws) == [0, 4, 8]
    assert len(calls) <= 1 + 2 * 3 * 4                                   # 1 + 2 k ceil(log2 B) = 25
    good = [j for j in range(B) if j not in (0, 4, 8)]
    L, R, st = real.bv.fold([datas[j] for j in good], [pis[j] for j in good], [ws[j] for j in good])
    assert not st.any() and tau_relation(real, L, R)
    assert real.bv.locate_invalid([datas[j] for j in good], [pis[j] for j in good], accepts) == []


def test_an_undecodable_proof_drops_out_of_the_fold(reals):
    real = reals["pi"]
    ks = [1, 0, 3]
    datas = [real.proofs[k][0] for k in ks]
    pis = [real.pi(real.proofs[k][1]) for k in ks]
    ws = weights_for(3, 8)
    for bad in (point_replaced(real, datas[0], 14, off_curve(real)), datas[0][:-1]):
        L, R, st = real.bv.fold([bad] + datas[1:], pis, ws)
        assert st[0] != 0 and not st[1:].any()
        L2, R2, _ = real.bv.fold(datas[1:], pis[1:], ws[1:])
        assert L == L2 and R == R2 and tau_relation(real, L, R)
