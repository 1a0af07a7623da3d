"""PLONK over the inner-product-argument commitment end to end on the MI355X: `prover.prove(..., ck=<IpaCommitterKey>)` and
`verifier.IpaBatchVerifier` against the reference verifier on integers (tests/ipa_plonk_ref.py: oracle/verifier_oracle.py composed with
tests/ipa_oracle.py over a known-logarithm key).  The tau-powers of tests/conftest.py are the comm_key, h a known multiple of G, and
test_prover_gpu.dlogs gives every commitment's logarithm, so the reference does Fr arithmetic and a point only where one is hashed.
Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ark_plonk_amd as zk  # noqa: E402
from ark_plonk_amd import prover, transcript  # noqa: E402
from ark_plonk_amd.curves import fr_to_mont, limbs_to_ints  # noqa: E402
from ark_plonk_amd.ipa import IpaCommitterKey  # noqa: E402
from ark_plonk_amd.verifier import IpaBatchVerifier  # noqa: E402
from oracle import bigint_oracle as bo  # noqa: E402
from oracle import verifier_oracle as vo  # noqa: E402
from oracle import wire_oracle as wo  # noqa: E402
from tests import ipa_plonk_ref as ref  # noqa: E402
from tests.conftest import srs_from_powers, tau_powers  # noqa: E402
from tests.test_prover_gpu import (assert_proof_bytes_equal_the_cpu_restatement, build_circuit, dev, dlogs, oracle_points,  # noqa: E402
                                   run_case)

pytestmark = pytest.mark.gpu
LABEL = b"end to end"
K_H = 0x5EED0F1A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E                  # h = K_H G
WHICH = [(0, 5), (0, 7), (1, 7), "pi"]
PI_LOG_N = 8


class Case:
    def __init__(self, ctx, oracle_cpu, cid, log_n, pk, kzg_proof, vk, pub, coeffs, wires):
        self.cid, self.log_n, self.ctx, self.cv = cid, log_n, ctx, bo.CURVES[cid]
        cv, n = self.cv, 1 << log_n
        self.vk, self.pub, (self.ca, self.cd) = vk, pub, coeffs
        self.vk_pts = oracle_points(cid, vk)
        pw_canon, _ = tau_powers(oracle_cpu, cid, n)
        self.key_logs = limbs_to_ints(pw_canon)                                  # comm_key[i] = tau^i G: d1 = n points
        self.ipa_key = IpaCommitterKey(srs_from_powers(ctx, cid, pw_canon), bo.ec_mul(cv, K_H, (cv.gx, cv.gy)), cid, ctx)
        m = lambda v: fr_to_mont(cid, [v])[0]                                    # noqa: E731
        self.prove = lambda key: prover.prove(pk, key, [dev(cid, w) for w in wires], self.pi(pub), self.seeded(), m(self.ca), m(self.cd))  # noqa: E731
        self.kzg_bytes = kzg_proof.to_bytes()
        self.proof = self.prove(self.ipa_key)
        self.data = self.proof.to_bytes()
        self.dlog = dlogs(cid, ctx, pk, kzg_proof)                               # the 13 commitments are the KZG proof's (test b)
        self.g = wo.fq_flag_bytes(cv)
        self.ipa_len = 16 + (2 * log_n + 1) * self.g + 34
        self._verifiers = {}

    def seeded(self):
        return transcript.seed_transcript(transcript.Transcript(LABEL, self.cid), self.vk, 1 << self.log_n)

    def pi(self, pub):
        return {i: fr_to_mont(self.cid, [v])[0] for i, v in pub.items()}

    def verifier(self, replay="host", ca=None):
        key = (replay, ca)
        if key not in self._verifiers:
            m = lambda v: fr_to_mont(self.cid, [v])[0]                            # noqa: E731
            self._verifiers[key] = IpaBatchVerifier(self.vk, 1 << self.log_n, self.seeded(), m(self.ca if ca is None else ca), m(self.cd),
                                                    self.ipa_key, self.cid, self.ctx, replay=replay)
        return self._verifiers[key]

    def accepted(self, data, pub=None, ca=None):
        return self.verifier("host", ca).verify([data], [self.pi(self.pub if pub is None else pub)])

    def ref(self, data, pub=None, dlog=None, ca=None):
        return ref.verify(self.cv, self.log_n, data, self.vk_pts, self.pub if pub is None else pub, dlog or self.dlog, self.key_logs, K_H,
                          self.ca if ca is None else ca, self.cd)

    # -- where things stand in the bytes
    def evals_at(self):
        return 13 * self.g + 2 * self.ipa_len

    def eval_offsets(self):
        """offsets of the 16 fixed and the 7 custom evaluations"""
        at = self.evals_at()
        out = [at + 32 * i for i in range(16)]
        pos = at + 16 * 32
        k = int.from_bytes(self.data[pos:pos + 8], "little")
        pos += 8
        for _ in range(k):
            ln = int.from_bytes(self.data[pos:pos + 8], "little")
            pos += 8 + ln
            out.append(pos)
            pos += 32
        assert pos == len(self.data) and len(out) == 23
        return out

    def put(self, at, chunk):
        return self.data[:at] + chunk + self.data[at + len(chunk):]

    def scalar_plus_one(self, at):
        v = (int.from_bytes(self.data[at:at + 32], "little") + 1) % self.cv.r
        return self.put(at, v.to_bytes(32, "little"))

    def gen(self):
        return wo.ser_g1(self.cv, (self.cv.gx, self.cv.gy))

    def ipa_field(self, k, name, i=0):
        """offset of a field of opening k (0: aw, 1: saw): "l" / "r" point i, "key", "c" """
        at = 13 * self.g + k * self.ipa_len
        return at + {"l": 8 + i * self.g, "r": 16 + (self.log_n + i) * self.g, "key": 16 + 2 * self.log_n * self.g,
                     "c": 16 + (2 * self.log_n + 1) * self.g}[name]


def pi_circuit(ctx, oracle_cpu):
    """test_verifier_gpu.pi_case's circuit (65 public-input rows, rows 0 and n - 1 among them) with all 65 values non-zero"""
    cid, log_n = 0, PI_LOG_N
    cv = bo.CURVES[cid]
    p, n = cv.r, 1 << log_n
    ca, cd = bo.seeded_scalars(cv, 0x51, 2)
    sel, sigma, table, wires, pub0 = build_circuit(cv, log_n, 99, False, (ca, cd))
    a, b, c, d = wires
    for i, v in pub0.items():
        c[i] = (c[i] - v) % p
    sel["q_arith"][n - 1], sel["q_o"][n - 1] = 1, p - 1
    rows = [0] + [i for i in range(1, n - 1) if sel["q_arith"][i] == 1][:63] + [n - 1]
    pub = dict(zip(rows, bo.seeded_scalars(cv, 0x1234, 65)))
    for i, v in pub.items():
        c[i] = (c[i] + v) % p
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    dom4 = zk.Radix2EvaluationDomain.new(4 * n, cid, ctx)
    pk = prover.ProverKey(dom, dom4, {k: dev(cid, v) for k, v in sel.items()}, [dev(cid, s) for s in sigma], [dev(cid, t) for t in table])
    pw_canon, _ = tau_powers(oracle_cpu, cid, n + 8)
    ck = zk.CommitterKey(srs_from_powers(ctx, cid, pw_canon), cid, ctx)
    vk = pk.verifier_key(ck)
    pre = transcript.seed_transcript(transcript.Transcript(LABEL, cid), vk, n)
    kzg = prover.prove(pk, ck, [dev(cid, w) for w in wires], {i: fr_to_mont(cid, [v])[0] for i, v in pub.items()}, pre,
                       fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0])
    return Case(ctx, oracle_cpu, cid, log_n, pk, kzg, vk, pub, (ca, cd), wires)


@pytest.fixture(scope="module")
def cases(ctx, oracle_cpu):
    out = {}
    for cid, log_n in WHICH[:3]:
        cv, pk, ck, kzg, pub, coeffs, wires = run_case(cid, log_n, ctx, oracle_cpu)
        out[(cid, log_n)] = Case(ctx, oracle_cpu, cid, log_n, pk, kzg, kzg.vk, pub, coeffs, wires)
    out["pi"] = pi_circuit(ctx, oracle_cpu)
    return out


@pytest.mark.parametrize("which", WHICH)
def test_device_proof_is_accepted_by_the_integer_verifier(which, cases):
    case = cases[which]
    ok, det = case.ref(case.data)
    assert ok, det
    assert len(case.data) == len(case.kzg_bytes) + 2 * (case.ipa_len - case.g - 1)


@pytest.mark.parametrize("which", WHICH)
def test_commitments_and_evaluations_are_the_kzg_proofs(which, cases):
    """Only the openings differ: the 13 commitments and the 23 evaluations (16 fixed, then the labelled ones) are the same bytes."""
    case = cases[which]
    g = case.g
    assert case.data[:13 * g] == case.kzg_bytes[:13 * g]
    assert case.data[case.evals_at():] == case.kzg_bytes[15 * g + 2:]
    assert case.prove(case.ipa_key).to_bytes() == case.data                      # and the IPA proof is a function of its inputs


@pytest.mark.parametrize("B", [1, 3, 65, 130])
@pytest.mark.parametrize("which", WHICH)
def test_batches_of_copies_are_accepted_on_both_replay_routes(which, B, cases):
    case = cases[which]
    seen = []
    for route in ("host", "device"):
        v = case.verifier(route)
        assert v.verify([case.data] * B, [case.pi(case.pub)] * B)
        assert not v.last["status"].any()
        seen.append((v.last["C"], v.last["v"]))
        assert v.locate_invalid([case.data] * B, [case.pi(case.pub)] * B) == []
    assert seen[0] == seen[1]


@pytest.mark.parametrize("which", WHICH)
def test_combined_commitments_and_values_are_the_integer_verifiers(which, cases):
    case = cases[which]
    ok, det = case.ref(case.data)
    v = case.verifier("host")
    assert v.verify([case.data] * 3, [case.pi(case.pub)] * 3)
    assert v.last["C"] == det["C"] * 3 and v.last["v"] == [tuple(det["v"])] * 3
    assert det["C"][0] is not None and det["C"][1] is not None and det["C"][0] != det["C"][1]


def same_verdict(case, data, pub=None, dlog=None, ca=None):
    got = case.accepted(data, pub, ca)
    want, _ = case.ref(data, pub, dlog, ca)
    assert got == want, (got, want)
    return got


@pytest.mark.parametrize("part", [range(0, 6), range(6, 12), range(12, 18), range(18, 23)])       # 16 fixed, then the 7 labelled ones
@pytest.mark.parametrize("which", WHICH)
def test_tamper_each_evaluation_plus_one(which, part, cases):
    case = cases[which]
    offs = case.eval_offsets()
    for i in part:
        assert not same_verdict(case, case.scalar_plus_one(offs[i])), ("evaluation", i)


@pytest.mark.parametrize("which", WHICH)
def test_the_untampered_proof_has_the_integer_verifiers_verdict(which, cases):
    assert same_verdict(cases[which], cases[which].data)


@pytest.mark.parametrize("part", [range(0, 7), range(7, 13)])
@pytest.mark.parametrize("which", WHICH)
def test_tamper_each_commitment_replaced_by_the_generator(which, part, cases):
    case = cases[which]
    for i in part:
        name = vo.COMMITMENTS[i]
        bad = case.put(i * case.g, case.gen())
        assert bad != case.data
        assert not same_verdict(case, bad, dlog=dict(case.dlog, **{name: 1})), name


@pytest.mark.parametrize("which", WHICH)
def test_tamper_the_fields_of_the_openings(which, cases):
    case = cases[which]
    for k, name, i in ((0, "l", 0), (1, "r", case.log_n - 1), (1, "l", 1), (0, "key", 0), (1, "key", 0)):
        bad = case.put(case.ipa_field(k, name, i), case.gen())
        assert bad != case.data
        assert not same_verdict(case, bad), (k, name, i)
    for k in (0, 1):
        assert not same_verdict(case, case.scalar_plus_one(case.ipa_field(k, "c"))), ("c", k)


@pytest.mark.parametrize("which", WHICH)
def test_tamper_public_input_plus_one(which, cases):
    case = cases[which]
    assert case.pub
    k = sorted(case.pub)[-1]
    assert not same_verdict(case, case.data, pub={**case.pub, k: (case.pub[k] + 1) % case.cv.r})


def test_tamper_wrong_coeff_a_where_the_circuit_has_the_widgets(cases):
    case = cases[(0, 7)]
    assert case.vk_pts["q_fixed"] is not None and case.vk_pts["q_var"] is not None
    assert not same_verdict(case, case.data, ca=(case.ca + 1) % case.cv.r)


@pytest.mark.parametrize("which", WHICH)
def test_mixed_batch_is_located(which, cases):
    case = cases[which]
    B = 65
    datas = [case.data] * B
    offs = case.eval_offsets()
    datas[0] = case.put(5 * case.g, case.gen())
    datas[31] = case.scalar_plus_one(offs[2])
    datas[64] = case.scalar_plus_one(case.ipa_field(1, "c"))
    datas[10] = case.put(case.ipa_field(0, "l") - 8, (case.log_n + 1).to_bytes(8, "little"))        # a bad L count
    pis = [case.pi(case.pub)] * B
    for route in ("host", "device"):
        v = case.verifier(route)
        assert not v.verify(datas, pis)
        assert v.locate_invalid(datas, pis) == [0, 10, 31, 64]
    good = [j for j in range(B) if j not in (0, 10, 31, 64)]
    assert case.verifier("host").verify([datas[j] for j in good], [pis[j] for j in good])
    for j in (0, 10, 31, 64):
        assert not case.ref(datas[j], dlog=dict(case.dlog, f_comm=1) if j == 0 else None)[0]


@pytest.mark.parametrize("cid,log_n", WHICH[:3])
def test_kzg_proof_bytes_are_unchanged(cid, log_n, ctx, oracle_cpu):
    assert_proof_bytes_equal_the_cpu_restatement(cid, log_n, ctx, oracle_cpu)


def test_a_polynomial_longer_than_the_key_is_refused(cases, ctx, oracle_cpu):
    case = cases[(0, 5)]
    pw_canon, _ = tau_powers(oracle_cpu, 0, 16)
    short = IpaCommitterKey(srs_from_powers(ctx, 0, pw_canon), bo.ec_mul(case.cv, K_H, (case.cv.gx, case.cv.gy)), 0, ctx)
    with pytest.raises(ValueError):
        case.prove(short)
