"""CPU suite of circuit compilation (ark_plonk_amd/compile.py): the restated definition of the wire permutation reproduces the two
expected outputs the reference itself holds (tests/golden/sigma_reference_cases.json), its two forms agree, the verifier key's byte
layout round-trips, and `from_gates` emits the canonical insertion order.  No device compute."""
import json
import os

import numpy as np

import ark_plonk_amd as zk
from ark_plonk_amd import _lib
from ark_plonk_amd import compile as zc
from oracle import bigint_oracle as bo
from tests import compile_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "sigma_reference_cases.json")))["cases"]


def test_restated_definition_reproduces_the_reference_cases():
    assert len(CASES) == 2
    for case in CASES:
        n = case["n"]
        ins_var, ins_pos = cr.canonical_insertions(n, *zip(*case["gates"]))
        want = [p for wire in case["sigma_pos"] for p in wire]
        assert cr.sigma_dict(n, ins_var, ins_pos) == want, case["source"]
        assert cr.sigma_numpy(n, ins_var, ins_pos).tolist() == want, case["source"]
        for cid in (0, 1):
            cv = bo.CURVES[cid]
            w = cv.root_of_unity(2)
            enc = cr.encode(cv.r, w, n, want)
            assert enc == [[cr.K[k] * pow(w, e, cv.r) % cv.r for k, e in wire] for wire in case["sigma_enc"]], (case["source"], cid)


def test_both_forms_agree_on_skewed_random_input():
    rng = np.random.default_rng(5)
    for log_n in (3, 7, 12):
        n = 1 << log_n
        m = 4 * n - 3
        var = rng.integers(1, 2 * n, size=m)
        var[rng.random(m) < 0.5] = 0                     # half of all positions on the zero variable
        pos = rng.permutation(4 * n)[:m]
        a = cr.sigma_numpy(n, var, pos)
        assert a.tolist() == cr.sigma_dict(n, var, pos)
        assert sorted(a.tolist()) == list(range(4 * n))
        assert cr.cycle_count(a) == len(set(var.tolist())) + 4 * n - m


def test_padded_size_is_the_circuit_bound():
    assert [zc.padded_size(g, t) for g, t in ((1, 0), (4, 0), (5, 0), (5, 9), (1024, 1024), (1025, 3))] == [1, 4, 8, 16, 1024, 2048]


def test_verifier_key_bytes_round_trip():
    for cid in (0, 1):
        cv = zk.get_curve(cid)
        pts = {}
        for i, name in enumerate(zc.VK_FIELDS):
            xy = None if i == 7 else zk.curves.g1_mul(cv, 3 + 5 * i)      # one commitment of an all-zero selector: infinity
            if xy is None:
                L = cv.fq_limbs
                pts[name] = zk.G1Affine(np.zeros(L, dtype=np.uint64), zk.curves.fq_to_mont(cv, [1])[0], True, cv.name)
            else:
                m = zk.curves.fq_to_mont(cv, list(xy))
                pts[name] = zk.G1Affine(m[0], m[1], False, cv.name)
        vk = zc.VerifierKey(1 << 11, pts, cv)
        data = vk.to_bytes()
        assert len(data) == 8 + 20 * _lib.lib().zk_g1_compressed_size(cid)
        assert data[:8] == (1 << 11).to_bytes(8, "little")
        back = zc.VerifierKey.from_bytes(data, cv)
        assert back.n == vk.n and dict(back) == dict(vk) and back.to_bytes() == data
        assert data[8:8 + (len(data) - 8) // 20] == zk.transcript.g1_serialize(pts["q_m"], cv)
        # it is the dict seed_transcript takes: two transcripts seeded from the key and from its bytes draw the same challenge
        t1 = vk.seed(zk.transcript.Transcript(b"vk", cv))
        t2 = zk.transcript.seed_transcript(zk.transcript.Transcript(b"vk", cv), dict(back), back.n)
        assert np.array_equal(t1.challenge_scalar(b"c"), t2.challenge_scalar(b"c"))


def test_from_gates_emits_the_canonical_insertion_order():
    case = CASES[1]
    n = case["n"]
    w = [list(c) for c in zip(*case["gates"])]
    d = zc.CircuitDescription.from_gates({}, *w, num_vars=case["num_vars"], device="cpu")
    ins_var, ins_pos = cr.canonical_insertions(n, *w)
    assert d.size() == n and d.n_gates == n
    assert d.ins_var.tolist() == ins_var and d.ins_pos.tolist() == ins_pos
    # a table longer than the gates sets the padded size, and with it the positions
    import torch
    d2 = zc.CircuitDescription.from_gates({}, *w, num_vars=4, table_cols=[torch.zeros((9, 4), dtype=torch.int64)], device="cpu")
    assert d2.size() == 16 and d2.ins_pos.tolist() == cr.canonical_insertions(16, *w)[1]
