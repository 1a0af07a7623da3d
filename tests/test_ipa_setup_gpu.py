"""The IPA key derivation on the MI355X (ark_plonk_amd/ipa.py over csrc/ipa_setup.hip: zk_ipa_sample_generators_dev,
zk_g1_from_random_bytes_batch_dev, IpaUniversalParams) against the checker on Python integers (tests/ipa_setup_ref.py).  Points, infinity
flags, attempt counts and statuses are compared exactly, index by index.  The checker costs about 5 ms per BLS12-381 generator (the
cofactor multiplication), so it is asked for a few hundred points per case, computed once and shared."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ark_plonk_amd as zk  # noqa: E402
from ark_plonk_amd import _lib, ipa, prover, transcript  # noqa: E402
from ark_plonk_amd.curves import fq_from_mont, fr_to_mont  # noqa: E402
from ark_plonk_amd.verifier import IpaBatchVerifier  # noqa: E402
from oracle import bigint_oracle as bo  # noqa: E402
from tests import edge_values as ev  # noqa: E402
from tests import ipa_oracle as io  # noqa: E402
from tests import ipa_setup_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
CHUNK = 512                      # ZK_H2C_CHUNK: indices per wavefront


def rows_of(curve, xy, inf):
    """device rows -> (x, y) | "inf" | None (a null row: all-zero words, flag 0)"""
    cv = zk.get_curve(curve)
    L = cv.fq_limbs
    xy = xy.cpu().numpy().view(np.uint64).reshape(-1, 2 * L)
    inf = inf.cpu().numpy()
    out = []
    for k in range(xy.shape[0]):
        if inf[k]:
            assert fq_from_mont(cv, xy[k].reshape(2, L)) == [0, 1], k            # GroupAffine::zero()
            out.append("inf")
        elif not xy[k].any():
            out.append(None)
        else:
            out.append(tuple(fq_from_mont(cv, xy[k].reshape(2, L))))
    return out


def derive(ctx, curve, digest, first, n, max_tries=0):
    xy, inf, tries, st, rounds = ipa._sample_generators_raw(curve, n, first, digest, ctx, max_tries)
    import torch
    torch.cuda.synchronize()
    return rows_of(curve, xy, inf), tries.cpu().numpy().tolist(), st.cpu().numpy().tolist(), rounds.cpu().numpy().tolist()


def expected(curve, digest, first, n, cap=0):
    """(rows, tries, statuses) of the checker; under a cap exactly the indices that need more attempts run out"""
    rows, tries, sts = [], [], []
    for st, p, a, _ in ref.generators(curve, digest, first, n):
        assert st == ref.OK
        if cap and a > cap:
            rows.append(None), tries.append(cap), sts.append(ref.EXHAUSTED)
        else:
            rows.append("inf" if p is bo.INF else p), tries.append(a), sts.append(ref.OK)
    return rows, tries, sts


@pytest.mark.parametrize("curve, digest", ref.COMBOS)
def test_ranges_equal_the_checker_index_by_index(ctx, curve, digest):
    """n around the wavefront's width at first_index 0; 65 from index 59 (the 39-attempt index of BN254 / blake2b) and from 2^32 - 3
    (the index crosses its low word); and a range is the concatenation of its parts"""
    whole = None
    for first, n in [(0, 0), (0, 1), (0, 2), (0, 63), (0, 64), (0, 65), (0, 130), (59, 65), (2 ** 32 - 3, 65)]:
        rows, tries, st, rounds = derive(ctx, curve, digest, first, n)
        want = expected(curve, digest, first, n)
        assert (rows, tries, st) == want, (first, n)
        assert len(rounds) == (n + CHUNK - 1) // CHUNK
        if (first, n) == (0, 130):
            whole = (rows, tries, st)
    if (curve, digest) == ("bn254", "blake2b"):
        assert whole[1][59] == 39
    a, b = derive(ctx, curve, digest, 0, 64), derive(ctx, curve, digest, 64, 66)
    assert tuple(x + y for x, y in zip(a[:3], b[:3])) == whole
    # the public function: the same points, and no complaint
    xy, inf = ipa.sample_generators(curve, 65, 59, digest, ctx)
    assert rows_of(curve, xy, inf) == whole[0][59:124]


@pytest.mark.parametrize("first", [2 ** 48 - 3, 2 ** 64 - 7])
@pytest.mark.parametrize("curve, digest", ref.COMBOS)
def test_indices_with_non_zero_upper_words(ctx, curve, digest, first):
    """The preimage splits the 64-bit index over three words of the message and shares the last of them with the retry counter.
    Six indices from 2^48 - 3 (the index crosses into the low half of that shared word) and from 2^64 - 7 (every bit of it set; the
    last range whose first + n does not wrap): points, attempt counts and statuses against the checker, index by index."""
    rows, tries, st, rounds = derive(ctx, curve, digest, first, 6)
    want = expected(curve, digest, first, 6)
    assert (rows, tries, st) == want, first
    assert len(rows) == 6 and len(rounds) == 1
    # not the points of the same range with the upper words dropped
    assert rows != expected(curve, digest, first % 2 ** 32, 6)[0]


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("curve, digest", ref.COMBOS)
def test_max_tries_exhausts_exactly_the_indices_that_need_more(ctx, curve, digest, cap):
    rows, tries, st, _ = derive(ctx, curve, digest, 0, 130, max_tries=cap)
    want = expected(curve, digest, 0, 130, cap)
    assert (rows, tries, st) == want
    assert ref.EXHAUSTED in st and ref.OK in st
    assert all((r is None) == (s == ref.EXHAUSTED) for r, s in zip(rows, st))
    with pytest.raises(RuntimeError):
        ipa.sample_generators(curve, 130, 0, digest, ctx, max_tries=cap)


def crafted(curve):
    """G-byte buffers for the corner cases of from_random_bytes, as (x, flag bits 7..6, extra top bits) -> bytes"""
    cv = bo.CURVES[curve]
    g = 8 * cv.fq_limbs
    enc = lambda x, flags=0: (x | flags << (8 * g - 2)).to_bytes(g, "little")                  # noqa: E731
    on = [x for x in range(2, 60) if ref.from_random_bytes(curve, enc(x))[0] == ref.OK][:2]
    off = [x for x in range(2, 60) if ref.from_random_bytes(curve, enc(x))[0] == ref.NOT_ON_CURVE][:2]
    assert len(on) == 2 and len(off) == 2
    out = [enc(0, 1), enc(0), enc(1, 1), enc(on[0], 1), enc(0, 3), enc(on[0], 3), enc(cv.q - 1), enc(cv.q), enc(cv.q + 1), enc(cv.q, 1), enc(cv.q, 3),
           enc(cv.q - 1, 2), enc(1), enc(1, 2)]
    for x in on + off:
        out += [enc(x), enc(x, 2)]                                                            # both signs of y; a non-residue under either flag
    if curve == "bls12_381":
        out += [(int.from_bytes(enc(on[0]), "little") | 1 << 381).to_bytes(g, "little"),      # bit 381: cleared, not rejected
                (int.from_bytes(enc(on[1], 2), "little") | 1 << 381).to_bytes(g, "little"),
                (int.from_bytes(enc(cv.q - 1), "little") | 1 << 381).to_bytes(g, "little")]
    for t, _ in ev.fq_targets(cv.q):                                                          # the base field's edges as x
        if t < 1 << (8 * g - 2):
            out += [enc(t), enc(t, 2)]
    return out


@pytest.mark.parametrize("clear", [0, 1])
@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_from_random_bytes_on_crafted_strings(ctx, curve, clear):
    """every corner case of the rule in ONE batch per string length, so that neighbours cannot disturb each other; lengths 0, 1,
    G - 1, G, G + 1 and 64 (a shorter string is zero-extended, a longer one cut: the bytes beyond G are filled with 0xa5 here)"""
    import torch
    cv = zk.get_curve(curve)
    L, g = cv.fq_limbs, 8 * cv.fq_limbs
    cases = crafted(curve)
    seen = set()
    for length in (0, 1, g - 1, g, g + 1, 64):
        strings = [(c + b"\xa5" * 64)[:length] if length > g else c[:length] for c in cases]
        n = len(strings)
        d_in = torch.from_numpy(np.frombuffer(b"".join(strings) or b"\x00", dtype=np.uint8).copy()).cuda()
        xy = torch.full((n, 2 * L), -1, dtype=torch.int64, device="cuda")
        inf = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
        ctx.use_torch_stream()
        _lib.check(_lib.lib().zk_g1_from_random_bytes_batch_dev(ctx.handle, cv.curve_id, d_in.data_ptr(), length, n, clear, xy.data_ptr(), inf.data_ptr(),
                                                                st.data_ptr()))
        torch.cuda.synchronize()
        rows, got_st = rows_of(curve, xy, inf), st.cpu().numpy().tolist()
        for k, s in enumerate(strings):
            wst, p, _ = ref.from_random_bytes(curve, s)
            if wst == ref.OK and p is not bo.INF and clear:
                p = ref.clear_cofactor(curve, p)
            want = None if wst != ref.OK else "inf" if p is bo.INF else p
            assert (got_st[k], rows[k]) == (wst, want), (length, k, s.hex())
            seen.add(wst)
            if want not in (None, "inf"):
                assert bo.on_curve(bo.CURVES[curve], want)
    assert seen == {ref.OK, ref.BAD_FLAGS, ref.X_NOT_REDUCED, ref.NOT_ON_CURVE, ref.INF_FLAG_X_NONZERO}


@pytest.mark.parametrize("curve, digest", ref.COMBOS)
def test_wave_local_search_runs_about_two_roots_per_index(ctx, curve, digest):
    """n = 2^16: every index resolves, sixteen sampled indices equal the checker (the last index of the first wavefront's chunk and the
    first of the second among them), and the wavefronts ran at most 4 n / 64 square-root rounds in all.  That is a condition on the
    schedule, not a timing: the candidates need about 2 n roots (1.965 to 2.015 per index in the CPU model), a per-lane loop would run
    about 7 n lane-slots (every wavefront as long as its unluckiest lane), and the bound leaves a factor of two for the chunk tails."""
    import torch
    n = 1 << 16
    xy, inf, d_tries, d_st, d_rounds = ipa._sample_generators_raw(curve, n, 0, digest, ctx, 0)
    torch.cuda.synchronize()
    assert int(d_st.max()) == ref.OK and int(inf.max()) == 0 and bool((xy != 0).any(dim=1).all())
    tries, rounds = d_tries.cpu().numpy().tolist(), d_rounds.cpu().numpy().tolist()
    assert len(rounds) == _lib.lib().zk_ipa_sample_generators_waves(n) == n // CHUNK
    sampled = [0, 1, 63, 64, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 4097, 12345, 20000, 32767, 32768, 50001, n - 2, n - 1]
    rows = rows_of(curve, xy[sampled], inf[sampled])
    for k, i in enumerate(sampled):
        wst, p, a, _ = ref.generators(curve, digest, i, 1)[0]
        assert (rows[k], tries[i]) == (p, a), i
    slots = 64 * sum(rounds)
    print(f"{curve} {digest}: {slots / n:.3f} lane-slots of square root per index, {sum(tries) / n:.3f} attempts per index")
    assert slots <= 4 * n
    assert 64 * sum(rounds) >= 1.9 * n                   # and no fewer than the candidates need: every root is counted


def test_argument_errors(ctx):
    L = _lib.lib()
    bad = _lib.ZK_ERR_BAD_ARG
    import torch
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert L.zk_ipa_sample_generators_dev(None, 0, 0, 0, 1, 0, p, p, None, p, None) == bad
    assert L.zk_ipa_sample_generators_dev(ctx.handle, 7, 0, 0, 1, 0, p, p, None, p, None) == bad
    assert L.zk_ipa_sample_generators_dev(ctx.handle, 0, 2, 0, 1, 0, p, p, None, p, None) == bad
    assert L.zk_ipa_sample_generators_dev(ctx.handle, 0, 0, 0, 1, 0, None, p, None, p, None) == bad
    assert L.zk_ipa_sample_generators_dev(ctx.handle, 0, 0, 0, 1, 0, p, None, None, p, None) == bad
    assert L.zk_ipa_sample_generators_dev(ctx.handle, 0, 0, 0, 1, 0, p, p, None, None, None) == bad
    assert L.zk_ipa_sample_generators_dev(ctx.handle, 0, 0, 2 ** 64 - 1, 2, 0, p, p, None, p, None) == bad
    assert L.zk_ipa_sample_generators_dev(ctx.handle, 0, 0, 0, 0, 0, None, None, None, None, None) == 0
    assert L.zk_g1_from_random_bytes_batch_dev(None, 0, p, 4, 1, 0, p, p, p) == bad
    assert L.zk_g1_from_random_bytes_batch_dev(ctx.handle, 9, p, 4, 1, 0, p, p, p) == bad
    assert L.zk_g1_from_random_bytes_batch_dev(ctx.handle, 0, None, 4, 1, 0, p, p, p) == bad
    assert L.zk_g1_from_random_bytes_batch_dev(ctx.handle, 0, p, 4, 1, 0, p, p, None) == bad
    assert L.zk_g1_from_random_bytes_batch_dev(ctx.handle, 0, None, 0, 0, 0, None, None, None) == 0
    assert [L.zk_ipa_sample_generators_waves(k) for k in (0, 1, CHUNK, CHUNK + 1)] == [0, 1, 1, 2]
    # optional outputs left out: the points are the same
    rows, _, _, _ = derive(ctx, "bn254", "blake2s", 0, 5)
    xy, inf = ipa.sample_generators("bn254", 5, 0, "blake2s", ctx)
    assert rows_of("bn254", xy, inf) == rows


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_commit_open_check_over_a_derived_key(ctx, curve):
    """setup(15) then trim(7): h and s are the checker's generators 17 and 16, the key its generators 0 .. 7; commitments equal the
    big-int MSM over those points; open and check agree with the protocol's restatement over real points (tests/ipa_oracle.py)"""
    cv = bo.CURVES[curve]
    digest = "blake2b"
    pp = ipa.IpaUniversalParams.setup(15, curve, digest, ctx)
    gens = [p for _, p, _, _ in ref.generators(curve, digest, 0, 18)]
    assert pp.max_degree == 15 and pp.h == gens[17] and pp.s == gens[16]
    assert rows_of(curve, *pp.comm_key) == gens[:16]
    with pytest.raises(ValueError):
        pp.trim(16)
    ck = pp.trim(7)
    assert ck.d1 == 8 and ck.h == gens[17] and ck.s == gens[16]
    key = gens[:8]
    coeffs = [bo.seeded_scalars(cv, 0x1DA + k, deg) for k, deg in enumerate((8, 5))]
    pm = [fr_to_mont(curve, c) for c in coeffs]
    comms = ck.commit(pm)
    G = io.Generic(cv)
    assert comms == [bo.msm(cv, key, c) for c in coeffs] == [io.commit(G, key, c) for c in coeffs]
    z, chi = bo.seeded_scalars(cv, 0x77, 2)
    proof = ck.open(pm, comms, z, chi, digest)
    exp = io.open_(G, key, gens[17], coeffs, comms, z, chi, digest)
    assert (proof.l_vec, proof.r_vec, proof.final_comm_key, proof.c) == (exp.l_vec, exp.r_vec, exp.final_comm_key, exp.c)
    values = [bo.horner(c, z, cv.r) for c in coeffs]
    assert ck.check(comms, z, values, proof, chi, digest) and io.check(G, key, gens[17], comms, z, values, proof, chi, digest)
    wrong = [values[0], (values[1] + 1) % cv.r]
    assert not ck.check(comms, z, wrong, proof, chi, digest) and not io.check(G, key, gens[17], comms, z, wrong, proof, chi, digest)
    # the full trim is the whole comm_key
    assert pp.trim(15).d1 == 16 and pp.trim(8).d1 == 16


def test_plonk_proof_over_a_key_from_setup_and_trim(ctx):
    """The 32-row circuit of tests/test_ipa_plonk_gpu.py proved over a key from setup(31) and trim(31), and verified by
    IpaBatchVerifier over the same key.  The integer reference verifier of that file computes in the key's logarithms and so needs a
    known-logarithm key; a derived key has none -- that is its point -- so the verdicts here are the device verifier's alone, on the
    honest proof and on the proof with one evaluation byte flipped."""
    from tests.test_prover_gpu import build_circuit, dev
    cid, log_n = 0, 5
    cv, n = bo.CURVES[cid], 32
    ca, cd = bo.seeded_scalars(cv, 0x51, 2)
    sel, sigma, table, wires, pub = build_circuit(cv, log_n, 7 + log_n + cid, False, (ca, cd))
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    dom4 = zk.Radix2EvaluationDomain.new(4 * n, cid, ctx)
    pk = prover.ProverKey(dom, dom4, {k: dev(cid, v) for k, v in sel.items()}, [dev(cid, s) for s in sigma], [dev(cid, t) for t in table])
    ck = ipa.IpaUniversalParams.setup(n - 1, cid, "blake2b", ctx).trim(n - 1)
    assert ck.d1 == n
    vk = pk.verifier_key(ck.key)
    seeded = lambda: transcript.seed_transcript(transcript.Transcript(b"end to end", cid), vk, n)        # noqa: E731
    m = lambda v: fr_to_mont(cid, [v])[0]                                                                  # noqa: E731
    pi = {i: m(v) for i, v in pub.items()}
    proof = prover.prove(pk, ck, [dev(cid, w) for w in wires], pi, seeded(), m(ca), m(cd))
    data = proof.to_bytes()
    v = IpaBatchVerifier(vk, n, seeded(), m(ca), m(cd), ck, cid, ctx)
    assert v.verify([data], [pi])
    g = 8 * zk.get_curve(cid).fq_limbs
    ipa_len = 16 + (2 * log_n + 1) * g + 34
    at = 13 * g + 2 * ipa_len                           # the first of the 16 fixed evaluations (tests/test_ipa_plonk_gpu.py: evals_at)
    bad = data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]
    assert not v.verify([bad], [pi])
    assert v.verify([data, data], [pi, pi]) and not v.verify([data, bad], [pi, pi])
