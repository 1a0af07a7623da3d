"""The inner-product-argument commitment on the MI355X (ark_plonk_amd/ipa.py over ark_plonk_amd/csrc/ipa.hip) against the
pure-Python oracle of tests/ipa_oracle.py: the key-fold kernel with its edge cases, whole openings byte for byte, the device check,
the final key through the SRS table path, and the ABI's behaviour next to KZG work on the same ctx.  Keys are known-logarithm test
keys G_i = k_i G (generated on the device by the fixed-base utility), so the oracle does Fr arithmetic only."""
import ctypes

import numpy as np
import pytest

import ipa_oracle as io
from oracle import bigint_oracle as bo

pytestmark = pytest.mark.gpu
CURVES = {0: bo.BLS12_381, 1: bo.BN254}


def rand_logs(cv, n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 1 << 63, size=(n, 5), dtype=np.uint64)
    return [(int(a) | int(b) << 63 | int(c) << 126 | int(d) << 189 | int(e) << 252) % cv.r for a, b, c, d, e in raw.tolist()]


def points_of(ctx, cid, logs):
    """k_i G on the device (affine Montgomery, (n, 2L) int64 tensor; k = 0 gives x = y = 0, infinity)."""
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib
    L = zk.get_curve(cid).fq_limbs
    sc = torch.from_numpy(zk.curves.ints_to_limbs(logs, 4).view(np.int64)).cuda()
    out = torch.empty((len(logs), 2 * L), dtype=torch.int64, device="cuda")
    ctx.use_torch_stream()
    _lib.check(_lib.lib().zk_g1_fixed_base_batch_dev(ctx.handle, cid, sc.data_ptr(), len(logs), out.data_ptr()))
    torch.cuda.synchronize()
    return out


def key_of(ctx, cid, d1, seed, precompute=True):
    import ark_plonk_amd as zk
    from ark_plonk_amd.ipa import IpaCommitterKey
    cv = CURVES[cid]
    logs = rand_logs(cv, d1 + 1, seed)
    logs, k_h = logs[:d1], logs[d1]
    bases = points_of(ctx, cid, logs).cpu().numpy().view(np.uint64)
    h = bo.ec_mul(cv, k_h, (cv.gx, cv.gy))
    ck = IpaCommitterKey(bases, h, zk.get_curve(cid), ctx)
    if precompute and d1 >= 1 << 14:
        ck.precompute()
    return ck, logs, k_h


def polys_mont(cid, n_polys, deg, seed):
    import ark_plonk_amd as zk
    cv = CURVES[cid]
    coeffs = [rand_logs(cv, deg, seed + k) for k in range(n_polys)]
    return coeffs, [zk.curves.fr_to_mont(cid, c) for c in coeffs]


def ipa_case(ctx, cid, d1, digest, n_polys=2, seed=1, deg=None, point=None):
    cv = CURVES[cid]
    ck, logs, k_h = key_of(ctx, cid, d1, seed)
    coeffs, pm = polys_mont(cid, n_polys, d1 if deg is None else deg, seed + 100)
    z = rand_logs(cv, 2, seed + 7)
    z, chi = (z[0] if point is None else point), z[1]
    KL = io.KnownLog(cv)
    comms_l = [io.commit(KL, logs, c) for c in coeffs]
    comms = ck.commit(pm)
    assert comms == [KL.point(c) for c in comms_l]
    proof = ck.open(pm, comms, z, chi, digest)
    exp = io.open_(KL, logs, k_h, coeffs, comms_l, z, chi, digest)
    return ck, coeffs, comms, z, chi, proof, exp


@pytest.mark.parametrize("cid", [0, 1])
def test_fold_key_matches_the_group_law_incl_edge_cases(ctx, cid):
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib
    cv = CURVES[cid]
    r = cv.r
    L = zk.get_curve(cid).fq_limbs
    for m, xi in ((300, rand_logs(cv, 1, 3)[0]), (1, 5), (129, 1), (200, r - 1)):
        kr = rand_logs(cv, m, 10 + m)
        kl = rand_logs(cv, m, 20 + m)
        if m >= 8:
            kl[0] = (-xi * kr[0]) % r          # k_l = -xi k_r: the result is infinity
            kl[1] = xi * kr[1] % r             # k_l = xi k_r: the final addition doubles
            kl[2] = 0                          # infinity as k_l (x = y = 0)
            kr[3] = 0                          # infinity as k_r
            kl[4], kr[4] = 0, 0
        key = points_of(ctx, cid, kl + kr)
        inf = torch.zeros(2 * m, dtype=torch.uint8, device="cuda")
        if m >= 8:
            inf[5] = 1                         # infinity by flag, with a finite point's bytes under it
            kl[5] = 0
        out = torch.zeros((m, 2 * L), dtype=torch.int64, device="cuda")
        oinf = torch.zeros(m, dtype=torch.uint8, device="cuda")
        xm = zk.curves.fr_to_mont(cid, [xi])
        _lib.check(_lib.lib().zk_ipa_fold_key_dev(ctx.handle, cid, m, key.data_ptr(), inf.data_ptr(), xm.ctypes.data, out.data_ptr(),
                                                  oinf.data_ptr()))
        got = out.cpu().numpy().view(np.uint64)
        gi = oinf.cpu().numpy()
        for i in range(m):
            e = (kl[i] + xi * kr[i]) % r
            if e == 0:
                assert gi[i] == 1, (m, i)
                continue
            P = bo.ec_mul(cv, e, (cv.gx, cv.gy))
            assert gi[i] == 0 and zk.curves.fq_from_mont(cid, got[i].reshape(2, L)) == [P[0], P[1]], (m, xi, i)


@pytest.mark.parametrize("m", [1, 127, 128, 129])
@pytest.mark.parametrize("cid", [0, 1])
def test_fold_key_at_the_edges_of_a_workgroup(ctx, cid, m):
    """The key fold normalises 128 results with one inversion (block_inverse.cuh); a lane with no finite result enters the products
    as 1.  Half-lengths around the workgroup: one lane, one lane short of a workgroup, a whole one, one lane into the second.  The
    three kinds of special lane -- a result at infinity (k_l = -xi k_r), a null k_r, a null k_l -- stand at lane 0, at the last active
    lane and in the middle (m = 1: one fold per kind), the rest are random; every lane against the oracle's group law, bit for bit."""
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib
    cv = CURVES[cid]
    r = cv.r
    L = zk.get_curve(cid).fq_limbs
    xi = rand_logs(cv, 1, 40 + m)[0]
    kinds = ("infinity", "null k_r", "null k_l")
    places = [{0: k} for k in kinds] if m == 1 else [{0: "infinity", m - 1: "null k_r", m // 2: "null k_l", 1: "null k_r", m - 2: "infinity"}]
    for place in places:
        kr = rand_logs(cv, m, 50 + m)
        kl = rand_logs(cv, m, 60 + m)
        for i, kind in place.items():
            if kind == "infinity":
                kl[i] = (-xi * kr[i]) % r
            elif kind == "null k_r":
                kr[i] = 0
            else:
                kl[i] = 0
        key = points_of(ctx, cid, kl + kr)
        inf = torch.zeros(2 * m, dtype=torch.uint8, device="cuda")
        out = torch.zeros((m, 2 * L), dtype=torch.int64, device="cuda")
        oinf = torch.zeros(m, dtype=torch.uint8, device="cuda")
        xm = zk.curves.fr_to_mont(cid, [xi])
        _lib.check(_lib.lib().zk_ipa_fold_key_dev(ctx.handle, cid, m, key.data_ptr(), inf.data_ptr(), xm.ctypes.data, out.data_ptr(),
                                                  oinf.data_ptr()))
        got = out.cpu().numpy().view(np.uint64)
        gi = oinf.cpu().numpy()
        for i in range(m):
            e = (kl[i] + xi * kr[i]) % r
            assert (e == 0) == (place.get(i) == "infinity"), (m, i)
            if e == 0:
                assert gi[i] == 1, (m, i, place)
                continue
            P = bo.ec_mul(cv, e, (cv.gx, cv.gy))
            assert gi[i] == 0 and zk.curves.fq_from_mont(cid, got[i].reshape(2, L)) == [P[0], P[1]], (m, i, place.get(i))


@pytest.mark.parametrize("digest", ["blake2b", "blake2s"])
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("log_d1", range(1, 13))
def test_open_matches_the_oracle_and_checks(ctx, log_d1, cid, digest):
    ck, coeffs, comms, z, chi, proof, exp = ipa_case(ctx, cid, 1 << log_d1, digest, seed=log_d1 * 10 + cid)
    assert proof == exp
    values = [bo.horner(c, z, CURVES[cid].r) for c in coeffs]
    assert ck.check(comms, z, values, proof, chi, digest)
    bad = io.IpaProof(list(proof.l_vec), list(proof.r_vec), proof.final_comm_key, (proof.c + 1) % CURVES[cid].r)
    assert not ck.check(comms, z, values, bad, chi, digest)
    ck.close()


@pytest.mark.parametrize("cid,digest,log_d1", [(0, "blake2b", 16), (1, "blake2s", 16), (0, "blake2s", 19), (1, "blake2b", 19),
                                               (0, "blake2b", 21), (1, "blake2s", 21)])
def test_large_open_matches_the_oracle_and_the_final_key_msm(ctx, cid, digest, log_d1):
    ck, coeffs, comms, z, chi, proof, exp = ipa_case(ctx, cid, 1 << log_d1, digest, seed=log_d1 + 1000 * cid, deg=(1 << log_d1) // 2)
    assert proof == exp
    assert proof.l_vec[0] is None            # degree < d1 / 2: a_r = 0 in round 0
    values = [bo.horner(c, z, CURVES[cid].r) for c in coeffs]
    assert ck.check(comms, z, values, proof, chi, digest)
    bad_values = [(values[0] + 1) % CURVES[cid].r] + values[1:]
    assert not ck.check(comms, z, bad_values, proof, chi, digest)
    ck.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_proof_shaped_openings_at_2_16(ctx, cid):
    """prover.rs:582-618: 11 polynomials at z and 7 at z * omega, n = 2^16 (d + 1 = 2n)."""
    import ark_plonk_amd as zk
    cv = CURVES[cid]
    n = 1 << 16
    ck, logs, k_h = key_of(ctx, cid, 2 * n, 77 + cid)
    KL = io.KnownLog(cv)
    omega = bo.CURVES[cid].root_of_unity(16)
    z = rand_logs(cv, 3, 5 + cid)
    for n_polys, point, chi in ((11, z[0], z[1]), (7, z[0] * omega % cv.r, z[2])):
        coeffs, pm = polys_mont(cid, n_polys, n, 300 + n_polys)
        comms = ck.commit(pm)
        proof = ck.open(pm, comms, point, chi, "blake2b")
        exp = io.open_(KL, logs, k_h, coeffs, [io.commit(KL, logs, c) for c in coeffs], point, chi, "blake2b")
        assert proof == exp
        assert ck.check(comms, point, [bo.horner(c, point, cv.r) for c in coeffs], proof, chi, "blake2b")
    ck.close()


def test_pending_round_interleaving_bad_arguments_and_kzg_after(ctx):
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib
    cid, cv = 0, CURVES[0]
    d1 = 1 << 14
    ck, logs, k_h = key_of(ctx, cid, d1, 4242)
    kzg_key = ck.key
    coeffs, pm = polys_mont(cid, 2, d1, 900)
    poly_dev = torch.from_numpy(pm[0].view(np.int64)).cuda()
    before = kzg_key.commit(poly_dev)
    comms = ck.commit(pm)
    z, chi = rand_logs(cv, 2, 31)
    KL = io.KnownLog(cv)
    exp = io.open_(KL, logs, k_h, coeffs, [io.commit(KL, logs, c) for c in coeffs], z, chi, "blake2s")
    # KZG commits on the same ctx between the rounds of an opening
    seen = []
    proof = ck.open(pm, comms, z, chi, "blake2s", between_rounds=lambda j: seen.append(kzg_key.commit(poly_dev)))
    assert proof == exp and len(seen) == 14 and all(s == before for s in seen)
    # a KZG commit after the opening still gives the same point
    assert kzg_key.commit(poly_dev) == before
    # ZK_ERR_PENDING while a deferred KZG round is open; the round closes as usual afterwards
    L = zk.get_curve(cid).fq_limbs
    a = torch.zeros((d1, 4), dtype=torch.int64, device="cuda")
    b = torch.zeros((d1, 4), dtype=torch.int64, device="cuda")
    work = torch.empty(_lib.lib().zk_ipa_workspace_bytes(cid, d1), dtype=torch.uint8, device="cuda")
    hp = np.zeros(2 * L, dtype=np.uint64)
    out = np.zeros(4 * L, dtype=np.uint64)
    oinf = np.zeros(2, dtype=np.uint8)
    lib = _lib.lib()

    def rnd(h, first, m):
        return lib.zk_ipa_round_dev(ctx.handle, h, first, m, a.data_ptr(), b.data_ptr(), work.data_ptr(), hp.ctypes.data, out.ctypes.data,
                                    oinf.ctypes.data)

    kzg_key.commit_begin([poly_dev])
    assert rnd(kzg_key._h, 1, d1 // 2) == _lib.ZK_ERR_PENDING
    assert kzg_key.round_end(1) == [before]
    # bad arguments
    assert rnd(None, 1, d1 // 2) == _lib.ZK_ERR_BAD_ARG
    assert rnd(kzg_key._h, 1, d1) == _lib.ZK_ERR_BAD_ARG          # 2m > d + 1
    assert rnd(kzg_key._h, 0, d1 // 2) == _lib.ZK_ERR_BAD_ARG     # the folded key holds d1 / 2 points
    assert rnd(kzg_key._h, 1, 3) == _lib.ZK_ERR_BAD_ARG           # not a power of two
    assert lib.zk_ipa_round_dev(None, kzg_key._h, 1, 4, a.data_ptr(), b.data_ptr(), work.data_ptr(), hp.ctypes.data, out.ctypes.data,
                                oinf.ctypes.data) == _lib.ZK_ERR_BAD_ARG
    three = zk.CommitterKey(points_of(ctx, cid, [1, 2, 3]).cpu().numpy().view(np.uint64), cid, ctx)
    assert rnd(three._h, 1, 1) == _lib.ZK_ERR_BAD_ARG              # d + 1 = 3 is not a power of two
    three.close()
    assert lib.zk_ipa_workspace_bytes(cid, 3) == 0
    ck.close()
