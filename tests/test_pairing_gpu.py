"""The device side of the pairing check (csrc/pairing.hip: one check per lane) against the host side, which tests/test_pairing.py pins
to an independent pairing -- so the device is pinned transitively -- and `BatchVerifier`'s yes / no answers on real proofs against the
trapdoor relation tau L == R that the other verifier tests use in the pairing's place."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ark_plonk_amd as zk  # noqa: E402
from ark_plonk_amd import _lib, verifier  # noqa: E402
from ark_plonk_amd.context import ptr_of  # noqa: E402
from ark_plonk_amd.curves import fq_to_mont, fr_to_mont, g1_mul, get_curve  # noqa: E402
from ark_plonk_amd.pairing import PairingKey  # noqa: E402
from tests.conftest import TAU  # noqa: E402

pytestmark = pytest.mark.gpu
CURVES = ("bls12_381", "bn254")
SIZES = (1, 63, 64, 65, 130)          # the lane tail, one full wave, a wave boundary, the multi-workgroup tail


@pytest.fixture(scope="module")
def keys():
    out = {name: PairingKey.from_trapdoor(TAU, name) for name in CURVES}
    yield out
    for k in out.values():
        k.close()


_POINTS = {}


def scalar_points(cv, ks):
    """k G for every k (0: infinity, written as (0, 1) with its flag) -> ((n, 2L) uint64 Montgomery, (n,) uint8)"""
    L = cv.fq_limbs
    xy = np.zeros((len(ks), 2 * L), dtype=np.uint64)
    inf = np.zeros(len(ks), dtype=np.uint8)
    one = fq_to_mont(cv, [1]).reshape(-1)
    for i, k in enumerate(ks):
        key = (cv.name, k % cv.r)
        if key not in _POINTS:
            _POINTS[key] = g1_mul(cv, k)
        p = _POINTS[key]
        if p is None:
            xy[i, L:] = one
            inf[i] = 1
        else:
            xy[i] = fq_to_mont(cv, list(p)).reshape(-1)
    return xy, inf


def to_dev(a, ctx):
    import torch
    t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a)
    return t.to(torch.device("cuda", ctx.device)).contiguous()


def gt_scalars(cv, n):
    """n scalars from a pool of five distinct points (the host side is computed once per distinct point), infinity at the first, the
    last and a middle index, and (r - 1) G"""
    pool = [1, 2, cv.r - 1, 0xDEADBEEF, TAU]
    ks = [pool[i % len(pool)] for i in range(n)]
    for i in {0, n // 2, n - 1}:
        ks[i] = 0
    if n > 3:
        ks[1] = cv.r - 1
    return ks


@pytest.fixture(scope="module")
def host_gt(keys):
    cache = {}

    def get(name, which, k):
        cv = get_curve(name)
        kk = (name, which, k % cv.r)
        if kk not in cache:
            xy, inf = scalar_points(cv, [k])
            P = zk.G1Affine(xy[0, :cv.fq_limbs], xy[0, cv.fq_limbs:], bool(inf[0]), cv.name)
            cache[kk] = keys[name].gt(P, which)
        return cache[kk]
    return get


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", CURVES)
def test_gt_batch_equals_the_host(name, n, which, keys, host_gt, ctx):
    cv = get_curve(name)
    ks = gt_scalars(cv, n)
    xy, inf = scalar_points(cv, ks)
    got = keys[name].gt_batch(to_dev(xy, ctx), to_dev(inf, ctx), which, ctx).cpu().numpy().view(np.uint64)
    assert got.shape == (n, 12, cv.fq_limbs)
    for i, k in enumerate(ks):
        assert np.array_equal(got[i], host_gt(name, which, k)), (i, hex(k))


@pytest.mark.parametrize("name", CURVES)
def test_gt_batch_reads_infinity_by_encoding_when_there_are_no_flags(name, keys, host_gt, ctx):
    cv = get_curve(name)
    xy, inf = scalar_points(cv, [0, 5, 0])
    xy[2, cv.fq_limbs:] = 0                                              # (0, 0)
    got = keys[name].gt_batch(to_dev(xy, ctx), None, 1, ctx).cpu().numpy().view(np.uint64)
    assert np.array_equal(got[0], host_gt(name, 1, 0)) and np.array_equal(got[2], host_gt(name, 1, 0))
    assert np.array_equal(got[1], host_gt(name, 1, 5))


@pytest.mark.parametrize("name", CURVES)
def test_check_batch_equals_the_trapdoor_verdict(name, keys, ctx):
    cv = get_curve(name)
    n = 130
    rng = np.random.default_rng(7)
    pool = [3, 0xABCDEF, cv.r - 2, int.from_bytes(rng.bytes(31), "little")]
    ls, rs, want = [], [], []
    for i in range(n):
        k = pool[i % len(pool)]
        kind = i % 5
        if kind == 0:                                  # valid
            ls.append(k), rs.append(k * TAU), want.append(1)
        elif kind == 1:                                # R off by G
            ls.append(k), rs.append(k * TAU + 1), want.append(0)
        elif kind == 2:                                # R negated
            ls.append(k), rs.append(-k * TAU), want.append(0)
        elif kind == 3:                                # both infinity
            ls.append(0), rs.append(0), want.append(1)
        else:                                          # one of them infinity
            ls.append(0 if i % 2 else k), rs.append(k if i % 2 else 0), want.append(0)
    want[n - 1], ls[n - 1], rs[n - 1] = 1, cv.r - 1, (cv.r - 1) * TAU        # the last lane of the tail: valid
    for l, r, w in zip(ls, rs, want):                                        # the trapdoor verdict: tau L == R
        assert w == int(l * TAU % cv.r == r % cv.r)
    lxy, linf = scalar_points(cv, ls)
    rxy, rinf = scalar_points(cv, rs)
    ok = keys[name].check_batch(to_dev(lxy, ctx), to_dev(linf, ctx), to_dev(rxy, ctx), to_dev(rinf, ctx), ctx).cpu().numpy()
    assert ok.tolist() == want
    for i in (0, 1, 2, 3, 4, n - 1):                                         # ... and the host check says the same
        L = zk.G1Affine(lxy[i, :cv.fq_limbs], lxy[i, cv.fq_limbs:], bool(linf[i]), cv.name)
        R = zk.G1Affine(rxy[i, :cv.fq_limbs], rxy[i, cv.fq_limbs:], bool(rinf[i]), cv.name)
        assert keys[name].check(L, R) == bool(want[i]), i


@pytest.mark.parametrize("name", CURVES)
def test_an_empty_batch_touches_nothing(name, keys, ctx):
    import torch
    cv = get_curve(name)
    dev = torch.device("cuda", ctx.device)
    canary = torch.full((64,), 0x5A, dtype=torch.uint8, device=dev)
    lib = _lib.lib()
    assert lib.zk_kzg_pairing_check_batch_dev(ctx.handle, keys[name]._h, ptr_of(canary), None, ptr_of(canary), None, 0, ptr_of(canary)) == _lib.ZK_OK
    assert lib.zk_pairing_gt_batch_dev(ctx.handle, keys[name]._h, 0, ptr_of(canary), None, 0, ptr_of(canary)) == _lib.ZK_OK
    assert lib.zk_kzg_pairing_check_batch_dev(ctx.handle, keys[name]._h, None, None, None, None, 0, None) == _lib.ZK_OK
    ctx.sync()
    assert bool((canary == 0x5A).all())
    e = torch.empty((0, 2 * cv.fq_limbs), dtype=torch.int64, device=dev)
    assert keys[name].check_batch(e, None, e, None, ctx).numel() == 0 and keys[name].gt_batch(e, None, 0, ctx).numel() == 0
    # null arrays with n > 0 are a code, not a launch
    assert lib.zk_kzg_pairing_check_batch_dev(ctx.handle, keys[name]._h, None, None, None, None, 1, None) == _lib.ZK_ERR_BAD_ARG
    assert lib.zk_pairing_gt_batch_dev(ctx.handle, keys[name]._h, 0, None, None, 1, None) == _lib.ZK_ERR_BAD_ARG


# ------------------------------------------------------------------------------------------------------------------ real proofs
@pytest.fixture(scope="module")
def cases(ctx, oracle_cpu, keys):
    """test_verifier_gpu's small circuits, one per curve, each with a verifier that has the pairing key"""
    from tests import test_verifier_gpu as tv
    from tests.test_prover_gpu import run_case
    out = {}
    for cid, log_n in ((0, 5), (1, 7)):
        cv, pk, ck, proof, pub, coeffs, wires = run_case(cid, log_n, ctx, oracle_cpu)
        real = tv.Real(cid, log_n, ctx, proof.vk, coeffs, [(proof.to_bytes(), pub)])
        m = lambda v: fr_to_mont(cid, [v])[0]          # noqa: E731
        name = CURVES[cid]
        real.pbv = zk.BatchVerifier(real.vk, 1 << log_n, real.seeded(), m(real.ca), m(real.cd), cid, ctx, pairing_key=keys[name])
        out[name] = real
    yield out
    for real in out.values():
        real.pbv.close()
        real.bv.close()


def mixed_batch(real, B=9):
    """B copies of the valid proof with one undecodable point (a status) and two changed evaluations (caught by the pairing alone)"""
    from tests import test_verifier_gpu as tv
    data, pub = real.proofs[0]
    datas = [data] * B
    enc = tv.off_curve(real) if real.cid == 0 else None
    if enc is not None:
        datas[0] = tv.point_replaced(real, data, 5, enc)
    else:
        datas[0] = data[:-1]                                                 # truncated: a parse status
    datas[4] = tv.eval_plus_one(real, data, 2)
    datas[8] = tv.eval_plus_one(real, data, 13)
    return datas, [real.pi(pub)] * B, tv.weights_for(B, 41)


@pytest.mark.parametrize("name", CURVES)
def test_verify_says_yes_to_valid_proofs_and_no_to_a_changed_byte(name, cases):
    from tests import test_verifier_gpu as tv
    real = cases[name]
    data, pub = real.proofs[0]
    B = 9
    pis = [real.pi(pub)] * B
    assert real.pbv.verify([data] * B, pis) is True                         # weights from the operating system
    assert real.pbv.verify([data] * B, pis, tv.weights_for(B, 5)) is True
    assert real.pbv.verify([], []) is True
    g, f = tv.wo.fq_flag_bytes(real.cv), tv.wo.fr_bytes(real.cv)
    o = 15 * g + 2 + 3 * f                                                   # the first byte of the fourth evaluation
    flipped = data[:o] + bytes([data[o] ^ 1]) + data[o + 1:]
    datas = [data] * B
    datas[6] = flipped
    assert real.pbv.verify(datas, pis) is False
    assert real.pbv.verify([data[:-1]] + [data] * (B - 1), pis) is False     # a non-zero status: no pairing needed


@pytest.mark.parametrize("name", CURVES)
def test_locate_invalid_with_the_key_equals_locate_invalid_with_the_trapdoor(name, cases):
    from tests import test_verifier_gpu as tv
    real = cases[name]
    datas, pis, ws = mixed_batch(real)
    want = real.pbv.locate_invalid(datas, pis, lambda L, R: tv.tau_relation(real, L, R), ws)
    assert want == [0, 4, 8]
    assert real.pbv.locate_invalid(datas, pis, weights=ws) == want
    assert real.pbv.locate_invalid(datas, pis) == want                       # ... and under fresh weights
    with pytest.raises(ValueError):
        real.bv.locate_invalid(datas, pis)                                   # neither a key nor a check


@pytest.mark.parametrize("name", CURVES)
def test_verdicts_equal_the_per_proof_trapdoor_verdicts(name, cases):
    from tests import test_verifier_gpu as tv
    real = cases[name]
    datas, pis, ws = mixed_batch(real)
    got = real.pbv.verdicts(datas, pis, ws)
    assert got.dtype == bool and got.shape == (9,)
    want = []
    for j in range(9):                                                       # each proof alone, under its own weights, by the trapdoor
        L, R, st = real.bv.fold([datas[j]], [pis[j]], [ws[j]])
        want.append(not st[0] and tv.tau_relation(real, L, R))
    assert got.tolist() == want == [j not in (0, 4, 8) for j in range(9)]
    st = real.pbv.prepare(datas, pis, ws)
    assert st[0] != 0 and not st[1:].any() and not got[0]                    # the proof with a status is False
    # the per-proof pairing inputs are the folds of the single-proof ranges
    xy_l, inf_l, xy_r, inf_r = real.pbv.pairing_inputs()
    for j in (1, 4):
        L, R = real.pbv.fold_range(j, j + 1)
        assert np.array_equal(xy_l[j].cpu().numpy().view(np.uint64), np.concatenate([L.x, L.y])) and not int(inf_l[j])
        assert np.array_equal(xy_r[j].cpu().numpy().view(np.uint64), np.concatenate([R.x, R.y])) and not int(inf_r[j])
    assert int(inf_l[0]) == 1 and int(inf_r[0]) == 1
    assert real.pbv.verdicts([], []).shape == (0,)
    assert real.pbv.verdicts(datas[1:4], pis[1:4]).tolist() == [True] * 3    # weights from the operating system
