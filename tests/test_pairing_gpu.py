"""The device side of the pairing check (csrc/pairing.hip: one check per lane) against the host side, which tests/test_pairing.py pins
to an independent pairing; against that independent pairing directly, at G1 inputs whose coordinates are base-field edges
(tests/golden/pairing_edges.json: the device build of the tower is not the host build); on more wavefronts than the card holds at
once; and `BatchVerifier`'s yes / no answers on real proofs against the trapdoor relation tau L == R that the other verifier tests
use in the pairing's place."""
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
from ark_plonk_amd.curves import fq_from_mont, g2_mul  # noqa: E402
from ark_plonk_amd.pairing import GT_POWER, G2Affine, PairingKey  # noqa: E402
from tests import pairing_ref as pr  # noqa: E402
from tests import test_pairing as tp  # noqa: E402
from tests.conftest import TAU  # noqa: E402
from tests.test_pairing_resources import WAVES_PER_SIMD  # noqa: E402

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


# ------------------------------------------------------------------------------------------------------------------ edge coordinates
def point_limbs(cv, pts):
    """(x, y) integer pairs -> (n, 2L) uint64 Montgomery words"""
    return np.stack([fq_to_mont(cv, list(p)).reshape(-1) for p in pts])


_WANT = {}


def edge_want(name, which):
    """fixture ** GT_POWER of every edge point, in the reference's polynomial basis: what a lane must hold"""
    if (name, which) not in _WANT:
        rc, c = pr.CURVES[name], GT_POWER[name]
        _WANT[(name, which)] = [pr.f_pow(rc, gt[which], c) for _, _, gt, _ in tp.edge_fixture(name)[0]]
    return _WANT[(name, which)]


def lane_poly(cv, rc, lane):
    return pr.tower_to_poly(rc, fq_from_mont(cv, lane.reshape(12, cv.fq_limbs)))


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", CURVES)
def test_gt_batch_at_edge_coordinates_equals_the_fixture(name, which, keys, ctx):
    """every edge point of the fixture, on or off the curve, through the device kernel: compared with the independent reference, not
    with the host.  Twice: in list order; and reversed, followed by the list rotated by five (the fixture has fewer than 64 points,
    so that lanes 63 and 64 exist), with infinity lanes -- flagged, and as (0, 1) / (0, 0) without a flag -- at 0, 63, 64 and last:
    every point in two other lanes, some beside skipped ones."""
    cv, rc = get_curve(name), pr.CURVES[name]
    L = cv.fq_limbs
    pts = [(x, y) for x, y, _, _ in tp.edge_fixture(name)[0]]
    want = edge_want(name, which)
    m = len(pts)
    xy = point_limbs(cv, pts)
    got = keys[name].gt_batch(to_dev(xy, ctx), to_dev(np.zeros(m, dtype=np.uint8), ctx), which, ctx).cpu().numpy().view(np.uint64)
    for i in range(m):
        assert lane_poly(cv, rc, got[i]) == want[i], (i, hex(pts[i][0]), hex(pts[i][1]))
    order = list(range(m))[::-1] + [(i + 5) % m for i in range(m)]
    one = fq_to_mont(cv, [1]).reshape(-1)
    zero_one, zero_zero = np.concatenate([np.zeros(L, dtype=np.uint64), one]), np.zeros(2 * L, dtype=np.uint64)
    lanes = [(xy[i], 0, i) for i in order]
    lanes.insert(0, (xy[3], 1, None))                       # a flag over a finite point's words
    lanes.insert(63, (zero_one, 0, None))
    lanes.insert(64, (zero_zero, 0, None))
    lanes.append((zero_one, 1, None))
    assert len(lanes) > 65 and [k for k, l in enumerate(lanes) if l[2] is None] == [0, 63, 64, len(lanes) - 1]
    bxy, binf = np.stack([l[0] for l in lanes]), np.array([l[1] for l in lanes], dtype=np.uint8)
    got = keys[name].gt_batch(to_dev(bxy, ctx), to_dev(binf, ctx), which, ctx).cpu().numpy().view(np.uint64)
    for k, (_, _, i) in enumerate(lanes):
        assert lane_poly(cv, rc, got[k]) == (pr.f_one() if i is None else want[i]), (k, i)


@pytest.mark.parametrize("name", CURVES)
def test_check_batch_at_edge_coordinates_equals_the_fixture(name, keys, ctx):
    """the fixture's check cases in one launch, valid and invalid interleaved as the fixture lists them: edge coordinates in L, in R
    (whose y the kernel negates), and both with R.y replaced by q - R.y; the verdicts are the reference's"""
    cv = get_curve(name)
    L = cv.fq_limbs
    chk = tp.edge_fixture(name)[1]
    want = [int(v) for _, _, v, _ in chk]
    assert len(chk) > 65 and sum(a != b for a, b in zip(want, want[1:])) > len(want) // 2      # interleaved
    lxy, rxy = point_limbs(cv, [c[0] for c in chk]), point_limbs(cv, [c[1] for c in chk])
    ok = keys[name].check_batch(to_dev(lxy, ctx), None, to_dev(rxy, ctx), None, ctx).cpu().numpy()
    assert ok.tolist() == want
    for i in (0, 1, 2, 3, 63, 64, len(chk) - 1):                             # ... and the host check says the same
        assert keys[name].check(zk.G1Affine(lxy[i, :L], lxy[i, L:], False, cv.name), zk.G1Affine(rxy[i, :L], rxy[i, L:], False, cv.name)) \
            == bool(want[i]), i


@pytest.mark.parametrize("name", CURVES)
def test_a_device_key_over_other_g2_points(name, ctx):
    """the (b1 H, b2 H) key of test_pairing.test_gt_with_other_g2_points on the device: line tables of points that are neither the
    generator nor [tau]H, against pairing_gt.json and the relation b2 L == b1 R"""
    cv, rc, c = get_curve(name), pr.CURVES[name], GT_POWER[name]
    fx = tp.fixture(name)
    (a1, b1), (a2, b2) = [k for k in fx if k[1] not in (1, TAU)]
    key = PairingKey(G2Affine.from_ints(*g2_mul(cv, b1), cv), G2Affine.from_ints(*g2_mul(cv, b2), cv), cv)
    try:
        xy, inf = scalar_points(cv, [a1, a2])
        for which, (i, (a, b)) in ((0, (0, (a1, b1))), (1, (1, (a2, b2)))):
            got = key.gt_batch(to_dev(xy, ctx), to_dev(inf, ctx), which, ctx).cpu().numpy().view(np.uint64)
            assert lane_poly(cv, rc, got[i]) == pr.f_pow(rc, fx[(a, b)], c), (which, hex(a), hex(b))
        # e(L, b2 H) e(-R, b1 H) == 1  <=>  b2 L == b1 R
        k = 0xC0FFEE
        ls = [b1 * k, b1 * k, b1 * k, 0, k, a1, b1, 0]
        rs = [b2 * k, b2 * k + 1, -b2 * k, 0, k * b2 * pow(b1, -1, cv.r), a2, b2, k]
        want = [int(b2 * l % cv.r == b1 * r % cv.r) for l, r in zip(ls, rs)]
        assert want == [1, 0, 0, 1, 1, 0, 1, 0]
        lxy, linf = scalar_points(cv, ls)
        rxy, rinf = scalar_points(cv, rs)
        ok = key.check_batch(to_dev(lxy, ctx), to_dev(linf, ctx), to_dev(rxy, ctx), to_dev(rinf, ctx), ctx).cpu().numpy()
        assert ok.tolist() == want
    finally:
        key.close()


@pytest.mark.parametrize("name", CURVES)
def test_views_with_a_storage_offset_give_the_same_lanes(name, keys, ctx):
    """rows [1:] of a larger contiguous tensor, for points and for flags: the kernels get the view's address, not the storage's"""
    import torch
    cv = get_curve(name)
    ks = [0, 5, 0xDEADBEEF, cv.r - 1, 0, 2, 7 * TAU]
    lxy, linf = scalar_points(cv, ks)
    rxy, rinf = scalar_points(cv, [k * TAU if i != 2 else 1 for i, k in enumerate(ks)])
    big = [to_dev(a, ctx) for a in (lxy, linf, rxy, rinf)]
    views = [t[1:] for t in big]
    assert all(v.storage_offset() != 0 and v.is_contiguous() for v in views)
    fresh = [v.clone() for v in views]
    assert all(f.storage_offset() == 0 for f in fresh)
    for which in (0, 1):
        a, b = keys[name].gt_batch(views[0], views[1], which, ctx), keys[name].gt_batch(fresh[0], fresh[1], which, ctx)
        assert torch.equal(a, b)
    a, b = keys[name].check_batch(*views, ctx), keys[name].check_batch(*fresh, ctx)
    assert torch.equal(a, b) and a.cpu().tolist() == [1, 0, 1, 1, 1, 1]
    host = keys[name].gt(zk.G1Affine(lxy[1, :cv.fq_limbs], lxy[1, cv.fq_limbs:], False, cv.name), 1)
    assert np.array_equal(keys[name].gt_batch(views[0], views[1], 1, ctx)[0].cpu().numpy().view(np.uint64), host)


# More wavefronts than the card holds at once: a workgroup is one wavefront, a CU has 4 SIMDs, and a SIMD holds WAVES_PER_SIMD (= 1:
# 512 // vgpr_count, tests/test_pairing_resources.py) wavefronts of these kernels, so 64 * 4 * CUs * WAVES_PER_SIMD lanes are resident
# and the per-lane scratch slots of the running Fq12 values are reused by whatever comes after.  MANY_WAVES_FACTOR = 2 is the factor
# the batch is sized with: two full rounds of the card and one more lane (131073 lanes on 256 CUs; times in profiles/pairing/notes.md).
MANY_WAVES_FACTOR = 2
MANY_WAVES_POOL = 9                        # the cycle length of the inputs: coprime to 64, so a pool entry meets every lane index


def many_waves_n(ctx):
    import torch
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    return MANY_WAVES_FACTOR * 64 * 4 * cus * WAVES_PER_SIMD + 1


def pool_points(name):
    """nine inputs of gt_batch: six edge points of the fixture (an end of the field as a value and as a stored word, (0, 2) or its
    neighbour, two off-curve extremes) and infinity three ways -> (xy, flags, fixture index or None)"""
    cv = get_curve(name)
    L = cv.fq_limbs
    pts = tp.edge_fixture(name)[0]
    m = len(pts)
    idx = [0, 4, m // 2, m - 7, m - 6, m - 1]
    xy = point_limbs(cv, [(pts[i][0], pts[i][1]) for i in idx])
    one = fq_to_mont(cv, [1]).reshape(-1)
    zero_one, zero_zero = np.concatenate([np.zeros(L, dtype=np.uint64), one]), np.zeros(2 * L, dtype=np.uint64)
    rows = [xy[0], zero_one, xy[1], xy[2], xy[3], xy[3], zero_zero, xy[4], xy[5]]
    flags = np.array([0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=np.uint8)
    assert len(rows) == MANY_WAVES_POOL and np.gcd(MANY_WAVES_POOL, 64) == 1
    return np.stack(rows), flags, [idx[0], None, idx[1], idx[2], idx[3], None, None, idx[4], idx[5]]


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", CURVES)
def test_gt_batch_on_more_waves_than_the_card_holds(name, which, keys, ctx):
    import torch
    cv, rc = get_curve(name), pr.CURVES[name]
    n = many_waves_n(ctx)
    xy, flags, src = pool_points(name)
    d_xy, d_flags = to_dev(xy, ctx), to_dev(flags, ctx)
    pool = keys[name].gt_batch(d_xy, d_flags, which, ctx)
    want = edge_want(name, which)
    host = pool.cpu().numpy().view(np.uint64)
    for j, i in enumerate(src):                                              # the pool's values are the fixture's
        assert lane_poly(cv, rc, host[j]) == (pr.f_one() if i is None else want[i]), j
    lane = torch.arange(n, device=d_xy.device) % MANY_WAVES_POOL
    got = keys[name].gt_batch(d_xy[lane].contiguous(), d_flags[lane].contiguous(), which, ctx)
    assert got.shape == (n, 12, cv.fq_limbs) and torch.equal(got, pool[lane])


@pytest.mark.parametrize("name", CURVES)
def test_check_batch_on_more_waves_than_the_card_holds(name, keys, ctx):
    import torch
    cv = get_curve(name)
    L = cv.fq_limbs
    n = many_waves_n(ctx)
    chk = tp.edge_fixture(name)[1]
    m = len(chk)
    mid = m // 8 * 4                                                         # a middle point's four cases, the first point's first two
    picks = [mid, mid + 1, mid + 2, mid + 3, 0, 1, m - 2]                    # (on BLS12-381: of order 3, valid either way), the last point
    lxy, rxy = point_limbs(cv, [chk[i][0] for i in picks]), point_limbs(cv, [chk[i][1] for i in picks])
    one = fq_to_mont(cv, [1]).reshape(-1)
    zero_one = np.concatenate([np.zeros(L, dtype=np.uint64), one])[None]
    lxy, rxy = np.concatenate([lxy, zero_one, zero_one]), np.concatenate([rxy, zero_one, rxy[:1]])      # both infinity; only L
    want = [int(chk[i][2]) for i in picks] + [1, 0]
    assert len(want) == MANY_WAVES_POOL and 0 < sum(want) < len(want)
    d_l, d_r = to_dev(lxy, ctx), to_dev(rxy, ctx)
    pool = keys[name].check_batch(d_l, None, d_r, None, ctx)
    assert pool.cpu().tolist() == want                                       # the pool's verdicts are the reference's
    lane = torch.arange(n, device=d_l.device) % MANY_WAVES_POOL
    got = keys[name].check_batch(d_l[lane].contiguous(), None, d_r[lane].contiguous(), None, ctx)
    assert got.shape == (n,) and torch.equal(got, pool[lane])


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
