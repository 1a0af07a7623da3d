"""The host pairing of csrc/pairing.hip (`ark_plonk_amd.pairing.PairingKey`), pinned to tests/golden/pairing_gt.json: values of the
reduced pairing by tests/pairing_ref.py, an independent definition on Python integers (one polynomial ring for Fq12, G2 untwisted
into E(Fq12), affine lines, a plain pow by (q^12 - 1) / r).  No GPU: the key preparation, `gt` and `check` run on the host."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ark_plonk_amd import _lib  # noqa: E402
from ark_plonk_amd.curves import fq_from_mont, fq_to_mont, g1_mul, g2_mul, get_curve  # noqa: E402
from ark_plonk_amd.msm import G1Affine  # noqa: E402
from ark_plonk_amd.pairing import GT_POWER, G2Affine, PairingKey  # noqa: E402
from tests import pairing_ref as pr  # noqa: E402
from tests.conftest import TAU  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "pairing_gt.json")
CURVES = ("bls12_381", "bn254")


def fixture(name):
    fx = json.load(open(FIXTURE))
    assert fx["tau"] == TAU
    return {(int(c["a"], 16), int(c["b"], 16)): [int(v, 16) for v in c["gt"]] for c in fx[name]["cases"]}


def g1(cv, k):
    """k G as a G1Affine (None: infinity)"""
    p = g1_mul(cv, k)
    if p is None:
        return None
    m = fq_to_mont(cv, list(p))
    return G1Affine(m[0], m[1], False, cv.name)


def g1_point(cv, pt):
    m = fq_to_mont(cv, list(pt))
    return G1Affine(m[0], m[1], False, cv.name)


def gt_poly(cv, rc, limbs):
    """a GT value of the library (12 x L Montgomery limbs, tower order) in the reference's polynomial basis"""
    return pr.tower_to_poly(rc, fq_from_mont(cv, np.asarray(limbs).reshape(12, cv.fq_limbs)))


_KEYS = {}


def key_of(name):
    if name not in _KEYS:
        _KEYS[name] = PairingKey.from_trapdoor(TAU, name)
    return _KEYS[name]


@pytest.mark.parametrize("name", CURVES)
def test_generators_and_fixture_are_what_the_reference_says(name):
    cv, rc = get_curve(name), pr.CURVES[name]
    assert (cv.g2x, cv.g2y) == rc.g2 and (cv.gx, cv.gy) == rc.g1 and (cv.q, cv.r) == (rc.q, rc.r)
    assert pr.on_twist(rc, rc.g2) and pr.g2_mul(rc, rc.r, reduce=False) is None
    for k in (1, 2, TAU, rc.r - 1):
        assert g2_mul(cv, k) == pr.g2_mul(rc, k)
    assert g2_mul(cv, rc.r) is None
    fx = fixture(name)
    assert {(1, 1), (1, TAU), (rc.r - 1, 1)} <= set(fx)
    assert fx[(1, 1)] == pr.ref_pairing(rc, rc.g1, rc.g2)              # the fixture is the reference's value (a fraction of a second)
    for (a, b), v in fx.items():
        assert v == pr.f_pow(rc, fx[(1, 1)], a * b % rc.r), (a, b)


@pytest.mark.parametrize("name", CURVES)
def test_published_power_matches_the_header(name):
    text = open(os.path.join(ROOT, "ark_plonk_amd", "csrc", "pairing.cuh")).read()
    macro = {"bls12_381": "ZK_PAIRING_GT_POWER_BLS12_381", "bn254": "ZK_PAIRING_GT_POWER_BN254"}[name]
    import re
    c = int(re.search(r"#define\s+" + macro + r"\s+(\d+)", text).group(1))
    assert c == GT_POWER[name] and c % get_curve(name).r != 0 and c in (1, 3)


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", CURVES)
def test_gt_equals_the_fixture_to_the_published_power(name, which):
    """PairingKey.gt(a G, which) in the polynomial basis == fixture ** c, bit for bit: which = 0 pairs with H, 1 with [tau]H"""
    cv, rc, key, c = get_curve(name), pr.CURVES[name], key_of(name), GT_POWER[name]
    fx = fixture(name)
    for (a, b), want in fx.items():
        if which == 0 and b == 1:
            assert gt_poly(cv, rc, key.gt(g1(cv, a), 0)) == pr.f_pow(rc, want, c), (a, b)
        if which == 1 and (a, b) == (1, TAU):
            assert gt_poly(cv, rc, key.gt(g1(cv, 1), 1)) == pr.f_pow(rc, want, c)
    if which == 1:                                                      # e(a G, [tau]H) = e(G, H)^(a tau), a = r - 1 too
        for a in (5, rc.r - 1):
            assert gt_poly(cv, rc, key.gt(g1(cv, a), 1)) == pr.f_pow(rc, fx[(1, 1)], a * TAU * c % rc.r), a


@pytest.mark.parametrize("name", CURVES)
def test_gt_with_other_g2_points(name):
    """a key over (b H, b' H) for the fixture's other b: the line tables of points that are not the generator"""
    cv, rc, c = get_curve(name), pr.CURVES[name], GT_POWER[name]
    fx = fixture(name)
    (a1, b1), (a2, b2) = [k for k in fx if k[1] not in (1, TAU)]
    key = PairingKey(G2Affine.from_ints(*g2_mul(cv, b1), cv), G2Affine.from_ints(*g2_mul(cv, b2), cv), cv)
    try:
        assert gt_poly(cv, rc, key.gt(g1(cv, a1), 0)) == pr.f_pow(rc, fx[(a1, b1)], c)
        assert gt_poly(cv, rc, key.gt(g1(cv, a2), 1)) == pr.f_pow(rc, fx[(a2, b2)], c)
    finally:
        key.close()


@pytest.mark.parametrize("name", CURVES)
def test_gt_of_infinity_is_one(name):
    cv, rc, key = get_curve(name), pr.CURVES[name], key_of(name)
    one = fq_to_mont(cv, [1]).reshape(-1)
    zero = np.zeros(cv.fq_limbs, dtype=np.uint64)
    for which in (0, 1):
        assert gt_poly(cv, rc, key.gt(None, which)) == pr.f_one()
        assert gt_poly(cv, rc, key.gt(G1Affine(zero, one, False, cv.name), which)) == pr.f_one()      # (0, 1) with no flag
        assert gt_poly(cv, rc, key.gt(G1Affine(zero, zero, False, cv.name), which)) == pr.f_one()     # (0, 0) with no flag
        got = key.gt(None, which)
        assert got[0].tolist() == one.tolist() and not got[1:].any()


@pytest.mark.parametrize("name", CURVES)
def test_gt_is_bilinear_through_the_library(name):
    cv, rc, key, c = get_curve(name), pr.CURVES[name], key_of(name), GT_POWER[name]
    a = int.from_bytes(os.urandom(32), "little") % rc.r or 1
    base = fixture(name)[(1, 1)]
    assert gt_poly(cv, rc, key.gt(g1(cv, a), 0)) == pr.f_pow(rc, base, a * c % rc.r), hex(a)


@pytest.mark.parametrize("name", CURVES)
def test_check_against_the_trapdoor(name):
    cv, key = get_curve(name), key_of(name)
    for k in (1, 12345, int.from_bytes(os.urandom(32), "little") % cv.r or 1, cv.r - 1):
        L = g1(cv, k)
        assert key.check(L, g1(cv, k * TAU)) is True, hex(k)
        assert key.check(L, g1(cv, k * TAU + 1)) is False, hex(k)
        assert key.check(L, g1(cv, -k * TAU)) is False, hex(k)
    G = g1(cv, 1)
    assert key.check(None, None) is True
    assert key.check(None, G) is False and key.check(G, None) is False
    inf = G1Affine(np.zeros(cv.fq_limbs, dtype=np.uint64), fq_to_mont(cv, [1]).reshape(-1), True, cv.name)
    assert key.check(inf, inf) is True and key.check(inf, G) is False


# ---- edge coordinates: tests/golden/pairing_edges.json (tests/golden/gen_pairing_edges.py), values of the independent reference at G1
# inputs whose coordinates are ends of Fq, its middle and 32/64-bit word boundaries, as values and as stored Montgomery words, and at
# off-curve extremes no curve point reaches -- the library's value is an algebraic function of (x, y), and so is the reference's
EDGE_FIXTURE = os.path.join(ROOT, "tests", "golden", "pairing_edges.json")
_EDGES = {}


def edge_fixture(name):
    """(points [(x, y, {0: gt with H, 1: gt with [tau]H}, on_curve)], checks [(L, R, valid, row)]) of one curve"""
    if not _EDGES:
        fx = json.load(open(EDGE_FIXTURE))
        assert fx["tau"] == TAU
        for c in CURVES:
            pts = [(int(p["x"], 16), int(p["y"], 16), {0: [int(v, 16) for v in p["gt_h"]], 1: [int(v, 16) for v in p["gt_tau_h"]]}, p["on_curve"])
                   for p in fx[c]["points"]]
            chk = [(tuple(int(v, 16) for v in r["L"]), tuple(int(v, 16) for v in r["R"]), r["valid"], r) for r in fx[c]["checks"]]
            _EDGES[c] = (pts, chk)
    return _EDGES[name]


def _edge_generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_pairing_edges", os.path.join(ROOT, "tests", "golden", "gen_pairing_edges.py"))
    mod = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    try:
        spec.loader.exec_module(mod)                     # a script: it puts tests/ in front of sys.path for its two imports
    finally:
        sys.path[:] = path
    return mod


@pytest.mark.parametrize("name", CURVES)
def test_edge_fixture_is_current(name):
    """the committed point list is the generator's, and three values and one verdict per curve are what the reference says today"""
    gen = _edge_generator()
    assert gen.TAU == TAU
    rc = pr.CURVES[name]
    pts, chk = edge_fixture(name)
    raw = json.load(open(EDGE_FIXTURE))[name]
    want = gen.point_list(gen.pr.CURVES[name])
    assert [(x, y, oc) for x, y, _, oc in pts] == [(x, y, oc) for x, y, _, oc in want]
    assert [p["what"] for p in raw["points"]] == [w for _, _, w, _ in want]
    assert len(pts) >= 30 and sum(oc for _, _, _, oc in pts) == len(pts) - 6 and len(chk) == 4 * (len(pts) - 6)
    if name == "bls12_381":
        assert (0, 2) in [(x, y) for x, y, _, _ in pts]
    tau_h = pr.g2_mul(rc, TAU)
    for i, which in ((0, 0), (len(pts) // 2, 1), (len(pts) - 1, 0)):        # the first, a middle one, the last (off the curve)
        x, y, gt, _ = pts[i]
        assert gt[which] == pr.ref_pairing(rc, (x, y), tau_h if which else rc.g2), (i, which)
    L, R, valid, row = chk[len(chk) // 8 * 4 + 2]                           # of a middle point, the "edge in R" case
    assert row["edge_in"] == "R" and not row["r_negated"]
    e = pr.f_mul(rc, pr.ref_pairing(rc, L, tau_h), pr.ref_pairing(rc, (R[0], -R[1] % rc.q), rc.g2))
    assert valid == (e == pr.f_one())
    if name == "bn254":
        assert all(v == (not r["r_negated"]) for _, _, v, r in chk)


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", CURVES)
def test_gt_at_edge_coordinates_equals_the_fixture(name, which):
    """PairingKey.gt at every fixture point, on or off the curve, == fixture ** c in the polynomial basis, bit for bit"""
    cv, rc, key, c = get_curve(name), pr.CURVES[name], key_of(name), GT_POWER[name]
    for i, (x, y, gt, _) in enumerate(edge_fixture(name)[0]):
        assert gt_poly(cv, rc, key.gt(g1_point(cv, (x, y)), which)) == pr.f_pow(rc, gt[which], c), (i, hex(x), hex(y))


@pytest.mark.parametrize("name", CURVES)
def test_check_at_edge_coordinates_equals_the_fixture(name):
    """PairingKey.check of every fixture case == the reference's verdict: edge coordinates in L, in R (whose y the check negates),
    and both with R.y replaced by q - R.y"""
    cv, key = get_curve(name), key_of(name)
    pts, chk = edge_fixture(name)
    assert any(v for _, _, v, _ in chk) and any(not v for _, _, v, _ in chk)
    for j, (L, R, valid, row) in enumerate(chk):
        assert key.check(g1_point(cv, L), g1_point(cv, R)) is valid, (j, row["point"], row["edge_in"], row["r_negated"])


# ---- unreduced G1 coordinates are a code on the host (include/ark_plonk_amd.h, the G1 paragraph of the pairing section)
def _unreduced(cv, limbs):
    """the same residue plus q where the sum fits the limbs, else q itself (the smallest unreduced value)"""
    L = cv.fq_limbs
    v = int.from_bytes(np.ascontiguousarray(limbs).tobytes(), "little") + cv.q
    if v >= 1 << (64 * L):
        v = cv.q
    return np.frombuffer(v.to_bytes(8 * L, "little"), dtype="<u8").copy()


@pytest.mark.parametrize("name", CURVES)
def test_unreduced_g1_coordinates_are_a_code(name):
    cv, key = get_curve(name), key_of(name)
    lib, bad, Ln = _lib.lib(), _lib.ZK_ERR_BAD_ARG, cv.fq_limbs
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)           # noqa: E731
    l = np.ascontiguousarray(g1(cv, 12345).xy(), dtype=np.uint64).reshape(-1).copy()
    r = np.ascontiguousarray(g1(cv, 12345 * TAU).xy(), dtype=np.uint64).reshape(-1).copy()
    ok = ctypes.c_int(7)
    assert lib.zk_kzg_pairing_check(key._h, p(l), 0, p(r), 0, ctypes.byref(ok)) == _lib.ZK_OK and ok.value == 1
    q_limbs = np.frombuffer(cv.q.to_bytes(8 * Ln, "little"), dtype="<u8").copy()
    one = fq_to_mont(cv, [1]).reshape(-1)
    for k in range(4):                                         # L.x, L.y, R.x, R.y
        pts = [l.copy(), r.copy()]
        pts[k // 2][(k % 2) * Ln:(k % 2 + 1) * Ln] = _unreduced(cv, pts[k // 2][(k % 2) * Ln:(k % 2 + 1) * Ln])
        ok = ctypes.c_int(7)
        assert lib.zk_kzg_pairing_check(key._h, p(pts[0]), 0, p(pts[1]), 0, ctypes.byref(ok)) == bad, k
        assert ok.value == 7, k                                # untouched
        with pytest.raises(_lib.ZkError) as e:
            key.check(G1Affine(pts[0][:Ln], pts[0][Ln:], False, cv.name), G1Affine(pts[1][:Ln], pts[1][Ln:], False, cv.name))
        assert e.value.code == bad
        if k < 2:
            for which in (0, 1):
                out = np.full((12, Ln), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
                assert lib.zk_pairing_gt(key._h, which, p(pts[0]), 0, p(out)) == bad, (k, which)
                assert (out == 0x5A5A5A5A5A5A5A5A).all()
            # ... and a point passed with its infinity flag is not inspected
            ok = ctypes.c_int(7)
            assert lib.zk_kzg_pairing_check(key._h, p(pts[0]), 1, p(r), 1, ctypes.byref(ok)) == _lib.ZK_OK and ok.value == 1
    # the unreduced spellings of the encodings of infinity: (q, one) and (q, q) without a flag
    for y in (one, q_limbs):
        spelled = np.concatenate([q_limbs, y])
        for args in ((spelled, r), (l, spelled), (spelled, spelled)):
            ok = ctypes.c_int(7)
            assert lib.zk_kzg_pairing_check(key._h, p(args[0]), 0, p(args[1]), 0, ctypes.byref(ok)) == bad and ok.value == 7
        out = np.zeros((12, Ln), dtype=np.uint64)
        assert lib.zk_pairing_gt(key._h, 0, p(spelled), 0, p(out)) == bad and not out.any()
        ok = ctypes.c_int(7)
        assert lib.zk_kzg_pairing_check(key._h, p(spelled), 1, p(spelled), 1, ctypes.byref(ok)) == _lib.ZK_OK and ok.value == 1
    # the largest reduced values pass the test (and are decided, whatever the verdict)
    top = np.frombuffer((cv.q - 1).to_bytes(8 * Ln, "little"), dtype="<u8").copy()
    ok = ctypes.c_int(7)
    assert lib.zk_kzg_pairing_check(key._h, p(np.concatenate([top, top])), 0, p(r), 0, ctypes.byref(ok)) == _lib.ZK_OK and ok.value == 0


def _key_new(cid, h, tau_h):
    out = ctypes.c_void_p()
    rc = _lib.lib().zk_pairing_key_new(cid, None if h is None else h.ctypes.data_as(ctypes.c_void_p),
                                       None if tau_h is None else tau_h.ctypes.data_as(ctypes.c_void_p), ctypes.byref(out))
    if rc == _lib.ZK_OK:
        _lib.lib().zk_pairing_key_free(out)
    else:
        assert out.value is None
    return rc


@pytest.mark.parametrize("name", CURVES)
def test_key_validation(name):
    cv, rc = get_curve(name), pr.CURVES[name]
    L = cv.fq_limbs
    good = G2Affine.from_ints(cv.g2x, cv.g2y, cv).limbs()
    other = G2Affine.from_ints(*g2_mul(cv, TAU), cv).limbs()
    assert _key_new(cv.curve_id, good, other) == _lib.ZK_OK
    bad = _lib.ZK_ERR_BAD_ARG
    # a point off the twist: y + 1; the encodings of infinity
    off = G2Affine.from_ints(cv.g2x, ((cv.g2y[0] + 1) % cv.q, cv.g2y[1]), cv).limbs()
    assert not pr.on_twist(rc, (cv.g2x, ((cv.g2y[0] + 1) % cv.q, cv.g2y[1])))
    zero_one = G2Affine.from_ints((0, 0), (1, 0), cv).limbs()
    for pt in (off, zero_one, np.zeros(4 * L, dtype=np.uint64)):
        assert _key_new(cv.curve_id, pt, other) == bad and _key_new(cv.curve_id, good, pt) == bad
    # a point of the twist outside the r-torsion
    out = pr.first_twist_point_outside_g2(rc)
    assert pr.on_twist(rc, out) and pr.g2_mul(rc, rc.r, out, reduce=False) is not None
    outside = G2Affine.from_ints(out[0], out[1], cv).limbs()
    assert _key_new(cv.curve_id, outside, other) == bad and _key_new(cv.curve_id, good, outside) == bad
    # an unreduced coordinate: the same residue plus q, in each of the four places
    q_limbs = np.frombuffer(cv.q.to_bytes(8 * L, "little"), dtype="<u8")
    for k in range(4):
        un = good.copy()
        v = int.from_bytes(un[k * L:(k + 1) * L].tobytes(), "little") + cv.q
        if v >= 1 << (64 * L):
            un[k * L:(k + 1) * L] = q_limbs                           # the modulus itself: the smallest unreduced value
        else:
            un[k * L:(k + 1) * L] = np.frombuffer(v.to_bytes(8 * L, "little"), dtype="<u8")
        assert _key_new(cv.curve_id, un, other) == bad, k
    # null pointers, an unknown curve
    assert _key_new(cv.curve_id, None, other) == bad and _key_new(cv.curve_id, good, None) == bad
    assert _lib.lib().zk_pairing_key_new(cv.curve_id, good.ctypes.data_as(ctypes.c_void_p), other.ctypes.data_as(ctypes.c_void_p), None) == bad
    assert _key_new(7, good, other) == bad and _key_new(-1, good, other) == bad
    with pytest.raises(_lib.ZkError) as e:
        PairingKey(G2Affine(off[:2 * L], off[2 * L:], cv), G2Affine(other[:2 * L], other[2 * L:], cv), cv)
    assert e.value.code == bad


def test_null_key_and_null_points_are_codes():
    lib = _lib.lib()
    bad = _lib.ZK_ERR_BAD_ARG
    key = key_of("bn254")
    buf = np.zeros(48, dtype=np.uint64)
    ok = ctypes.c_int(0)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.zk_kzg_pairing_check(None, p, 0, p, 0, ctypes.byref(ok)) == bad
    assert lib.zk_kzg_pairing_check(key._h, None, 0, p, 0, ctypes.byref(ok)) == bad
    assert lib.zk_kzg_pairing_check(key._h, p, 0, None, 0, ctypes.byref(ok)) == bad
    assert lib.zk_kzg_pairing_check(key._h, p, 0, p, 0, None) == bad
    assert lib.zk_pairing_gt(None, 0, p, 0, p) == bad and lib.zk_pairing_gt(key._h, 2, p, 0, p) == bad
    assert lib.zk_pairing_gt(key._h, 0, None, 0, p) == bad and lib.zk_pairing_gt(key._h, 0, p, 0, None) == bad
    assert lib.zk_kzg_pairing_check_batch_dev(None, key._h, p, None, p, None, 1, p) == bad
    assert lib.zk_pairing_gt_batch_dev(None, key._h, 0, p, None, 1, p) == bad
    lib.zk_pairing_key_free(None)


def test_batch_verifier_without_a_key_says_so():
    """`verify` and `verdicts` need a key, and `locate_invalid` needs a key or the caller's check: a ValueError before any GPU work"""
    from ark_plonk_amd.verifier import BatchVerifier
    bv = BatchVerifier.__new__(BatchVerifier)
    bv.pairing_key, bv._res, bv._key_ck = None, None, None
    for call in (lambda: bv.verify([]), lambda: bv.verdicts([]), lambda: bv.locate_invalid([], None)):
        with pytest.raises(ValueError):
            call()


def test_generated_constants_are_current():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_pairing_constants.py")], capture_output=True, text=True, check=True)
    assert out.stdout == open(os.path.join(ROOT, "ark_plonk_amd", "csrc", "pairing_params.h")).read()
