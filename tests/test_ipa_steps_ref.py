"""tests/ipa_steps_ref.py -- the opening cut at the C ABI's seams, the checker of tests/test_ipa_steps_gpu.py -- against the whole
opening of tests/ipa_oracle.py, and the special challenges the GPU tests choose against what they claim.  Python integers only."""
import numpy as np
import pytest

import ipa_oracle as io
import ipa_steps_ref as sr
from oracle import bigint_oracle as bo
from test_ipa import make_instance

CURVES = {0: bo.BLS12_381, 1: bo.BN254}


@pytest.mark.parametrize("digest", ["blake2b", "blake2s"])
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("d1", [1, 2, 8, 64])
def test_steps_under_the_transcript_reproduce_the_opening(d1, cid, digest):
    cv = CURVES[cid]
    logs, k_h, polys, z, chi = make_instance(cv, d1, 3, 77 * d1 + 5 * cid + (digest == "blake2s"))
    KL = io.KnownLog(cv)
    comms = [io.commit(KL, logs, p) for p in polys]
    want = io.open_(KL, logs, k_h, polys, comms, z, chi, digest)
    assert sr.open_by_steps(KL, logs, k_h, polys, comms, z, chi, digest) == want
    assert len(want.l_vec) == d1.bit_length() - 1
    if d1 <= 8:
        G = (cv.gx, cv.gy)
        GE = io.Generic(cv)
        key = [bo.ec_mul(cv, k, G) for k in logs]
        h = bo.ec_mul(cv, k_h, G)
        comms_g = [io.commit(GE, key, p) for p in polys]
        assert io.open_(GE, key, h, polys, comms_g, z, chi, digest) == want
        assert sr.open_by_steps(GE, key, h, polys, comms_g, z, chi, digest) == want


@pytest.mark.parametrize("cid", [0, 1])
def test_b_is_any_vector_and_both_groups_agree_step_by_step(cid):
    """b random (no powers), a with a zero, chosen challenges: every L, R and the final key agree between logarithms and real points"""
    cv = CURVES[cid]
    r = cv.r
    logs, k_h, polys, z, chi = make_instance(cv, 8, 2, 900 + cid)
    a, b = polys
    a[3] = 0
    G = (cv.gx, cv.gy)
    xis = [r - 1, pow(2, -1, r), z]
    known = sr.Steps(io.KnownLog(cv)).walk(a, b, logs, k_h, lambda j, *_: xis[j])
    real = sr.Steps(io.Generic(cv)).walk(a, b, [bo.ec_mul(cv, k, G) for k in logs], bo.ec_mul(cv, k_h, G), lambda j, *_: xis[j])
    assert len(known) == len(real) == 3
    for (L1, R1, x1, a1, b1, k1), (L2, R2, x2, a2, b2, k2) in zip(known, real):
        assert (L1, R1, x1, a1, b1) == (L2, R2, x2, a2, b2)
        assert [bo.ec_mul(cv, k, G) for k in k1] == k2


@pytest.mark.parametrize("cid", [0, 1])
def test_powers_incl_zero_and_a_root_of_unity(cid):
    cv = CURVES[cid]
    r = cv.r
    st = sr.Steps(io.KnownLog(cv))
    assert st.powers(5, 0) == []
    assert st.powers(0, 4) == [1, 0, 0, 0]
    assert st.powers(1, 3) == [1, 1, 1]
    assert st.powers(r - 1, 4) == [1, r - 1, 1, r - 1]
    w = bo.CURVES[cid].root_of_unity(4)                     # a primitive 16th root of unity
    pw = st.powers(w, 17)
    assert pw == [pow(w, i, r) for i in range(17)] and pw[16] == 1 and pw[8] == r - 1 and len(set(pw[:16])) == 16


@pytest.mark.parametrize("cid", [0, 1])
def test_chosen_challenges_do_what_they_claim(cid):
    cv = CURVES[cid]
    r = cv.r
    logs, k_h, polys, z, chi = make_instance(cv, 16, 2, 31 + cid)
    a, b = polys
    st = sr.Steps(io.KnownLog(cv))
    m = 8
    for i in (0, 1, m - 1):
        kl, kr = logs[i], logs[i + m]
        xi = sr.xi_to_infinity(r, kl, kr)
        assert 0 < xi < r and xi == -kl * pow(kr, -1, r) % r
        key2 = st.fold(a, b, logs, xi)[2]
        assert key2[i] == 0 and io.KnownLog(cv).point(key2[i]) is None
        assert all(k != 0 for j, k in enumerate(key2) if j != i)
        xi = sr.xi_to_doubling(r, kl, kr)
        assert 0 < xi < r and xi * kr % r == kl
        key2 = st.fold(a, b, logs, xi)[2]
        assert key2[i] == 2 * kl % r
    # xi = 1, r - 1: the plain sum and difference of the halves; 2 and 2^-1 are each other's inverse on the a side
    a1, b1, k1 = st.fold(a, b, logs, 1)
    assert a1 == [(x + y) % r for x, y in zip(a[:m], a[m:])] and k1 == [(x + y) % r for x, y in zip(logs[:m], logs[m:])]
    a2, b2, k2 = st.fold(a, b, logs, r - 1)
    assert a2 == [(x - y) % r for x, y in zip(a[:m], a[m:])] and b2 == [(x - y) % r for x, y in zip(b[:m], b[m:])]
    a3, b3, k3 = st.fold(a, b, logs, pow(2, -1, r))
    assert a3 == [(x + 2 * y) % r for x, y in zip(a[:m], a[m:])] and [2 * x % r for x in k3] == [(2 * x + y) % r for x, y in zip(logs[:m], logs[m:])]
    with pytest.raises(AssertionError):
        st.fold(a, b, logs, 0)
    with pytest.raises(AssertionError):
        st.fold(a, b, logs, r)


@pytest.mark.parametrize("two_m", [2, 16])
@pytest.mark.parametrize("cid", [0, 1])
def test_short_first_round_is_the_walk_over_a_key_of_the_first_points(cid, two_m):
    cv = CURVES[cid]
    logs, k_h, polys, z, chi = make_instance(cv, 64, 2, 500 + cid + two_m)
    a, b = polys[0][:two_m], polys[1][:two_m]
    st = sr.Steps(io.KnownLog(cv))
    rng = np.random.default_rng(two_m)
    xis = [int.from_bytes(rng.bytes(40), "little") % cv.r for _ in range(6)]
    long_key = st.walk(a, b, logs, k_h, lambda j, *_: xis[j])
    short_key = st.walk(a, b, logs[:two_m], k_h, lambda j, *_: xis[j])
    assert long_key == short_key and len(long_key) == two_m.bit_length() - 1
    assert st.round_(a, b, logs, k_h) == st.round_(a, b, logs[:two_m], k_h)
    assert st.fold(a, b, logs, xis[0]) == st.fold(a, b, logs[:two_m], xis[0])
    # ... and differs from the walk over the key's LAST 2m points: the key does take part
    assert st.round_(a, b, logs[-two_m:], k_h) != st.round_(a, b, logs, k_h)
