"""CPU checks of tests/large_ref.py, the vectorised references of the large-size GPU tests, against the big-integer restatement
(oracle/bigint_oracle.py) at small sizes."""
import numpy as np
import pytest

import large_ref as lr
from oracle import bigint_oracle as bo


def _ints(a):
    return [sum(int(row[k]) << (64 * k) for k in range(4)) for row in np.asarray(a, dtype=np.uint64)]


def _from_mont(oracle_cpu, cid, a):
    return oracle_cpu.limbs_to_ints(oracle_cpu.convert(cid, "fr", False, a))


@pytest.mark.parametrize("cid", [0, 1])
def test_full_range_covers_the_field(cid):
    r = bo.CURVES[cid].r
    a = lr.full_range(cid, 1 << 16, 3)
    v = _ints(a)
    assert a.shape == (1 << 16, 4) and a.dtype == np.uint64 and lr.is_canonical(cid, a)
    assert all(0 <= x < r for x in v)
    assert max(v) > r - (r >> 10) and min(v) < r >> 10             # both ends of [0, r) are reached
    assert sum(x >= r // 2 for x in v) > 0.48 * len(v)               # the top half as often as the bottom one
    assert np.array_equal(a, lr.full_range(cid, 1 << 16, 3)) and not np.array_equal(a, lr.full_range(cid, 1 << 16, 4))
    # the redraw path: rows with top limb r_3 are kept only below r
    rl = lr.r_limbs(cid)
    b = np.tile(rl, (4, 1))
    assert not lr._lt(b, rl).any() and lr._lt(b - np.array([1, 0, 0, 0], dtype=np.uint64), rl).all()


@pytest.mark.parametrize("cid", [0, 1])
def test_near_r_and_r_minus_one(cid):
    r = bo.CURVES[cid].r
    v = _ints(lr.near_r(cid, 4096, 9))
    assert all(r - (1 << 64) <= x < r for x in v) and len(set(v)) == 4096
    assert lr.is_canonical(cid, lr.near_r(cid, 4096, 9))
    assert _ints(lr.r_minus_one(cid, 3)) == [r - 1] * 3
    assert not lr.is_canonical(cid, lr.r_limbs(cid))


@pytest.mark.parametrize("cid", [0, 1])
def test_powers(cid, oracle_cpu):
    cv = bo.CURVES[cid]
    w = cv.root_of_unity(7)
    for n in (0, 1, 2, 5, 128, 200):
        got = _from_mont(oracle_cpu, cid, lr.powers(oracle_cpu, cid, w, n))
        assert got == [pow(w, i, cv.r) for i in range(n)]


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("kind", [bo.KIND_FFT, bo.KIND_COSET_FFT])
def test_decimation_identity(cid, kind, oracle_cpu):
    cv = bo.CURVES[cid]
    log_n, log_m = 7, 4
    x = lr.full_range(cid, 13, 70 + kind)
    full = _from_mont(oracle_cpu, cid, oracle_cpu.ntt(cid, kind, log_n, x))
    assert full == bo.ntt(cv, kind, log_n, _from_mont(oracle_cpu, cid, x))
    s = 1 << (log_n - log_m)
    for t in range(s):
        assert _from_mont(oracle_cpu, cid, lr.decimated(oracle_cpu, cid, kind, log_n, log_m, x, t)) == full[t::s], t


@pytest.mark.parametrize("cid", [0, 1])
def test_grand_product_terms(cid, oracle_cpu):
    cv = bo.CURVES[cid]
    log_n = 6
    n = 1 << log_n
    cols = [lr.full_range(cid, n, 600 + k) for k in range(8)]
    cols[1][:4] = lr.r_minus_one(cid, 4)
    ints = [_from_mont(oracle_cpu, cid, c) for c in cols]
    beta, gamma = lr.full_range(cid, 2, 610)
    ez, elast = bo.perm_product(cv, log_n, ints[:4], ints[4:], *_from_mont(oracle_cpu, cid, np.stack([beta, gamma])))
    num, den = lr.perm_terms(oracle_cpu, cid, log_n, cols[:4], cols[4:], beta, gamma)
    z, last = lr.mont(oracle_cpu, cid, ez), lr.mont(oracle_cpu, cid, [elast])[0]
    assert lr.check_product(oracle_cpu, cid, z, last, num, den) is None
    bad = z.copy()
    bad[37, 0] ^= np.uint64(1 << 9)
    assert lr.check_product(oracle_cpu, cid, bad, last, num, den) == 36
    assert lr.check_product(oracle_cpu, cid, z, lr.mont(oracle_cpu, cid, [elast + 1])[0], num, den) == n - 1
    unreduced = z.copy()
    unreduced[5] = lr.r_limbs(cid)
    with pytest.raises(AssertionError):
        lr.check_product(oracle_cpu, cid, unreduced, last, num, den)
    delta, eps = lr.full_range(cid, 2, 620)
    ep, elastp = bo.lookup_product(cv, *ints[:4], *_from_mont(oracle_cpu, cid, np.stack([delta, eps])))
    num, den = lr.lookup_terms(oracle_cpu, cid, *cols[:4], delta, eps)
    p, lastp = lr.mont(oracle_cpu, cid, ep), lr.mont(oracle_cpu, cid, [elastp])[0]
    assert lr.check_product(oracle_cpu, cid, p, lastp, num, den) is None
    assert lr.check_product(oracle_cpu, cid, p, p[0], num, den) == n - 1


@pytest.mark.parametrize("cid", [0, 1])
def test_witnesses_and_evaluations(cid, oracle_cpu):
    cv = bo.CURVES[cid]
    polys = [lr.full_range(cid, ln, 90 + ln) for ln in (1, 2, 50)]
    zs = [lr.full_range(cid, 1, 80)[0], lr.mont(oracle_cpu, cid, [0])[0], lr.r_minus_one(cid, 1)[0]]
    jobs = [(p, z) for p in polys for z in zs]
    ws = lr.witnesses(oracle_cpu, cid, jobs)
    evs = lr.evaluations(oracle_cpu, cid, jobs)
    for (p, z), w, e in zip(jobs, ws, evs):
        pi, zi = _from_mont(oracle_cpu, cid, p), _from_mont(oracle_cpu, cid, z.reshape(1, 4))[0]
        assert _from_mont(oracle_cpu, cid, e.reshape(1, 4))[0] == bo.horner(pi, zi, cv.r)
        assert w.shape[0] == p.shape[0] - 1
        # p(X) - p(z) = (X - z) w(X): compare at a second point
        x = 12345
        assert (bo.horner(pi, x, cv.r) - bo.horner(pi, zi, cv.r)) % cv.r == \
            (x - zi) * bo.horner(_from_mont(oracle_cpu, cid, w) if w.shape[0] else [], x, cv.r) % cv.r
