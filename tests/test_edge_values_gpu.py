"""The scalar-field kernels on the inputs uniform sampling never draws (tests/edge_values.py): the ends of the field, limb and word
boundaries, and the stored words at which the load conversion of the quotient kernel changes its quotient estimate -- the quotient,
both grand products, the lookup compression and the KZG evaluation / opening, every output against oracle/bigint_oracle.py."""
import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import linearisation, lookup, permutation, quotient
from ark_plonk_amd.curves import fr_from_mont, fr_to_mont
from oracle import bigint_oracle as bo
from tests import edge_values as ev
from tests.conftest import TAU, srs_from_powers, tau_powers

pytestmark = pytest.mark.gpu

COL = {"q_fixed": "q_fixed_group_add", "q_var": "q_variable_group_add"}
CH = {"range": "range_challenge", "logic": "logic_challenge", "fixed": "fixed_base_challenge", "var": "var_base_challenge",
      "lookup": "lookup_challenge"}
STRIDES = (1, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107)


def dev(cid, ints):
    import torch
    a = fr_to_mont(cid, ints) if len(ints) else np.zeros((0, 4), dtype=np.uint64)
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 4)).cuda()


def m1(cid, x):
    return fr_to_mont(cid, [x])[0]


def back(cid, t):
    return fr_from_mont(cid, t.cpu().numpy().view(np.uint64).reshape(-1, 4)) if t.shape[0] else []


def special(cv, seed, k):
    """k challenges cycling through 0, 1, r - 1 and a seeded value, starting at another one for every seed"""
    rnd = bo.seeded_scalars(cv, 0xED00 + seed, k)
    return [(0, 1, cv.r - 1, rnd[j])[(j + seed) % 4] for j in range(k)]


# ---------------------------------------------------------------------------------------------------------------- quotient
def quotient_case(cv, log_n, fill, shift):
    n4 = 4 << log_n
    if fill == "edges":                 # every column the edge set, another stride and start per column
        col = {name: ev.edge_column(cv, n4, STRIDES[k], 5 * k) for k, name in enumerate(bo.QUOTIENT_COLS)}
    elif fill == "minus_one":
        col = {name: [cv.r - 1] * n4 for name in bo.QUOTIENT_COLS}
    else:                               # zero but the selectors
        col = {name: ev.edge_column(cv, n4, STRIDES[k], 5 * k) if name.startswith("q_") else [0] * n4 for k, name in enumerate(bo.QUOTIENT_COLS)}
    ch = dict(zip(bo.QUOTIENT_CHALLENGES, special(cv, shift, len(bo.QUOTIENT_CHALLENGES))))
    return col, ch


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("log_n", [3, 6])
@pytest.mark.parametrize("fill", ["edges", "minus_one", "selectors_only"])
def test_quotient_every_point(cid, log_n, fill, ctx):
    """All 4n points, with every challenge at 0, 1, r - 1 and a seeded value in turn (four runs)."""
    cv = bo.CURVES[cid]
    dom = zk.Radix2EvaluationDomain.new(1 << log_n, cid, ctx)
    for shift in range(4):
        col, ch = quotient_case(cv, log_n, fill, shift)
        d = {k: dev(cid, v) for k, v in col.items()}
        got = quotient.compute_quotient_evals(dom, {COL.get(k, k): v for k, v in d.items() if not k.startswith("sigma")},
                                              [d[f"sigma{k}"] for k in range(4)], {CH.get(k, k): m1(cid, v) for k, v in ch.items()})
        want = bo.quotient_evals(cv, log_n, col, ch)
        got = back(cid, got)
        bad = [i for i in range(len(want)) if got[i] != want[i]]
        assert not bad, (shift, bad[:8])


# ---------------------------------------------------------------------------------------------------------------- grand products
def perm_case(cv, log_n, which):
    """edge wires, seeded sigma columns (an edge sigma makes w + beta sigma + gamma = 0 an accident of the pairing, which is the
    error case of test_grand_product_gpu.py, not this one)"""
    n = 1 << log_n
    s1, s2 = bo.seeded_scalars(cv, 0xEA00 + log_n, 2)
    beta, gamma = ((1, cv.r - 1), (cv.r - 1, s1), (s2, 1), (cv.r - 1, cv.r - 1))[which]
    wires = [ev.edge_column(cv, n, STRIDES[k + which], 9 * k + 4) for k in range(4)]
    sigmas = [bo.seeded_scalars(cv, 0xEA10 + 4 * log_n + k, n) for k in range(4)]
    return wires, sigmas, beta, gamma


def lookup_case(cv, n, which):
    """f, t and h1 from the edge set, h2 seeded (as above: the denominators stay non-zero).  delta = r - 1 makes 1 + delta and so every
    numerator zero; epsilon = 1 or r - 1 zeroes the numerator of the rows with f = -epsilon, which the edge column holds once per turn
    of the edge set.  The argument is cyclic in its rows, so the four columns are turned together until the longest run of non-zero
    numerators starts at row 0: the values before the first zero are what the comparison is about."""
    p = cv.r
    s1, s2 = bo.seeded_scalars(cv, 0xEB00 + n, 2)
    delta, eps = ((1, s1), (p - 1, s1), (s2, 1), (s2, p - 1))[which]
    f, t, h1 = (ev.edge_column(cv, n, STRIDES[k + 2 * which], 7 * k) for k in range(3))
    h2 = bo.seeded_scalars(cv, 0xEB10 + which, n)
    e1d = eps * (1 + delta) % p
    zero = [i for i in range(n) if (eps + f[i]) % p == 0 or (e1d + t[i] + delta * t[(i + 1) % n]) % p == 0]
    if zero and len(zero) < n:
        gap, turn = max(((zero[(j + 1) % len(zero)] - z - 1) % n, (z + 1) % n) for j, z in enumerate(zero))
        f, t, h1, h2 = (c[turn:] + c[:turn] for c in (f, t, h1, h2))
    return f, t, h1, h2, delta, eps


def run_perm(cid, log_n, wires, sigmas, beta, gamma, ctx):
    dom = zk.Radix2EvaluationDomain.new(1 << log_n, cid, ctx)
    z, last = permutation.permutation_evals(dom, [dev(cid, w) for w in wires], [dev(cid, s) for s in sigmas], m1(cid, beta), m1(cid, gamma),
                                            return_last=True)
    return back(cid, z), fr_from_mont(cid, last.reshape(1, 4))[0]


def run_lookup(cid, f, t, h1, h2, delta, eps, ctx):
    p, last = permutation.lookup_permutation_evals(ctx, cid, dev(cid, f), dev(cid, t), dev(cid, h1), dev(cid, h2), m1(cid, delta), m1(cid, eps),
                                                   return_last=True)
    return back(cid, p), fr_from_mont(cid, last.reshape(1, 4))[0]


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("log_n", [7, 11])
def test_grand_products_on_edge_wires(cid, log_n, ctx):
    cv = bo.CURVES[cid]
    for which in range(4):
        wires, sigmas, beta, gamma = perm_case(cv, log_n, which)
        assert run_perm(cid, log_n, wires, sigmas, beta, gamma, ctx) == bo.perm_product(cv, log_n, wires, sigmas, beta, gamma), which
        f, t, h1, h2, delta, eps = lookup_case(cv, 1 << log_n, which)
        assert run_lookup(cid, f, t, h1, h2, delta, eps, ctx) == bo.lookup_product(cv, f, t, h1, h2, delta, eps), which


@pytest.mark.parametrize("cid", [0, 1])
def test_grand_products_zero_numerator(cid, ctx):
    """A numerator that vanishes at row 5 of 128: every later value and the dropped last one are 0, as in the serial loop -- and the call
    succeeds (only a zero DENOMINATOR is ZK_ERR_NOT_INVERTIBLE)."""
    cv = bo.CURVES[cid]
    log_n, n, p = 7, 128, cv.r
    wires, sigmas, _, _ = perm_case(cv, log_n, 0)
    beta, gamma = bo.seeded_scalars(cv, 0xEC00, 2)
    wires[2][5] = -(beta * bo.PERM_K[2] * pow(cv.root_of_unity(log_n), 5, p) + gamma) % p
    want = bo.perm_product(cv, log_n, wires, sigmas, beta, gamma)
    assert want[0][5] != 0 and want[0][6:] == [0] * (n - 6) and want[1] == 0
    assert run_perm(cid, log_n, wires, sigmas, beta, gamma, ctx) == want
    f, t, h1, h2, _, _ = lookup_case(cv, n, 0)
    delta, eps = bo.seeded_scalars(cv, 0xEC10, 2)
    f[5] = -eps % p
    want = bo.lookup_product(cv, f, t, h1, h2, delta, eps)
    assert want[0][5] != 0 and want[0][6:] == [0] * (n - 6) and want[1] == 0
    assert run_lookup(cid, f, t, h1, h2, delta, eps, ctx) == want


# ---------------------------------------------------------------------------------------------------------------- lookup compression
def round2_case(cv, n, zeta):
    e = ev.edge_elements(cv)
    rows = len(e)
    table_cols = [[e[(STRIDES[k] * (j % rows) + 3 * k) % rows] for j in range(n)] for k in range(4)]
    wires = [ev.edge_column(cv, n, STRIDES[k + 4], k) for k in range(4)]
    q = [1 if i % 3 else 0 for i in range(n - 100)]                    # shorter than n: the rest counts as zero
    for i, qi in enumerate(q):
        if qi:
            for k in range(4):
                wires[k][i] = table_cols[k][(7 * i) % n]
    return table_cols, q, wires, zeta


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("zeta", ["0", "1", "r-1"])
def test_lookup_compression_on_edge_wires(cid, zeta, ctx):
    cv = bo.CURVES[cid]
    n = 512
    table_cols, q, wires, z = round2_case(cv, n, {"0": 0, "1": 1, "r-1": cv.r - 1}[zeta])
    want_t, want_f, want_h1, want_h2 = bo.lookup_round2(cv, n, table_cols, q, wires, z)
    zm = m1(cid, z)
    t = lookup.compress_table([dev(cid, c) for c in table_cols], zm, cid, ctx)
    f = lookup.compress_query(dev(cid, q), [dev(cid, w) for w in wires], zm, t, curve=cid, ctx=ctx)
    assert back(cid, t) == want_t
    assert back(cid, f) == want_f
    h1, h2 = lookup.combine_split(t, f, cid, ctx)
    assert back(cid, h1) == want_h1 and back(cid, h2) == want_h2


# ---------------------------------------------------------------------------------------------------------------- KZG
KZG_LONG = 64 * 1024 + 1                  # CHUNK * SCAN_T + 1 coefficients: past one chunk per lane of the scan
_srs = {}


def srs(cid, ctx, oracle_cpu):
    """tau^i G for i < KZG_LONG on the device (one per curve for the module) and the first 64 as big-int points"""
    if cid not in _srs:
        pw_canon, _ = tau_powers(oracle_cpu, cid, KZG_LONG)
        bases = srs_from_powers(ctx, cid, pw_canon)
        _srs[cid] = (zk.CommitterKey(bases, cid, ctx), bases, bo.srs_powers(bo.CURVES[cid], TAU, 64))
    return _srs[cid]


def kzg_points(cv, m):
    log_n = max(m - 1, 1).bit_length()
    return [("0", 0), ("1", 1), ("r-1", cv.r - 1), ("omega", cv.root_of_unity(log_n))]


def point_ints(cid, pt):
    if pt.infinity:
        return None
    return (zk.curves.fq_from_mont(cid, pt.x.reshape(1, -1))[0], zk.curves.fq_from_mont(cid, pt.y.reshape(1, -1))[0])


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_kzg_open_and_evaluate_on_edge_coefficients(cid, m, ctx, oracle_cpu):
    """Two polynomials of edge coefficients (m and m // 2 + 1 of them) opened at 0, 1, r - 1 and a domain point with the challenge
    r - 1: the witness commitment against bo.kzg_open over the same powers of tau, every evaluation against Horner's rule."""
    cv = bo.CURVES[cid]
    ck, _, powers = srs(cid, ctx, oracle_cpu)
    polys = [ev.edge_column(cv, m, 3, 1), ev.edge_column(cv, m // 2 + 1, 7, 2)]
    d_polys = [dev(cid, p) for p in polys]
    chi = cv.r - 1
    pts = kzg_points(cv, m)
    vals = linearisation.evaluate_batch([d_polys[k] for k in range(2) for _ in pts], fr_to_mont(cid, [z for _ in range(2) for _, z in pts]), cid, ctx)
    assert fr_from_mont(cid, vals) == [bo.horner(polys[k], z, cv.r) for k in range(2) for _, z in pts]
    for name, z in pts:
        got = ck.open(d_polys, m1(cid, z), m1(cid, chi))
        assert point_ints(cid, got) == bo.kzg_open(cv, powers, polys, z, chi), name


@pytest.mark.parametrize("cid", [0, 1])
def test_kzg_open_and_evaluate_past_one_chunk_per_lane(cid, ctx, oracle_cpu):
    """64 * 1024 + 1 edge coefficients: the evaluations against Horner's rule, the witness element by element and its commitment against
    the C++ restatement (synthetic division, then its own MSM over the same powers)."""
    cv = bo.CURVES[cid]
    ck, bases, _ = srs(cid, ctx, oracle_cpu)
    poly = ev.edge_column(cv, KZG_LONG, 5, 3)
    pm = fr_to_mont(cid, poly)
    d_poly = dev(cid, poly)
    pts = kzg_points(cv, KZG_LONG)
    vals = linearisation.evaluate_batch([d_poly] * len(pts), fr_to_mont(cid, [z for _, z in pts]), cid, ctx)
    assert fr_from_mont(cid, vals) == [bo.horner(poly, z, cv.r) for _, z in pts]
    b_host = bases.cpu().numpy().view(np.uint64)
    one = m1(cid, 1)
    for name, z in pts:
        zm = m1(cid, z)
        w = oracle_cpu.kzg_witness(cid, pm, zm)
        got_w = zk.msm.kzg_witness([d_poly], zm, one, cid, ctx).cpu().numpy().view(np.uint64)
        assert np.array_equal(got_w, oracle_cpu.convert(cid, "fr", False, w)), name
        exp_xy, exp_inf = oracle_cpu.kzg_commit(cid, b_host, w)
        got = ck.open([d_poly], zm, one)
        assert bool(got.infinity) == bool(exp_inf) and np.array_equal(got.xy(), exp_xy), name


@pytest.mark.parametrize("cid", [0, 1])
def test_kzg_sum_of_32_terms_at_its_extreme(cid, ctx, oracle_cpu):
    """The one tight bound of the KZG kernels (kzg.hip: kzg_rlc adds up to MAX_POLYS = 32 lazily reduced products, below 64r, and the
    product that follows has room for 70.7r on BLS12-381): 32 terms with every coefficient r - 1 and every multiplier r - 1.  The linear
    combination at lengths 1 and 65 against poly_scale / poly_add, and the opening of 32 polynomials of 65 coefficients with the
    challenge r - 1 at z = 1 and z = r - 1 against bo.kzg_open.  With 32 equal polynomials the powers of -1 cancel and the combination is
    the zero polynomial, so the opening is also taken with polynomial k cut to 65 - k coefficients, where nothing cancels."""
    cv = bo.CURVES[cid]
    p, top = cv.r, cv.r - 1
    for m in (1, 65):
        polys = [[top] * m for _ in range(32)]
        got = linearisation.lincomb([dev(cid, q) for q in polys], fr_to_mont(cid, [top] * 32), curve=cid, ctx=ctx)
        assert back(cid, got) == bo.poly_add(*[bo.poly_scale(q, top, p) for q in polys], p=p), m
    ck, _, powers = srs(cid, ctx, oracle_cpu)
    for name, polys in (("equal", [[top] * 65 for _ in range(32)]), ("ragged", [[top] * (65 - k) for k in range(32)])):
        d_polys = [dev(cid, q) for q in polys]
        for z in (1, top):
            got = ck.open(d_polys, m1(cid, z), m1(cid, top))
            assert point_ints(cid, got) == bo.kzg_open(cv, powers, polys, z, top), (name, z)
