"""The field products of csrc/fields.cuh -- the chained ones of Fs<P, true> (one multiply-add chain per column, the high-half digit
cut from the unbiased column sum), which the two accumulation kernels run, and the plain ones of every other kernel on the way
(precompute, the reductions, the fixed base) -- through the kernels that are built from them, limb for limb against the CPU oracle
(oracle.cpu.msm_g1) and, for the fixed base, against ark_plonk_amd.curves.g1_mul.  The products cannot be called on the device by
themselves; a wrong carry or digit in any of them changes a coordinate of a bucket and with it the one sum each case compares.

Both curves, and both accumulation paths, forced the way tests/test_accumulate_lean_gpu.py forces them: an MSM below 2^13 scalars
runs the per-window kernel (msm_accumulate<F, false>), and a key with a window table runs msm_accumulate_batch from 2^13 scalars on.
The table path has no shorter MSM, so there the sizes below are the scalars that are NOT zero in a vector of 2^13 (a zero scalar has
no digit and adds no reference): the accumulation sees the references of n points, the oracle is given the same padded vector.
  sizes         n = 1, 2, 63, 64, 65, 1024 random points under random scalars;
  chunk edges   n = 1024 under four distinct scalars: every window holds at most four buckets of some 256 references, which span the
                chunks of 32 references of the per-window path and, with the option chunk_l = 8, of the table path;
  edge points   the Fq-edge set of tests/edge_values.py (the generators of tests/test_edge_points_gpu.py) under two scalars, so that
                every window adds up half the set in one bucket; scalars at most (r - 1) / 2 on BLS12-381, where the set lies
                outside the subgroup (the rule of that test's docstring);
  P == Q        one base 64 times under one scalar: the second reference of every bucket takes dbl_affine (sqr, dot2);
  P == -Q       a base and its negation under one scalar, alone (the sum is infinity) and in front of a third point (the run is at
                infinity in the middle of a bucket);
  fixed base    zk_g1_fixed_base_batch_dev on 64 scalars: 0, 1, r - 1, (r - 1) / 2, single bits, all-ones."""
import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib
from oracle import bigint_oracle as bo
from tests import edge_values as ev

pytestmark = pytest.mark.gpu

CURVES = pytest.mark.parametrize("cid", [0, 1], ids=["bls12_381", "bn254"])
PRE_N = 1 << 13                 # the shortest MSM of the table path
SIZES = (1, 2, 63, 64, 65, 1024)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _limbs4(ints):
    return zk.curves.ints_to_limbs(ints, 4)


def _neg(cv, words_of, pt):
    return words_of([(pt[0], cv.q - pt[1])])[0]


def _cases(cid, oracle_cpu):
    """name -> (bases words (PRE_N, 2L), scalars as ints (n <= PRE_N; the rest of the vector is zero))"""
    cv = bo.CURVES[cid]
    rng = np.random.default_rng(0xF1E1D + cid)
    srs = oracle_cpu.srs_powers(cid, 0x7A5C0DE, PRE_N)          # distinct points k G
    rand = bo.seeded_scalars(cv, 0xC4A1 + cid, 1024)
    out = {f"random_{n}": (srs, rand[:n]) for n in SIZES}
    pool = bo.seeded_scalars(cv, 0xC4A2 + cid, 4)
    out["chunk_edges_1024"] = (srs, [pool[int(i)] for i in rng.integers(0, 4, size=1024)])

    # the Fq-edge points, tiled to the table length; two scalars at most `top`
    top = cv.r - 1 if cid == 1 else (cv.r - 1) // 2
    pts = [tuple(e) for e in ev.edge_points(cv)]
    words = ev.points_to_limbs(cv, pts)
    m = len(pts)
    two = [top, ev.edge_scalars(cv, 8, top, stride=3, start=4, seed=70 + cid)[5]]
    assert 1 < two[1] <= top
    out["edge_points"] = (words[np.arange(PRE_N) % m], [two[i & 1] for i in range(m)])

    G = (cv.gx, cv.gy)
    P, Q = bo.ec_mul(cv, 0xB16B00B5, G), bo.ec_mul(cv, 0x5EED, G)
    wP, wQ = ev.points_to_limbs(cv, [P, Q])
    k = rand[7]
    same = srs.copy()
    same[:64] = wP
    out["p_equals_q"] = (same, [k] * 64)
    opp = srs.copy()
    opp[0], opp[1], opp[2] = wP, _neg(cv, lambda p: ev.points_to_limbs(cv, p), P), wQ
    out["p_plus_minus_p"] = (opp, [k, k])
    out["p_minus_p_then_q"] = (opp, [k, k, k])
    return out


@pytest.fixture(scope="module")
def expected(oracle_cpu):
    """per curve: name -> (bases, padded scalar limbs, n, the oracle's (xy, infinity)); the oracle runs once per case, on the padded
    vector -- its zero scalars add nothing, so the same point is expected of the first n scalars alone"""
    made = {}

    def get(cid):
        if cid not in made:
            made[cid] = {}
            for name, (bases, scal) in _cases(cid, oracle_cpu).items():
                s = _limbs4(list(scal) + [0] * (PRE_N - len(scal)))
                made[cid][name] = (bases, s, len(scal), oracle_cpu.msm_g1(cid, bases, s))
        return made[cid]
    return get


def _assert_point(got, want, tag):
    exp_xy, exp_inf = want
    L = len(exp_xy) // 2
    assert got.infinity == bool(exp_inf), tag
    if not exp_inf:
        assert np.array_equal(got.x, exp_xy[:L]) and np.array_equal(got.y, exp_xy[L:]), tag


@CURVES
def test_products_through_both_accumulation_paths(cid, ctx, expected):
    cases = expected(cid)
    assert cases["p_plus_minus_p"][3][1] == 1 and cases["p_minus_p_then_q"][3][1] == 0 and cases["p_equals_q"][3][1] == 0
    keys = {}
    try:
        for name, (bases, s, n, want) in cases.items():
            if id(bases) not in keys:                          # one key, and one table, per base array
                keys[id(bases)] = zk.CommitterKey(_dev(bases), cid, ctx)
            ck = keys[id(bases)]
            d_s = _dev(s)
            assert n < PRE_N
            _assert_point(ck.msm(d_s[:n].contiguous()), want, f"curve {cid} {name} per-window")
        for ck in keys.values():
            ck.precompute()
            assert ck.table_window_bits() == 16 and ck.table_windows() != 0
        for name, (bases, s, n, want) in cases.items():
            ck = keys[id(bases)]
            for chunk_l in (0, 8) if name == "chunk_edges_1024" else (0,):
                ctx.set_option("chunk_l", chunk_l)
                try:
                    _assert_point(ck.msm(_dev(s)), want, f"curve {cid} {name} table, chunk_l {chunk_l}")
                finally:
                    ctx.set_option("chunk_l", 0)
    finally:
        for ck in keys.values():
            ck.close()


@CURVES
def test_fixed_base_on_64_scalars(cid, ctx):
    import torch
    cv = bo.CURVES[cid]
    r = cv.r
    bits = r.bit_length()
    ks = [0, 1, r - 1, (r - 1) // 2, (1 << 256) - 1, (1 << 255) - 1, (1 << 64) - 1, (1 << 30) - 1]
    ks += [1 << b for b in (1, 29, 30, 31, 32, 63, 64, 127, 128, bits - 2, bits - 1, 255)]
    ks += bo.seeded_scalars(cv, 0xF1BA5E + cid, 64 - len(ks))
    assert len(ks) == 64
    out = torch.empty((64, 2 * cv.fq_limbs), dtype=torch.int64, device="cuda")
    d_k = _dev(_limbs4(ks))
    ctx.use_torch_stream()
    _lib.check(_lib.lib().zk_g1_fixed_base_batch_dev(ctx.handle, cid, d_k.data_ptr(), 64, out.data_ptr()))
    torch.cuda.synchronize()
    want = ev.points_to_limbs(cv, [zk.curves.g1_mul(cid, k) for k in ks])
    assert not want[0].any()                                    # k = 0: the all-zero words
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
