"""The G1 kernels on curve points whose coordinates are base-field edges (tests/edge_values.py: edge_points), every result bit for bit.

Every other base point of the suite is k G for a seeded k, so its coordinates are uniform in Fq; the signed 30-bit-limb field
(csrc/fields.cuh) and the group law over it (csrc/ecu.cuh, csrc/ecq.cuh) promise limb ranges -- strict / almost bounds, one-step
carries, canon_floor on (-2p, 2p), the limb-0 shortcut of madd_finish, from_sat / to_sat at the ends of the word range, is_null() as
"all limbs zero" -- that such inputs never approach.  The edge set aims at each of them in the three forms a coordinate takes: its
value, the stored arkworks word, and the strict limbs of the internal form.  tests/test_fieldu.py runs the same set through the host
compile of the same headers and holds the two references (the big-int law and the C++ Pippenger) equal on it.

The rule for BLS12-381.  BN254 has cofactor 1: every curve point is in G1.  A BLS12-381 edge point is on the curve but outside the
r-torsion subgroup, so r P != O.  The group law, the Pippenger digits, the table rows 2^(c w) P and the NAF of the IPA key fold use a
scalar as an integer and are right on any curve point; the one step that uses r P = O is the scalar fold of the folded window
geometry (MsmGeom::neg, scalar_fold in csrc/msm_sort.hip: k > (r - 1) / 2 becomes (r - k)(-P)).  Therefore
  * every BLS12-381 MSM here takes canonical scalars in [0, (r - 1) / 2] -- fixed where the vector is built and asserted, never
    filtered; (r - 1) / 2 itself, which is not folded, is in;
  * the MSMs go through the canonical-scalar entry points only (multi_scalar_mul, CommitterKey.msm, msm_partial,
    commit_batch(canonical=[True ...])): on the Montgomery-coefficient path the scalar is from_mont of the input;
  * cancellation is built from negated points (x, q - y), never from r - s;
  * BN254 takes the whole range [0, r - 1]: the only run of the scalar fold over edge points with scalars above (r - 1) / 2.
    make_geom folds where that removes a window: at 3 bits on BN254 (window 3, and window 0 at these lengths), at 2, 4, 5, 15 and
    17 bits on BLS12-381, where the folded geometry runs with scalars up to the boundary;
  * the IPA key fold is integer-scalar throughout and takes the whole range on both curves.

What each test reaches, and why a wrong limb of one point fails it (all comparisons are array equality with the oracle's words):
  test_per_window_path: zk_msm_g1 (host arrays) and zk_srs_register_dev + zk_msm_g1_srs_dev (device tensors, flags) at the windows
      0, 2, 3, 4, 5, 8, 13, 16.  bases_to_internal (from_sat + canonical_lt2p of every edge word, the three infinity encodings next
      to (0, 2)), the per-window sort, msm_accumulate's accumulate_chunk (madd of an edge point into an empty, an equal and an
      opposite accumulator), then the reduction: with some 200 points nearly every bucket holds one point, so (x, y, 1, 1) with
      edge x and y is what msm_seg_reduce(_q) and msm_win_finish_q (window 13) / msm_win_finish (window 16) add up; the host tail
      (g1_host.h over the same law) turns the window sums into the affine result.  One sum over all points: a wrong limb in any
      bucket changes it.
  test_edge_outputs: the same pipeline at window 0 onto an edge RESULT -- [P] and [P, Q, -Q] with scalars [1] and [1, k, k] -- so
      that the host tail's inversion, canon_floor and to_sat end on the edge words, compared with the input words.
  test_table_path: the set tiled to 2^14 bases, every tile in another order, so equal and opposite points meet in the shared
      buckets.  msm_precompute (255 doublings per point from an edge, rows normalised by the batched inversion and stored through
      canonical_lt2p) for 16-, 17- and 18-bit windows; msm_accumulate_batch over the table; msm_combine_q (one job) and msm_combine
      (three jobs); msm_seg_reduce_q / msm_win_finish_q, and for 18 bits the wide reduction with msm_node_reduce_q; 17 bits is the
      folded geometry on BLS12-381 (15 windows; BN254 has 15 either way).  Single MSMs are 2^13 long, the shortest the table path takes; the two
      partials are the halves of 2^14, so that both stay on the table path (the second through a base offset), and their host sum
      (zk_g1_sum_partials) equals the single MSM over all 2^14.
  test_ipa_key_fold: ipa_fold_key over the set against itself rotated, m not a multiple of the 128-lane block: dbl / madd chains on
      edge points by the NAF of xi, the block's batched inversion and canonical_lt2p of each result; xi = 0 returns the left edge
      point itself through that inversion, xi = 1 with L = -R gives infinity and with L = R the doubling branch of madd.
  test_fixed_base_on_edge_scalars: g1_fixed_base, which builds the bases of nearly every other device test, on the edge SCALARS and
      on r, r + 1, 2^256 - 1, against the big-int affine law (k mod r) G; k = 0 (mod r) gives the all-zero words."""
import random

import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib
from oracle import bigint_oracle as bo
from tests import edge_values as ev

pytestmark = pytest.mark.gpu

CURVES = pytest.mark.parametrize("cid", [0, 1], ids=["bls12_381", "bn254"])
PRE_MIN_N = 1 << 13             # ZK_PRE_MIN_N: the shortest MSM of the table path


def scalar_top(cv):
    """the largest scalar an MSM over edge points may take: see the rule above"""
    return cv.r - 1 if cv.curve_id == 1 else (cv.r - 1) // 2


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _dev_u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _limbs4(ints):
    return zk.curves.ints_to_limbs(ints, 4)


def _assert_point(got, exp_xy, exp_inf, tag):
    assert got.infinity == bool(exp_inf), tag
    if not exp_inf:
        assert np.array_equal(got.xy(), exp_xy), tag


class _Set:
    """the edge points of one curve with their words, and the vector of the per-window test with the oracle's sum, built once"""

    def __init__(self, cid, oracle_cpu):
        self.cid, self.cv = cid, bo.CURVES[cid]
        cv = self.cv
        self.pts = [tuple(e) for e in ev.edge_points(cv)]
        self.words = ev.points_to_limbs(cv, self.pts)
        self.top = scalar_top(cv)
        self.rows = ev.edge_msm_rows(cv, self.top)
        scal = [s for _, s, _ in self.rows]
        assert max(scal) <= self.top and {0, 1, self.top} <= set(scal)
        self.bases, self.scal, self.flags, all_flags = ev.rows_arrays(cv, self.rows)
        self.exp = oracle_cpu.msm_g1(cid, self.bases, self.scal, inf=all_flags)
        assert not self.exp[1]


@pytest.fixture(scope="module")
def sets(oracle_cpu):
    made = {}

    def get(cid):
        if cid not in made:
            made[cid] = _Set(cid, oracle_cpu)
        return made[cid]
    return get


@CURVES
@pytest.mark.parametrize("window", [0, 2, 3, 4, 5, 8, 13, 16])
def test_per_window_path(cid, window, ctx, sets):
    s = sets(cid)
    ctx.set_msm_window(window)
    try:
        got = zk.VariableBaseMSM.multi_scalar_mul(s.bases, s.scal, cid, infinity=s.flags, ctx=ctx)
        _assert_point(got, *s.exp, f"host arrays, window {window}")
        ck = zk.CommitterKey(_dev(s.bases), cid, ctx, infinity=_dev_u8(s.flags))
        try:
            _assert_point(ck.msm(_dev(s.scal)), *s.exp, f"device tensors, window {window}")
        finally:
            ck.close()
    finally:
        ctx.set_msm_window(0)


@CURVES
def test_edge_outputs(cid, ctx, sets):
    """MSM([P], [1]) and MSM([P, Q, -Q], [1, k, k]) are P, limb for limb the input words: the whole pipeline onto an edge result."""
    s = sets(cid)
    cv, m = s.cv, len(s.pts)
    ks = ev.edge_scalars(cv, m, s.top, stride=3, start=4, seed=10 + cid)
    assert max(ks) <= s.top
    for i in range(m):
        j = (5 * i + 1) % m
        if s.pts[j][0] == s.pts[i][0]:                       # a partner is another point and not the negation
            j = (j + 1) % m
        assert s.pts[j][0] != s.pts[i][0]
        got = zk.VariableBaseMSM.multi_scalar_mul(s.words[i:i + 1], _limbs4([1]), cid, ctx=ctx)
        _assert_point(got, s.words[i], 0, ("alone", i))
        nq = ev.points_to_limbs(cv, [(s.pts[j][0], cv.q - s.pts[j][1])])[0]
        got = zk.VariableBaseMSM.multi_scalar_mul(np.stack([s.words[i], s.words[j], nq]), _limbs4([1, ks[i], ks[i]]), cid, ctx=ctx)
        _assert_point(got, s.words[i], 0, ("P + k Q - k Q", i, j, hex(ks[i])))


@CURVES
def test_table_path(cid, ctx, sets, oracle_cpu):
    s = sets(cid)
    cv, m = s.cv, len(s.pts)
    n = 2 * PRE_MIN_N
    rng = random.Random(0x7AB1E + cid)
    idx = []
    while len(idx) < n:                                      # tiles of the whole set, each in another order
        tile = list(range(m))
        rng.shuffle(tile)
        idx += tile
    idx = np.array(idx[:n])
    bases_h = s.words[idx]
    bases = _dev(bases_h)
    vecs = []
    for k in range(3):
        sc = ev.edge_scalars(cv, n, s.top, stride=(5, 11, 17)[k], start=3 * k, seed=20 + 3 * cid + k)
        assert max(sc) <= s.top
        vecs.append(_limbs4(sc))
    want_short = [oracle_cpu.msm_g1(cid, bases_h[:PRE_MIN_N], v[:PRE_MIN_N]) for v in vecs]
    want_all = oracle_cpu.msm_g1(cid, bases_h, vecs[0])
    d_short = [_dev(v[:PRE_MIN_N]) for v in vecs]
    d_all = _dev(vecs[0])
    for c in (0, 16, 17, 18):                                # 0: no table, the per-window path at this length; a key holds one table
        ck = zk.CommitterKey(bases, cid, ctx)
        try:
            if c:
                ck.precompute(c)
            assert ck.table_window_bits() == c
            _assert_point(ck.msm(d_short[0]), *want_short[0], (c, "one vector"))
            got = ck.commit_batch(d_short, canonical=[True] * 3)
            assert len(got) == 3
            for k in range(3):
                _assert_point(got[k], *want_short[k], (c, "batch", k))
            _assert_point(ck.msm(d_all), *want_all, (c, "both halves as one"))
            parts = [ck.msm_partial(d_all[:PRE_MIN_N], 0), ck.msm_partial(d_all[PRE_MIN_N:], PRE_MIN_N)]
            _assert_point(zk.sum_partials(np.stack(parts), cid), *want_all, (c, "partials"))
        finally:
            ck.close()


@CURVES
def test_ipa_key_fold(cid, ctx, sets, oracle_cpu):
    import torch
    s = sets(cid)
    cv, m0 = s.cv, len(s.pts)
    L = cv.fq_limbs
    neg = lambda p: (p[0], cv.q - p[1])
    right = [s.pts[(i + 37) % m0] for i in range(m0)]
    # with xi = 1: L = -R folds to infinity, L = R takes the doubling branch of the last addition
    left = list(s.pts) + [neg(s.pts[9]), s.pts[21]]
    right += [s.pts[9], s.pts[21]]
    m = len(left)
    assert m % 128 and m > 128
    key_h = ev.points_to_limbs(cv, left + right)
    key = _dev(key_h)
    inf = torch.zeros(2 * m, dtype=torch.uint8, device="cuda")
    one = _limbs4([1])[0]
    for xi in (0, 1, 2, cv.r - 1, bo.seeded_scalars(cv, 0xF01D + cid, 1)[0]):
        out = torch.zeros((m, 2 * L), dtype=torch.int64, device="cuda")
        oinf = torch.zeros(m, dtype=torch.uint8, device="cuda")
        xm = zk.curves.fr_to_mont(cid, [xi])
        ctx.use_torch_stream()
        _lib.check(_lib.lib().zk_ipa_fold_key_dev(ctx.handle, cid, m, key.data_ptr(), inf.data_ptr(), xm.ctypes.data, out.data_ptr(),
                                                  oinf.data_ptr()))
        got, gi = out.cpu().numpy().view(np.uint64), oinf.cpu().numpy()
        xl = np.stack([one, _limbs4([xi])[0]])
        exp = [oracle_cpu.msm_g1(cid, np.stack([key_h[i], key_h[m + i]]), xl, threads=1) for i in range(m)]
        if xi == 1:
            assert exp[m - 2][1] == 1 and exp[m - 1][1] == 0   # the cancelling pair and the doubling pair
        for i, (exp_xy, exp_inf) in enumerate(exp):
            assert gi[i] == exp_inf, (hex(xi), i)
            if not exp_inf:
                assert np.array_equal(got[i], exp_xy), (hex(xi), i)
        if xi == 0:
            assert np.array_equal(got, key_h[:m])


@CURVES
def test_fixed_base_on_edge_scalars(cid, ctx):
    import torch
    cv = bo.CURVES[cid]
    ks = ev.edge_elements(cv) + [cv.r, cv.r + 1, (1 << 256) - 1]
    out = torch.empty((len(ks), 2 * cv.fq_limbs), dtype=torch.int64, device="cuda")
    d_k = _dev(_limbs4(ks))
    ctx.use_torch_stream()
    _lib.check(_lib.lib().zk_g1_fixed_base_batch_dev(ctx.handle, cid, d_k.data_ptr(), len(ks), out.data_ptr()))
    torch.cuda.synchronize()
    G = (cv.gx, cv.gy)
    pow2 = [G]                                                # 2^i G, shared: k G is then the sum over the set bits of k mod r by the
    for _ in range(cv.r.bit_length() - 1):                    # same affine law as bo.ec_mul, with a third of its inversions
        pow2.append(bo.ec_add(cv, pow2[-1], pow2[-1]))
    pts = []
    for k in ks:
        acc = None
        for i in range(cv.r.bit_length()):
            if (k % cv.r) >> i & 1:
                acc = bo.ec_add(cv, acc, pow2[i])
        pts.append(acc)
    for i in (4, 7, len(ks) - 1):                             # r - 1, (r - 1) / 2, 2^256 - 1: bo.ec_mul itself
        assert pts[i] == bo.ec_mul(cv, ks[i] % cv.r, G)
    want = ev.points_to_limbs(cv, pts)
    assert not want[0].any() and not want[-3].any()           # k = 0 and k = r: the all-zero words
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
