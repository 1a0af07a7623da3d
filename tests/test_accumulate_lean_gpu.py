"""The bucket accumulation (csrc/msm_accumulate.hip: accumulate_chunk) on inputs chosen so that every step of a lane that is not a
plain addition is taken: a run that starts (the point is written over the accumulator), P == Q (the row is read again and doubled),
P == -Q (the run is at infinity in the middle of a bucket and the next reference starts it again), a row that holds no point, a run
that ends at every reference, and one bucket that spans many chunks (head partial, whole-chunk runs, tail partial).

Each case runs on the table path at its smallest length (2^13 scalars, c = 16) and at 2^13 + 1 (odd), and on the per-window path at
1024 and 33 scalars, on both curves, and is compared limb for limb with oracle.cpu.msm_g1 -- the reference's algorithm, which has no
exceptional-case shortcuts of its own to hide behind (checked without a GPU against the scalar identity sum s_i k_i G)."""
import numpy as np
import pytest

import ark_plonk_amd as zk
from oracle import bigint_oracle as bo

pytestmark = pytest.mark.gpu

N = (1 << 13) + 1
LENGTHS = ((True, 1 << 13), (True, N), (False, 1024), (False, 33))        # (table path, scalars)
KINDS = ("duplicates", "cancellation", "infinity_in_srs", "single_reference_buckets", "one_heavy_bucket", "uniform")


def _limbs(cv, pt):
    R = 1 << (64 * cv.fq_limbs)
    return np.array(bo.int_to_limbs(bo.to_mont(pt[0], cv.q, R), cv.fq_limbs) + bo.int_to_limbs(bo.to_mont(pt[1], cv.q, R), cv.fq_limbs),
                    dtype=np.uint64)


def eight_point_srs(cid):
    """N points drawn from 8 distinct ones, four points and their negatives: (bases, the multiplier k_i of every point)"""
    cv = bo.CURVES[cid]
    rng = np.random.default_rng(800 + cid)
    ks = [int(k) for k in rng.integers(2, 1 << 40, size=4)]
    pts, mult = [], []
    for k in ks:
        x, y = bo.ec_mul(cv, k, (cv.gx, cv.gy))
        pts += [_limbs(cv, (x, y)), _limbs(cv, (x, cv.q - y))]
        mult += [k, cv.r - k]
    pick = rng.integers(0, 8, size=N)
    return np.stack([pts[int(i)] for i in pick]), [mult[int(i)] for i in pick]


def case_inputs(cid, kind, oracle_cpu):
    """(bases, infinity flags or None, scalars as ints, multipliers k_i with P_i = k_i G or None)"""
    cv = bo.CURVES[cid]
    rng = np.random.default_rng(900 + cid)
    bases, mult = eight_point_srs(cid)
    inf = None
    if kind == "duplicates":
        pool = bo.seeded_scalars(cv, 31, 16)
        scal = [pool[int(i)] for i in rng.integers(0, 16, size=N)]
    elif kind == "cancellation":
        # pairs s, r - s on equal points (the SRS repeats with period 2: point 2j + 1 is point 2j)
        bases, mult = np.repeat(bases[: (N + 1) // 2], 2, axis=0)[:N], [m for m in mult[: (N + 1) // 2] for _ in (0, 1)][:N]
        pool = bo.seeded_scalars(cv, 32, 16)
        half = [pool[int(i)] for i in rng.integers(0, 16, size=(N + 1) // 2)]
        scal = [v for s in half for v in (s, cv.r - s)][:N]
    elif kind == "infinity_in_srs":
        inf = np.zeros(N, dtype=np.uint8)
        inf[::7] = 1
        mult = [0 if i % 7 == 0 else m for i, m in enumerate(mult)]
        pool = bo.seeded_scalars(cv, 33, 16)
        scal = [pool[int(i)] for i in rng.integers(0, 16, size=N)]
    elif kind == "single_reference_buckets":
        scal = [int(v) for v in rng.permutation(N) + 1]               # distinct, below 2^15: one digit, one reference per bucket
    elif kind == "one_heavy_bucket":
        bases, mult = oracle_cpu.srs_powers(cid, 0x7A5C0DE, N), None  # distinct points: a genuine long sum in every window's one bucket
        scal = [bo.seeded_scalars(cv, 34, 1)[0]] * N
    else:
        bases, mult = oracle_cpu.srs_powers(cid, 0x7A5C0DE, N), None
        scal = bo.seeded_scalars(cv, 35, N)
    return bases, inf, scal, mult


@pytest.fixture(scope="module")
def expected(oracle_cpu):
    """inputs and the oracle's result of every (curve, kind, length), computed once"""
    out = {}
    for cid in (0, 1):
        for kind in KINDS:
            bases, inf, scal, _ = case_inputs(cid, kind, oracle_cpu)
            s = zk.curves.ints_to_limbs(scal, 4)
            out[cid, kind] = (bases, inf, s, {n: oracle_cpu.msm_g1(cid, bases[:n], s[:n], None if inf is None else inf[:n]) for _, n in LENGTHS})
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cid", [0, 1])
def test_accumulation_steps_that_are_not_additions(cid, kind, ctx, expected):
    import torch
    L = bo.CURVES[cid].fq_limbs
    bases, inf, s, want = expected[cid, kind]
    d_s = torch.from_numpy(s.view(np.int64)).cuda()
    # a key over device bases is never shared with another registration of the same points
    d_inf = None if inf is None else torch.from_numpy(inf).cuda()
    ck = zk.CommitterKey(torch.from_numpy(bases.view(np.int64)).cuda(), cid, ctx, infinity=d_inf)
    try:
        for use_table, n in sorted(LENGTHS):                          # the per-window lengths first, then the table is built
            if use_table and ck.table_windows() == 0:
                ck.precompute()
                assert ck.table_window_bits() == 16
            assert use_table == (ck.table_windows() != 0)
            got = ck.msm(d_s[:n].contiguous())
            exp_xy, exp_inf = want[n]
            tag = f"curve {cid} {kind} n={n} {'table' if use_table else 'per-window'}"
            assert got.infinity == bool(exp_inf), tag
            assert np.array_equal(got.x, exp_xy[:L]) and np.array_equal(got.y, exp_xy[L:]), tag
    finally:
        ck.close()
