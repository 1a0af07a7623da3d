"""Every launch route of the bucket reduction (csrc/msm_reduce.hip) at the smallest length the table path takes, 2^13 points, against the
CPU oracle's Pippenger, limb for limb, through the public calls.  Which kernels a case reaches follows from the code:

  (a) 16-bit table, random scalars: one job -> msm_combine_q, three jobs -> msm_combine<F, 1> (option combine_sg = 2 / 4: the
      <F, 2> / <F, 4> instances); then msm_seg_reduce_q and msm_win_finish_q<F, 512> (64 virtual windows of 64 chains).
  (b) the same table, skewed scalars.  At this length the plan gives 16 references per lane (pre_plan_geom halves chunk_l down to 16,
      and chunk_len never goes below 16), so a bucket with m references spans at least m / 16 chunks: 49152 references are more than
      COMBINE_MEDIUM = 2048 chunks (msm_combine_block takes the bucket), 1024 are between COMBINE_SMALL = 32 and that
      (msm_combine_wave).
  (c) options pre_vw = 8, pre_logg = 0: 4096 segments per virtual window, logq = 4 -> msm_seg_reduce + msm_win_finish with the second
      (total) output, which no other input reaches.
  (d) 18-bit table (2^17 shared buckets): the wide reduction -- msm_seg_reduce, msm_node_reduce_q, msm_win_finish_q raw, level 4.

The per-window path (window 13: msm_win_finish_q<F, 1024>; window 16: msm_win_finish without the total) is covered by
tests/test_msm_gpu.py, the device window-sum form and g1_sum_winsums_q by test_winsums_form_with_short_and_empty_jobs
(tests/test_distributed.py)."""
import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib

pytestmark = pytest.mark.gpu

N = 1 << 13                     # ZK_PRE_MIN_N: the smallest length of the table path
CHUNK = 16                      # references per lane at this length (see above)
COMBINE_SMALL, COMBINE_MEDIUM = 32, 2048
D1, D2 = 0x2345, 0x0678         # the two heavy buckets: different, below 2^15 (no carry into the next window)
CURVES = pytest.mark.parametrize("cid", [0, 1], ids=["bls12_381", "bn254"])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _random(seed, n=N):
    s = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    s[:, 3] &= np.uint64((1 << 60) - 1)           # below r of either curve
    return s


def _skewed(c, seed, d1=D1, d2=D2):
    """6144 x d1 in the windows 0 .. 7 (c bits each), 1024 x d2 alone, 1024 random scalars"""
    heavy = sum(d1 << (c * w) for w in range(8))
    s = _random(seed)
    s[:6144] = zk.curves.ints_to_limbs([heavy], 4)[0]
    s[6144:7168] = zk.curves.ints_to_limbs([d2], 4)[0]
    return s


def _assert_size_classes(scal, c, d1=D1, d2=D2):
    """references of the constructed rows in the buckets d1 and d2 (their windows hold no carry): the workgroup and the wavefront class"""
    if c == 16:
        win = np.ascontiguousarray(scal[:7168]).view(np.uint16)              # little-endian: 16 windows of 16 bits per scalar
        refs1, refs2 = int((win[:6144] == d1).sum()), int((win[6144:] == d2).sum())
    else:
        k1, k2 = (sum(int(scal[i, j]) << (64 * j) for j in range(4)) for i in (0, 6144))
        refs1 = 6144 * sum(((k1 >> (c * w)) & ((1 << c) - 1)) == d1 for w in range(256 // c + 1))
        refs2 = 1024 * sum(((k2 >> (c * w)) & ((1 << c) - 1)) == d2 for w in range(256 // c + 1))
    assert refs1 == 49152 and refs2 == 1024
    assert refs1 // CHUNK > COMBINE_MEDIUM and COMBINE_SMALL < refs2 // CHUNK <= COMBINE_MEDIUM


class _Key:
    """2^13 points k_i G (random 62-bit k_i) of one curve, and the oracle's result for every scalar vector asked for, computed once"""

    def __init__(self, ctx, cid, oracle_cpu):
        import torch
        self.ctx, self.cid, self.oracle = ctx, cid, oracle_cpu
        cv = zk.get_curve(cid)
        g = torch.Generator(device="cuda").manual_seed(8100 + cid)
        ks = torch.randint(1, 1 << 62, (N, 4), dtype=torch.int64, device="cuda", generator=g)
        ks[:, 1:] = 0
        self.bases = torch.empty((N, 2 * cv.fq_limbs), dtype=torch.int64, device="cuda")
        ctx.use_torch_stream()
        _lib.check(_lib.lib().zk_g1_fixed_base_batch_dev(ctx.handle, cid, ks.data_ptr(), N, self.bases.data_ptr()))
        self.bases_h = self.bases.cpu().numpy().view(np.uint64)
        self.tables, self.scal, self.exp = {}, {}, {}

    def table(self, c):
        if c not in self.tables:
            self.tables[c] = zk.CommitterKey(self.bases, self.cid, self.ctx).precompute(c)
            assert self.tables[c].table_window_bits() == c
        return self.tables[c]

    def case(self, name, make):
        if name not in self.scal:
            self.scal[name] = make()
            self.exp[name] = self.oracle.msm_g1(self.cid, self.bases_h, self.scal[name])
        return self.scal[name]

    def check(self, c, names, tag):
        """one job through the single-MSM entry point, several as one round batch: the oracle's points"""
        ck = self.table(c)
        dev = [_dev(self.scal[n]) for n in names]
        got = [ck.msm(dev[0])] if len(names) == 1 else ck.commit_batch(dev, canonical=[True] * len(names))
        assert len(got) == len(names)
        for n, pt in zip(names, got):
            exp_xy, exp_inf = self.exp[n]
            assert pt.infinity == bool(exp_inf), (tag, n)
            if not exp_inf:
                assert np.array_equal(pt.xy(), exp_xy), (tag, n)

    def close(self):
        for ck in self.tables.values():
            ck.close()


@pytest.fixture(scope="module")
def keys(ctx, oracle_cpu):
    ks = {}

    def get(cid):
        if cid not in ks:
            ks[cid] = _Key(ctx, cid, oracle_cpu)
            for j in range(3):
                ks[cid].case(f"random{j}", lambda j=j: _random(100 * cid + j))
        return ks[cid]
    yield get
    for k in ks.values():
        k.close()


RANDOM3 = ["random0", "random1", "random2"]


@CURVES
def test_sixteen_bit_table_one_and_three_jobs_and_the_combine_sg_option(ctx, keys, cid):
    k = keys(cid)
    k.check(16, RANDOM3[:1], "one job")
    k.check(16, RANDOM3, "three jobs")
    try:
        for sg in (2, 4):
            ctx.set_option("combine_sg", sg)
            k.check(16, RANDOM3, f"three jobs, combine_sg {sg}")
    finally:
        ctx.set_option("combine_sg", 0)


def test_skewed_scalars_fill_both_combine_queues(keys):
    k = keys(0)
    skew = k.case("skew16", lambda: _skewed(16, 16))
    _assert_size_classes(skew, 16)
    skew_b = k.case("skew16b", lambda: _skewed(16, 17, D2, D1))
    _assert_size_classes(skew_b, 16, D2, D1)
    k.check(16, ["skew16"], "skew, one job")
    k.check(16, ["skew16", "random1", "skew16b"], "skew, three jobs")


def test_lane_reduction_with_the_total_output(ctx, keys):
    k = keys(0)
    try:
        ctx.set_option("pre_vw", 8)
        ctx.set_option("pre_logg", 0)
        k.check(16, RANDOM3[:1], "pre_vw 8, pre_logg 0, one job")
        k.check(16, RANDOM3, "pre_vw 8, pre_logg 0, three jobs")
    finally:
        ctx.set_option("pre_vw", 0)
        ctx.set_option("pre_logg", -1)


@CURVES
def test_eighteen_bit_table_takes_the_wide_reduction(keys, cid):
    k = keys(cid)
    k.check(18, RANDOM3[:1], "wide, one job")
    k.check(18, RANDOM3, "wide, three jobs")
    if cid == 0:
        skew = k.case("skew18", lambda: _skewed(18, 18))
        _assert_size_classes(skew, 18)
        k.check(18, ["skew18"], "wide, skew, one job")
