"""The segmented G1 MSM on the MI355X (ark_plonk_amd.msm.segments_msm over csrc/g1_segments.hip): many small MSMs over one set of
bases, each as a point.  The oracle is known logarithms: base i = k_i G (test_ipa_gpu.points_of), so segment s must be
(sum_t scalar_t k_index[t] mod r) G -- one big-int scalar multiplication per segment; one small case is added up term by term with
the big-int group law over the points themselves."""
import numpy as np
import pytest

from oracle import bigint_oracle as bo
from test_ipa_gpu import CURVES, points_of, rand_logs

pytestmark = pytest.mark.gpu
SEG_OK, SEG_BAD_RANGE, SEG_BAD_INDEX = 0, 1, 2


def run(ctx, cid, bases, inf, offsets, index, scalars):
    """segments_msm on host lists -> ([(x, y) | None per segment], [status])"""
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd.msm import segments_msm
    L = zk.get_curve(cid).fq_limbs
    sc = torch.from_numpy(zk.curves.ints_to_limbs(scalars, 4).view(np.int64)).cuda().view(-1, 4)
    xy, oinf, st = segments_msm(bases, inf, torch.tensor(offsets, dtype=torch.int64, device="cuda"),
                                torch.tensor(np.asarray(index, dtype=np.uint32).view(np.int32), dtype=torch.int32, device="cuda"), sc, cid, ctx)
    torch.cuda.synchronize()
    xy, oinf = xy.cpu().numpy().view(np.uint64), oinf.cpu().numpy()
    one = zk.curves.fq_to_mont(cid, [0, 1]).reshape(-1)
    pts = []
    for s in range(len(offsets) - 1):
        if oinf[s]:
            assert (xy[s] == one).all(), ("infinity is written as (0, 1)", s)
            pts.append(None)
        else:
            pts.append(tuple(zk.curves.fq_from_mont(cid, xy[s].reshape(2, L))))
    return pts, st.cpu().numpy().tolist()


def expect(cv, logs, offsets, index, scalars, s):
    e = sum(scalars[t] * logs[index[t]] for t in range(offsets[s], offsets[s + 1])) % cv.r
    return bo.ec_mul(cv, e, (cv.gx, cv.gy)) if e else None


def special_scalars(cv, n, seed):
    sc = rand_logs(cv, n, seed)
    for i, v in enumerate((0, 1, 2, cv.r - 1, (1 << 255) - 19)):       # 2^255 - 19 is above r: the integer multiple
        if 3 * i + 1 < n:
            sc[3 * i + 1] = v
    return sc


@pytest.mark.parametrize("cid", [0, 1])
def test_segment_lengths_around_the_wavefront_in_one_call(ctx, cid):
    cv = CURVES[cid]
    logs = rand_logs(cv, 23, 5)
    bases = points_of(ctx, cid, logs)
    lens = [0, 1, 2, 63, 64, 65, 130]
    offsets = [0] + np.cumsum(lens).tolist()
    n = offsets[-1]
    index = np.random.default_rng(11).integers(0, 23, size=n).tolist()          # 325 terms over 23 bases: repeats
    scalars = special_scalars(cv, n, 77)
    got, st = run(ctx, cid, bases, None, offsets, index, scalars)
    assert st == [SEG_OK] * len(lens)
    assert got[0] is None
    for s in range(len(lens)):
        assert got[s] == expect(cv, logs, offsets, index, scalars, s), (cid, s)


@pytest.mark.parametrize("n_seg", [1, 3, 64, 65])
@pytest.mark.parametrize("cid", [0, 1])
def test_segment_counts_around_the_workgroup(ctx, cid, n_seg):
    cv = CURVES[cid]
    logs = rand_logs(cv, 9, 6)
    bases = points_of(ctx, cid, logs)
    lens = [(3 * s + 1) % 5 for s in range(n_seg)]
    offsets = [0] + np.cumsum(lens).tolist()
    n = offsets[-1]
    index = np.random.default_rng(n_seg).integers(0, 9, size=n).tolist()
    scalars = special_scalars(cv, n, 100 + n_seg)
    got, st = run(ctx, cid, bases, None, offsets, index, scalars)
    assert st == [SEG_OK] * n_seg
    for s in range(n_seg):
        assert got[s] == expect(cv, logs, offsets, index, scalars, s), (cid, n_seg, s)


@pytest.mark.parametrize("cid", [0, 1])
def test_equal_opposite_and_infinite_terms(ctx, cid):
    """What the LDS reduction and the lane's own loop meet: P + P, P + (-P), a sum that cancels across lanes 0 and 63, an
    infinity-flagged base under a non-zero scalar, an all-zero-words base under a zero scalar."""
    import torch
    cv = CURVES[cid]
    r = cv.r
    k, k2, s, s2 = rand_logs(cv, 4, 9)
    logs = [k, r - k, k2, 0, k2]               # 0: P   1: -P   2: Q   3: all-zero words   4: Q's words under an infinity flag
    bases = points_of(ctx, cid, logs)
    inf = torch.tensor([0, 0, 0, 0, 1], dtype=torch.uint8, device="cuda")
    eff = logs[:4] + [0]
    segs = [
        ([0, 0], [s, s]),                                            # the same base under the same scalar, lanes 0 and 1
        ([0, 1], [s, s]),                                            # P and -P under equal scalars
        ([0] + [2] * 62 + [1], [s] + [0] * 62 + [s]),                # cancels across lanes 0 and 63, zero scalars between
        ([4, 2], [s, s2]),                                           # infinity by flag, with a non-zero scalar
        ([3, 2], [0, s2]),                                           # all-zero words, with scalar 0
        ([4], [s]),                                                  # nothing but infinity
        ([0, 2] * 40, [s, s2] * 40),                                 # lanes with two terms each, the same two points repeated
    ]
    offsets, index, scalars = [0], [], []
    for ix, sc in segs:
        index += ix
        scalars += sc
        offsets.append(len(index))
    got, st = run(ctx, cid, bases, inf, offsets, index, scalars)
    assert st == [SEG_OK] * len(segs)
    for j in range(len(segs)):
        assert got[j] == expect(cv, eff, offsets, index, scalars, j), (cid, j)
    assert got[1] is None and got[2] is None and got[5] is None


@pytest.mark.parametrize("cid", [0, 1])
def test_bad_offsets_and_indices_are_statuses(ctx, cid):
    cv = CURVES[cid]
    logs = rand_logs(cv, 4, 12)
    bases = points_of(ctx, cid, logs)
    scalars = rand_logs(cv, 8, 13)
    #                 ok      descends  ok      index == n_bases   ok      ends beyond n_terms
    offsets = [0, 3, 2, 5, 7, 8, 12]
    index = [0, 1, 2, 3, 0, 1, 4, 2]
    got, st = run(ctx, cid, bases, None, offsets, index, scalars)
    assert st == [SEG_OK, SEG_BAD_RANGE, SEG_OK, SEG_BAD_INDEX, SEG_OK, SEG_BAD_RANGE]
    for s in (0, 2, 4):
        assert got[s] is not None and got[s] == expect(cv, logs, offsets, index, scalars, s), (cid, s)
    assert got[1] is None and got[3] is None and got[5] is None
    index[6] = 0xFFFFFFFF
    got2, st2 = run(ctx, cid, bases, None, offsets, index, scalars)
    assert st2 == st and got2 == got


@pytest.mark.parametrize("cid", [0, 1])
def test_term_by_term_against_the_group_law(ctx, cid):
    import ark_plonk_amd as zk
    cv = CURVES[cid]
    L = zk.get_curve(cid).fq_limbs
    logs = rand_logs(cv, 3, 21)
    bases = points_of(ctx, cid, logs)
    pts = [tuple(zk.curves.fq_from_mont(cid, row.reshape(2, L))) for row in bases.cpu().numpy().view(np.uint64)]
    assert all(bo.on_curve(cv, p) for p in pts)
    scalars = [3, cv.r - 2, 5, 1]
    index = [0, 1, 2, 0]
    got, st = run(ctx, cid, bases, None, [0, 3, 4], index, scalars)
    acc = bo.INF
    for t in range(3):
        acc = bo.ec_add(cv, acc, bo.ec_mul(cv, scalars[t], pts[index[t]]))
    assert st == [SEG_OK, SEG_OK] and got == [acc, pts[0]]


def ladder_scalars(cv):
    """256-bit scalars at and above r: the double-and-add walks the integer, so for a base of order r its accumulator passes through
    -q (k = r: the last addition gives infinity), q (k = r + 2: the last addition doubles) and infinity in mid-ladder (k = 2r + 1)"""
    r = cv.r
    sc = [r, r + 1, r + 2, 2 * r, 2 * r + 1, 2 * r + 2, (1 << 256) - 1]
    assert all(r <= k < 1 << 256 for k in sc)
    return sc


@pytest.mark.parametrize("cid", [0, 1])
def test_scalars_at_and_above_the_group_order(ctx, cid):
    """Each such scalar alone in a one-term segment, and in lanes 0, 1 and 63 of 65-term segments (the 65th term is lane 0's second)
    whose other terms are random: (k mod r) P per term"""
    cv = CURVES[cid]
    logs = rand_logs(cv, 11, 31)
    bases = points_of(ctx, cid, logs)
    special = ladder_scalars(cv)
    offsets, index, scalars = [0], [], []
    for j, k in enumerate(special):
        index.append(j % 11)
        scalars.append(k)
        offsets.append(len(index))
    rng = np.random.default_rng(41)
    for s in range(3):
        ix = rng.integers(0, 11, size=65).tolist()
        sc = rand_logs(cv, 65, 50 + s)
        for slot, lane in enumerate((0, 1, 63)):
            sc[lane] = special[(3 * s + slot) % len(special)]
        index += ix
        scalars += sc
        offsets.append(len(index))
    got, st = run(ctx, cid, bases, None, offsets, index, scalars)
    assert st == [SEG_OK] * (len(offsets) - 1)
    for s in range(len(offsets) - 1):
        assert got[s] == expect(cv, logs, offsets, index, scalars, s), (cid, s)
    G = (cv.gx, cv.gy)
    assert got[0] is None and got[3] is None                                     # r P and 2r P
    assert got[1] == bo.ec_mul(cv, logs[1], G) and got[2] == bo.ec_mul(cv, 2 * logs[2] % cv.r, G)


def test_a_base_outside_the_subgroup_takes_the_integer_scalar(ctx):
    """BLS12-381's (0, 2) has order 3 (the point test_from_random_bytes_on_crafted_strings feeds to the cofactor kernel): k P is the
    integer multiple, k mod 3, never (k mod r) P -- the big-int double-and-add on the point itself, the scalar unreduced"""
    import torch
    import ark_plonk_amd as zk
    cid, cv = 0, CURVES[0]
    P3 = (0, 2)
    assert bo.on_curve(cv, P3) and bo.ec_mul(cv, 3, P3) is bo.INF and bo.ec_mul(cv, 2, P3) == (0, cv.q - 2)
    k_q = rand_logs(cv, 1, 33)[0]
    Q = bo.ec_mul(cv, k_q, (cv.gx, cv.gy))
    rows = np.concatenate([zk.curves.fq_to_mont(cid, list(P3)).reshape(1, -1), points_of(ctx, cid, [k_q]).cpu().numpy().view(np.uint64)])
    bases = torch.from_numpy(rows.view(np.int64)).cuda()
    ks = [1, 2, 3, 4, cv.r, (1 << 256) - 1]
    assert sorted({k % 3 for k in ks}) == [0, 1, 2] and cv.r % 3 != 0
    offsets, index, scalars = [0], [], []
    for k in ks:                                             # alone
        index.append(0)
        scalars.append(k)
        offsets.append(len(index))
    for k in ks:                                             # next to a term of the subgroup
        index += [0, 1]
        scalars += [k, 5]
        offsets.append(len(index))
    got, st = run(ctx, cid, bases, None, offsets, index, scalars)
    assert st == [SEG_OK] * (2 * len(ks))
    for j, k in enumerate(ks):
        want = bo.ec_mul(cv, k, P3)
        assert want == [bo.INF, P3, (0, cv.q - 2)][k % 3]
        assert got[j] == want, k
        assert got[len(ks) + j] == bo.ec_add(cv, want, bo.ec_mul(cv, 5, Q)), k


def test_no_segments_null_arguments_and_unknown_curve(ctx):
    import torch
    from ark_plonk_amd import _lib
    f = _lib.lib().zk_msm_g1_segments_dev
    assert f(ctx.handle, 0, 0, None, None, 0, None, 0, None, None, None, None, None) == 0
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    xy = torch.zeros(12, dtype=torch.int64, device="cuda")
    inf = torch.zeros(1, dtype=torch.uint8, device="cuda")
    st = torch.full((1,), 9, dtype=torch.uint8, device="cuda")
    ok = [ctx.handle, 0, 0, None, None, 1, off.data_ptr(), 0, None, None, xy.data_ptr(), inf.data_ptr(), st.data_ptr()]
    assert f(*ok) == 0                                                # one empty segment over no bases
    torch.cuda.synchronize()
    assert inf.cpu().tolist() == [1] and st.cpu().tolist() == [SEG_OK]
    for k in (6, 10, 11, 12):                                         # offsets, the three outputs
        bad = list(ok)
        bad[k] = None
        assert f(*bad) == _lib.ZK_ERR_BAD_ARG, k
    terms = list(ok)
    terms[7] = 1                                                      # a term count with no term arrays
    assert f(*terms) == _lib.ZK_ERR_BAD_ARG
    assert f(*([ctx.handle, 7] + ok[2:])) == _lib.ZK_ERR_BAD_ARG
    assert f(*([None] + ok[1:])) == _lib.ZK_ERR_BAD_ARG
