"""The compact form of the wide partition sort (csort_* in csrc/msm_sort.hip: whole tables of folded 17-bit windows) against the CPU
oracle's Pippenger, limb for limb, through the public calls -- with inputs chosen to break a packed staging record, the slab
recovery of the placement kernel or a run boundary.  Geometries the form does not take (16-bit tables, a 20-bit table, a
window-sharded table: `pre_compact` in csrc/msm_common.cuh refuses them, so they run the psort_* family -- int16 digits and uint8
low bucket bits at 16 bits, int32 and uint16 above) agree with the same oracle.  The 16-bit cases reach every digit kernel of that
window: the two-scalars-per-lane kernel of even lengths over a whole table, and the generic kernel with int16 digits for odd
lengths and window-sharded tables.  Tables of 18, 20 and 21 bits and the window-sharded 17-bit table take skewed scalars too: one
partition holds every reference, so the placement kernel with lob at run time walks several tiles and scans one, two and four
counters per lane.  Several expected points are the point at infinity or a single multiple of one base: that is intended."""
import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib
from oracle import bigint_oracle as bo

pytestmark = pytest.mark.gpu

N_SRS = (1 << 20) + 64
OFFSET = 37


def _limbs(vals):
    return zk.curves.ints_to_limbs([int(v) for v in vals], 4)


def _rand_canonical(rng, n, top_bits=62):
    s = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    s[:, 3] &= np.uint64((1 << top_bits) - 1)
    return s


def scalar_cases(cv, n, seed=1, c=17):
    """name -> (n, 4) canonical scalars.  No GPU needed: the oracle can be run on these anywhere.  c: the window bits of the table the
    skewed cases are cut for (all_equal, one_partition, last_partition are built digit by digit: 2^(c-1) buckets per window, 256
    sort partitions of 2^(c-9))."""
    r = cv.r
    rng = np.random.default_rng(seed)
    nw, half, per_part = 256 // c, 1 << (c - 1), 1 << (c - 9)       # whole windows in 256 bits: 15 of 17 bits, 16 of 16
    out = {}
    out["random"] = _rand_canonical(rng, n)
    # one bucket of every window holds all n references (the workgroup-per-bucket class of the combine)
    k = 0
    for w in range(nw):
        k |= (0x1234 + 77 * w) << (c * w)
    out["all_equal"] = np.tile(_limbs([k]), (n, 1))
    # every digit of every scalar in sort partition 0: |digit| in 1 .. 2^(c-9) (256 at c = 17)
    d = rng.integers(1, per_part + 1, size=(n, nw))
    m = min(n, 4096)
    reps = (n + m - 1) // m
    out["one_partition"] = np.tile(_limbs([sum(int(d[i, w]) << (c * w) for w in range(nw)) for i in range(m)]), (reps, 1))[:n]
    # ... and in the last one (|digit| = 2^(c-1) - 2^(c-9) + 1 .. 2^(c-1): the carry runs through every window; at c = 16 the
    # digit -32768 is the lowest an int16 holds)
    top = [sum((half - int(d[i, w]) + 1) << (c * w) for w in range(nw - 1)) for i in range(m)]
    out["last_partition"] = np.tile(_limbs(top), (reps, 1))[:n]
    # blocks of 128 equal scalars, 16 values: a slab's run inside a partition is longer than a wavefront, the partition itself short
    vals = _limbs([int.from_bytes(rng.bytes(31), "little") for _ in range(16)])
    out["blocks_of_equal"] = vals[(np.arange(n) // 128) % 16]
    out["zeros"] = np.zeros((n, 4), dtype=np.uint64)
    one = np.zeros((n, 4), dtype=np.uint64)
    one[n - 1] = _limbs([r - 5])[0]
    out["single_nonzero_last"] = one
    one = np.zeros((n, 4), dtype=np.uint64)
    one[0] = (1, 0, 0, 0)
    out["single_one_first"] = one
    # the fold's edge: r - 1 -> 1 negated, (r - 1) / 2 stays, (r + 1) / 2 -> (r - 1) / 2 negated
    edge = [r - 1, (r - 1) // 2, (r + 1) // 2, 1, 0, r - 2, (r - 1) // 2 - 1, (r + 1) // 2 + 1]
    out["fold_edges"] = np.tile(_limbs(edge), ((n + 7) // 8, 1))[:n]
    mixed = _rand_canonical(rng, n, 63)        # up to 2^255 > r: a few per cent are reduced below r first, half are folded
    mixed[:: 7] = _limbs([r - 1])[0]
    mixed[3:: 11] = _limbs([(r + 1) // 2])[0]
    if c == 16:
        # No fold at 16 bits, so nothing brings an unreduced scalar below r there, and the ABI asks for canonical scalars: above r the
        # top window can carry out of the 256 bits (bits 240 .. 254 all set, plus a carry).  Same values mod r.
        big = [i for i in range(n) if int(mixed[i, 3]) >= (r >> 192)]
        if big:
            mixed[big] = _limbs([sum(int(mixed[i, j]) << (64 * j) for j in range(4)) % r for i in big])
    out["random_with_edges"] = mixed
    return out


@pytest.fixture(scope="module")
def key17(ctx):
    """2^20 + 64 points k_i G (random 62-bit k_i) with the default table: 17-bit windows, 15 rows"""
    import torch
    cv = zk.get_curve(0)
    g = torch.Generator(device="cuda").manual_seed(1717)
    ks = torch.randint(1, 1 << 62, (N_SRS, 4), dtype=torch.int64, device="cuda", generator=g)
    ks[:, 1:] = 0
    bases = torch.empty((N_SRS, 2 * cv.fq_limbs), dtype=torch.int64, device="cuda")
    ctx.use_torch_stream()
    _lib.check(_lib.lib().zk_g1_fixed_base_batch_dev(ctx.handle, 0, ks.data_ptr(), N_SRS, bases.data_ptr()))
    ck = zk.CommitterKey(bases, 0, ctx).precompute()
    assert ck.table_windows() == 15
    yield ck, bases, bases.cpu().numpy().view(np.uint64)
    ck.close()


def _assert_point(got, exp_xy, exp_inf, tag):
    assert got.infinity == bool(exp_inf), tag
    if not exp_inf:
        assert np.array_equal(got.xy(), exp_xy), tag


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


# 2^13: the smallest length of the table path; + 1; an odd length; lengths that no slab count divides
@pytest.mark.parametrize("n", [1 << 13, (1 << 13) + 1, 100003, 300002])
def test_canonical_cases_against_the_oracle(n, key17, oracle_cpu):
    ck, _, bases_h = key17
    for name, scal in scalar_cases(zk.get_curve(0), n, seed=n).items():
        exp_xy, exp_inf = oracle_cpu.msm_g1(0, bases_h[:n], scal)
        if name == "zeros":
            assert exp_inf
        _assert_point(ck.msm(_dev(scal)), exp_xy, exp_inf, f"{name} n={n}")


@pytest.mark.parametrize("name", ["random_with_edges", "all_equal", "one_partition"])
def test_full_length_at_an_offset_of_a_longer_srs(name, key17, oracle_cpu):
    ck, _, bases_h = key17
    n = 1 << 20
    scal = scalar_cases(zk.get_curve(0), n, seed=20)[name]
    exp_xy, exp_inf = oracle_cpu.msm_g1(0, bases_h[OFFSET:OFFSET + n], scal)
    _assert_point(ck.msm(_dev(scal), base_offset=OFFSET), exp_xy, exp_inf, name)
    exp_xy, exp_inf = oracle_cpu.msm_g1(0, bases_h[:n], scal)
    _assert_point(ck.msm(_dev(scal)), exp_xy, exp_inf, name + " offset 0")


@pytest.mark.parametrize("n", [1 << 13, 65537, 1 << 20])
def test_montgomery_coefficients_against_the_oracle(n, key17, oracle_cpu):
    ck, _, bases_h = key17
    cv = zk.get_curve(0)
    cases = scalar_cases(cv, n, seed=3 * n)
    for name in ("random", "fold_edges", "all_equal", "zeros"):
        mont = oracle_cpu.convert(0, "fr", True, np.ascontiguousarray(cases[name] if name != "random" else cases[name] >> np.uint64(1)))
        exp_xy, exp_inf = oracle_cpu.kzg_commit(0, bases_h, mont)
        _assert_point(ck.commit(_dev(mont)), exp_xy, exp_inf, f"{name} n={n}")


def _oracle_open(oracle_cpu, bases_h, polys, z, chi):
    n = max(p.shape[0] for p in polys)
    comb = np.zeros((n, 4), dtype=np.uint64)
    chi_pow = oracle_cpu.convert(0, "fr", True, np.array([[1, 0, 0, 0]], dtype=np.uint64))
    for p in polys:
        term = oracle_cpu.fr_op(0, "mul", p, np.repeat(chi_pow, p.shape[0], axis=0))
        comb[: p.shape[0]] = oracle_cpu.fr_op(0, "add", comb[: p.shape[0]], term)
        chi_pow = oracle_cpu.fr_op(0, "mul", chi_pow, chi.reshape(1, 4))
    return oracle_cpu.kzg_commit(0, bases_h, oracle_cpu.kzg_witness(0, comb, z))


def _sixteen_jobs(cv, oracle_cpu):
    """Sixteen jobs of mixed lengths: Montgomery commits, canonical jobs and two openings (the second overwrites the witness buffer
    of the first after the first job's scalars were taken)."""
    lens = [1 << 16, (1 << 16) - 3, 1 << 13, 8193, 50001, 1 << 16, 30000]
    names = ["random", "fold_edges", "all_equal", "one_partition", "random_with_edges", "zeros", "last_partition"]
    mont = []
    for ln, nm in zip(lens, names):
        s = scalar_cases(cv, ln, seed=ln + 5)[nm]
        if nm in ("random", "random_with_edges"):
            s = s >> np.uint64(2)
        mont.append(oracle_cpu.convert(0, "fr", True, np.ascontiguousarray(s)))
    canon = [scalar_cases(cv, 40001, seed=9)["random_with_edges"], scalar_cases(cv, 1 << 14, seed=10)["single_nonzero_last"]]
    return mont, canon


def _run_round(ck, mont, canon, z, chi):
    d_m = [_dev(m) for m in mont]
    d_c = [_dev(c) for c in canon]
    ck.commit_begin(d_m[:4])
    ck.open_begin(d_m[:3], z, chi)
    ck.commit_begin(d_c, canonical=[True, True])
    ck.commit_begin(d_m[4:])
    ck.open_begin(d_m[3:], z, chi)
    ck.commit_begin(d_m[:4][::-1])
    assert ck.commit_begin([d_c[0]], canonical=[True]) == 16
    return ck.round_end()


def test_sixteen_job_deferred_round_and_the_same_under_a_memory_budget(ctx, key17, oracle_cpu):
    ck, _, bases_h = key17
    cv = zk.get_curve(0)
    mont, canon = _sixteen_jobs(cv, oracle_cpu)
    z = oracle_cpu.convert(0, "fr", True, _limbs(bo.seeded_scalars(bo.CURVES[0], 1, 1)))[0]
    chi = oracle_cpu.convert(0, "fr", True, _limbs(bo.seeded_scalars(bo.CURVES[0], 2, 1)))[0]
    want = [oracle_cpu.kzg_commit(0, bases_h, m) for m in mont[:4]]
    want.append(_oracle_open(oracle_cpu, bases_h, mont[:3], z, chi))
    want += [oracle_cpu.msm_g1(0, bases_h[: c.shape[0]], c) for c in canon]
    want += [oracle_cpu.kzg_commit(0, bases_h, m) for m in mont[4:]]
    want.append(_oracle_open(oracle_cpu, bases_h, mont[3:], z, chi))
    want += want[:4][::-1]
    want.append(want[5])
    assert len(want) == 16
    ctx1 = zk.Context(ctx.device)
    ctx1.use_torch_stream()
    ck1 = ck.with_ctx(ctx1)
    got = _run_round(ck1, mont, canon, z, chi)
    for k, (pt, (exp_xy, exp_inf)) in enumerate(zip(got, want)):
        _assert_point(pt, exp_xy, exp_inf, f"job {k}")
    st0 = ctx1.round_mem_stats()
    ctx1.close()
    assert st0["early_closes"] == 0
    # four average sets' worth of memory: the round closes early and the sets of closed jobs are adopted by jobs of other lengths
    ctx2 = zk.Context(ctx.device)
    ctx2.use_torch_stream()
    ck2 = ck.with_ctx(ctx2)
    try:
        ctx2.set_option("round_mem_limit_mb", max(1, (4 * (st0["set_bytes"] // 16)) >> 20) + 1)
        got2 = _run_round(ck2, mont, canon, z, chi)
        assert ctx2.round_mem_stats()["early_closes"] >= 1
        assert got2 == got
        assert _run_round(ck2, mont, canon, z, chi) == got        # again: the sets exist now, some adopted from shorter jobs
    finally:
        ctx2.set_option("round_mem_limit_mb", 0)
    ctx2.close()


def _small_key(ctx, cid, n, seed):
    import torch
    cv = zk.get_curve(cid)
    g = torch.Generator(device="cuda").manual_seed(seed)
    ks = torch.randint(1, 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    ks[:, 1:] = 0
    bases = torch.empty((n, 2 * cv.fq_limbs), dtype=torch.int64, device="cuda")
    ctx.use_torch_stream()
    _lib.check(_lib.lib().zk_g1_fixed_base_batch_dev(ctx.handle, cid, ks.data_ptr(), n, bases.data_ptr()))
    return bases, bases.cpu().numpy().view(np.uint64)


def test_bn254_sixteen_bit_table_keeps_its_kernels_and_agrees(ctx, oracle_cpu):
    n = 1 << 14
    bases, bases_h = _small_key(ctx, 1, n, 254)
    ck = zk.CommitterKey(bases, 1, ctx).precompute()
    assert ck.table_windows() == 16
    cv = zk.get_curve(1)
    rng = np.random.default_rng(254)
    scal = _rand_canonical(rng, n, 60)
    scal[::5] = _limbs([cv.r - 1])[0]
    scal[1::9] = _limbs([(cv.r + 1) // 2])[0]
    exp_xy, exp_inf = oracle_cpu.msm_g1(1, bases_h, scal)
    _assert_point(ck.msm(_dev(scal)), exp_xy, exp_inf, "bn254 c=16")
    ck.close()


def test_twenty_bit_table_and_window_sharded_rows_keep_their_kernels_and_agree(ctx, oracle_cpu):
    """c = 20 (psort_* with int32 digits and 2048 buckets per partition) and a 17-bit table of which a rank owns every other row (the digit kernel
    walks all windows and keeps the owned ones): neither is the compact form's geometry."""
    n = 1 << 14
    bases, bases_h = _small_key(ctx, 0, n, 2017)
    cv = zk.get_curve(0)
    scal = scalar_cases(cv, n, seed=2017)["random_with_edges"]
    exp_xy, exp_inf = oracle_cpu.msm_g1(0, bases_h, scal)
    ck = zk.CommitterKey(bases, 0, ctx).precompute(20)
    assert ck.table_windows() == 13
    _assert_point(ck.msm(_dev(scal)), exp_xy, exp_inf, "c=20")
    ck.close()
    parts = []
    for g in range(2):
        ckw = zk.CommitterKey(bases, 0, ctx).precompute(17, rows=(g, 2))
        assert ckw.table_rows() == (g, 2, 8 - g) and ckw.table_windows() == 15
        parts.append(ckw.commit_batch_partial([_dev(scal)], canonical=[True]))
        ckw.close()
    _assert_point(zk.sum_partials_batch(np.stack(parts), 0)[0], exp_xy, exp_inf, "c=17, rows (g, 2)")
    # the same scalars over the whole 17-bit table: the compact form
    ck = zk.CommitterKey(bases, 0, ctx).precompute(17)
    _assert_point(ck.msm(_dev(scal)), exp_xy, exp_inf, "c=17 whole")
    ck.close()


@pytest.fixture(scope="module")
def bases14(ctx):
    """2^14 points k_i G on BLS12-381, shared by the tables below"""
    return _small_key(ctx, 0, 1 << 14, 1821)


# What make_geom (csrc/msm_common.cuh) gives for the 255-bit r of BLS12-381: 255 // c + 1 windows -- the top bits of r - 1 plus a carry
# stay far below 2^(c-1) in the last one -- and the fold to 254 bits would need ceil(254 / c) windows, which is no fewer at these
# widths (15, 13, 13), so it is not taken.  NB = 2^(c-9) buckets per partition: 512, 2048, 4096 for the 1024 lanes of psort_final.
WIDE_TABLE_WINDOWS = {18: 15, 20: 13, 21: 13}


@pytest.fixture(scope="module", params=[18, 20, 21])
def key_wide(request, ctx, bases14):
    c = request.param
    bases, bases_h = bases14
    ck = zk.CommitterKey(bases, 0, ctx).precompute(c)
    assert ck.table_windows() == WIDE_TABLE_WINDOWS[c] == 255 // c + 1
    yield c, ck, bases_h
    ck.close()


@pytest.mark.parametrize("n", [1 << 13, (1 << 13) + 1])
def test_wide_tables_with_skewed_partitions_against_the_oracle(n, key_wide, oracle_cpu):
    """psort_scatter / psort_final with lob at run time beyond the few hundred references per partition that random scalars give at
    2^14 points: one counter per lane with idle lanes (c = 18), two (20) and four (21, the 144 KiB LDS maximum), and with
    one_partition ~12 * n references in partition 0 -- six tiles of PS_TILE, the multi-tile loop of the placement kernel."""
    c, ck, bases_h = key_wide
    cases = scalar_cases(zk.get_curve(0), n, seed=c * n, c=c)
    for name in ("one_partition", "last_partition", "all_equal", "random_with_edges"):
        exp_xy, exp_inf = oracle_cpu.msm_g1(0, bases_h[:n], cases[name])
        _assert_point(ck.msm(_dev(cases[name])), exp_xy, exp_inf, f"{name} n={n} c={c}")


@pytest.mark.parametrize("name", ["one_partition", "last_partition"])
def test_window_sharded_seventeen_bit_rows_with_skewed_partitions(name, ctx, bases14, oracle_cpu):
    """The window-sharded 17-bit table (rows (g, 2): not the compact form, so psort_* with uint16 low bits and lob = 8) with all the
    references of the owned rows in the first or the last partition."""
    bases, bases_h = bases14
    n = (1 << 13) + 1
    scal = scalar_cases(zk.get_curve(0), n, seed=1702)[name]
    exp_xy, exp_inf = oracle_cpu.msm_g1(0, bases_h[:n], scal)
    parts = []
    for g in range(2):
        ckw = zk.CommitterKey(bases[:n], 0, ctx).precompute(17, rows=(g, 2))
        assert ckw.table_rows() == (g, 2, 8 - g) and ckw.table_windows() == 15
        parts.append(ckw.commit_batch_partial([_dev(scal)], canonical=[True]))
        ckw.close()
    _assert_point(zk.sum_partials_batch(np.stack(parts), 0)[0], exp_xy, exp_inf, f"{name}, c=17, rows (g, 2)")


@pytest.fixture(scope="module", params=[0, 1], ids=["bls12_381", "bn254"])
def key16(request, ctx):
    """2^14 points k_i G with a whole table of 16-bit windows (16 rows): what every table below 2^19 points is"""
    cid = request.param
    bases, bases_h = _small_key(ctx, cid, 1 << 14, 1600 + cid)
    ck = zk.CommitterKey(bases, cid, ctx).precompute(16)
    assert ck.table_windows() == 16 and ck.table_rows() == (0, 1, 16)
    yield cid, ck, bases, bases_h
    ck.close()


def _mont(oracle_cpu, cid, scal):
    return oracle_cpu.convert(cid, "fr", True, np.ascontiguousarray(scal))


# 2^13: the smallest length of the table path, even (two scalars per lane in the digit kernel); + 1: odd (the generic digit kernel)
@pytest.mark.parametrize("form", ["canonical", "montgomery"])
@pytest.mark.parametrize("n", [1 << 13, (1 << 13) + 1])
def test_sixteen_bit_table_even_and_odd_lengths_against_the_oracle(n, form, key16, oracle_cpu):
    cid, ck, _, bases_h = key16
    cases = scalar_cases(zk.get_curve(cid), n, seed=16 * n + cid, c=16)
    for name in ("random_with_edges", "all_equal", "one_partition", "last_partition", "zeros"):
        scal = cases[name]
        if form == "canonical":
            exp_xy, exp_inf = oracle_cpu.msm_g1(cid, bases_h[:n], scal)
            got = ck.msm(_dev(scal))
        else:
            if name == "random_with_edges":
                scal = scal >> np.uint64(2)         # (every limb: below r of either curve, as into_mont asks)
            mont = _mont(oracle_cpu, cid, scal)
            exp_xy, exp_inf = oracle_cpu.kzg_commit(cid, bases_h, mont)
            got = ck.commit(_dev(mont))
        if name == "zeros":
            assert exp_inf
        _assert_point(got, exp_xy, exp_inf, f"{name} n={n} {form} curve {cid}")


def test_sixteen_bit_window_sharded_rows_agree(ctx, key16, oracle_cpu):
    """A 16-bit table of which a rank owns every other row: the generic digit kernel walks all 16 windows and keeps the owned rows as
    int16 digits (an odd length, so that nothing but that kernel could take it either way)."""
    cid, _, bases, bases_h = key16
    n = (1 << 13) + 1
    scal = scalar_cases(zk.get_curve(cid), n, seed=2016 + cid, c=16)["random_with_edges"]
    exp_xy, exp_inf = oracle_cpu.msm_g1(cid, bases_h[:n], scal)
    parts = []
    for g in range(2):
        ckw = zk.CommitterKey(bases[:n], cid, ctx).precompute(16, rows=(g, 2))
        assert ckw.table_rows() == (g, 2, 8) and ckw.table_windows() == 16
        parts.append(ckw.commit_batch_partial([_dev(scal)], canonical=[True]))
        ckw.close()
    _assert_point(zk.sum_partials_batch(np.stack(parts), cid)[0], exp_xy, exp_inf, f"c=16, rows (g, 2), curve {cid}")


def test_sixteen_bit_deferred_round_of_mixed_lengths(key16, oracle_cpu):
    """Four jobs of one deferred round over the whole 16-bit table, even and odd lengths, Montgomery and canonical: one launch of the
    scatter and of the placement kernel (job = blockIdx.y) over jobs whose slabs differ in length."""
    cid, ck, _, bases_h = key16
    cv = zk.get_curve(cid)
    lens = [8192, 8193, 12001, 1 << 14]
    scal = [scalar_cases(cv, ln, seed=ln + cid, c=16)[nm] for ln, nm in zip(lens, ["random", "last_partition", "random_with_edges", "one_partition"])]
    mont = [_mont(oracle_cpu, cid, scal[0] >> np.uint64(2)), _mont(oracle_cpu, cid, scal[1])]           # (below r of either curve)
    want = [oracle_cpu.kzg_commit(cid, bases_h, m) for m in mont] + [oracle_cpu.msm_g1(cid, bases_h[: s.shape[0]], s) for s in scal[2:]]
    ck.commit_begin([_dev(m) for m in mont])
    assert ck.commit_begin([_dev(s) for s in scal[2:]], canonical=[True, True]) == 4
    for k, (pt, (exp_xy, exp_inf)) in enumerate(zip(ck.round_end(), want)):
        _assert_point(pt, exp_xy, exp_inf, f"job {k} of {lens[k]} curve {cid}")
