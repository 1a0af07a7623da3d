"""BASELINE.json configs that round 1 left untested under -m gpu (VERDICT.md "configs untested"), each checking a RESULT:
  config 3  MSM at 2^22 on the window-table path and on the per-window path (KZG identity), and the same MSM cut into 8 point
            shards -> zk_kzg_round_batch_partial_dev per shard -> zk_g1_sum_partials_batch == the single result
  config 4  BN254: NTT at 2^18 and 2^20 (4n) against the C++ restatement, all four kinds; window-table MSM at 2^18
  config 5  the Poseidon size point: plonk-hashing/src/lib.rs:1-12 is empty, so only a padded size exists.  Assumption
            (DESIGN.md section 5): a width-3 Poseidon permutation = 8 full rounds x 12 gates + 57 partial rounds x 6 gates = 438
            gates; 2^16 hashes -> 28.7 M gates -> n = 2^25, 4n = 2^27.  NTT round trips at 2^25 and 2^27 and an MSM identity
            at 2^25 (window table: 64 GiB of the 288 GB card).
plus the window-table MSM with every table window c the library accepts (16..21) against c = 16 and the CPU restatement."""
import numpy as np
import pytest

import ark_plonk_amd as zk
import large_ref as lr
from conftest import assert_is_scalar_times_g, srs_from_powers, sum_scalar_times_powers, tau_powers
from oracle import bigint_oracle as bo

pytestmark = pytest.mark.gpu


def _rand_scalars(n, seed, bits62=61):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    s[:, 3] &= np.uint64((1 << bits62) - 1)       # < 2^253: canonical for both curves
    return s


def _full_range_scalars(cid, n, seed):
    """Scalars uniform over [0, r), the first 4096 in [r - 2^64, r): bits 253 and 254 and the top window's upper digits in use."""
    s = lr.full_range(cid, n, seed)
    s[:4096] = lr.near_r(cid, 4096, seed + 1)
    return s


def test_config3_msm_2_22_table_plain_and_8_shards(ctx, oracle_cpu):
    import torch
    cid, log_n = 0, 22
    n = 1 << log_n
    pw_c, pw_m = tau_powers(oracle_cpu, cid, n)
    bases = srs_from_powers(ctx, cid, pw_c)
    scal = _rand_scalars(n, 22)
    k = sum_scalar_times_powers(oracle_cpu, cid, scal, pw_m)
    d_s = torch.from_numpy(scal.view(np.int64)).cuda()
    full = _full_range_scalars(cid, n, 0x3F22)
    k_full = sum_scalar_times_powers(oracle_cpu, cid, full, pw_m)
    d_full = torch.from_numpy(full.view(np.int64)).cuda()
    ck = zk.CommitterKey(bases, cid, ctx)
    plain = ck.msm(d_s)                                   # per-window path
    assert_is_scalar_times_g(plain, k, cid)
    plain_full = ck.msm(d_full)
    assert_is_scalar_times_g(plain_full, k_full, cid)
    ck.precompute()
    tab = ck.msm(d_s)                                     # window-table path (8 GiB table)
    assert tab == plain
    assert ck.msm(d_full) == plain_full
    ck.close()
    del d_full
    # 8 point shards, as 8 ranks would hold them: every shard its own SRS slice + table, partial over its scalar slice
    G = 8
    parts = []
    for g in range(G):
        lo, hi = g * n // G, (g + 1) * n // G
        cks = zk.CommitterKey(bases[lo:hi].contiguous(), cid, ctx).precompute()
        parts.append(cks.commit_batch_partial([d_s[lo:hi]], canonical=[True]))     # (1, 3L) Jacobian
        cks.close()
    got = zk.sum_partials_batch(np.stack(parts), cid)[0]   # (ranks, jobs = 1, 3L)
    assert got == plain
    # 8 WINDOW shards (BASELINE.json north_star: "shards its windows/buckets across GPUs"): every rank registers the whole SRS, builds
    # the table rows of the windows g, g + 8 (2 of the 15 rows; rank 7: one) and sums all n scalars' digits of those windows.  The
    # partials go through both forms of the exchange: host Jacobian partials, and the device form (the last reduction kernel writes
    # the job's virtual-window sums into the tensor the all-gather would send; zk_g1_sum_winsums_dev adds the ranks' element-wise)
    parts, dev_parts = [], []
    pw = None
    for g in range(G):
        ckw = zk.CommitterKey(bases, cid, ctx).precompute(rows=(g, G))
        assert ckw.table_rows() == (g, G, (15 - g + G - 1) // G) and ckw.table_windows() == 15
        parts.append(ckw.commit_batch_partial([d_s], canonical=[True]))
        pw = ckw.winsums_dev_words()
        buf = torch.zeros((1, pw), dtype=torch.int64, device="cuda")
        ckw.commit_begin([d_s], canonical=[True])
        ckw.round_end_winsums_dev(buf, 1)
        dev_parts.append(buf)
        if g == G - 1:
            got_dev = ckw.sum_winsums_dev(torch.stack(dev_parts).reshape(G, pw).contiguous(), G, 1)[0]
        ckw.close()
    assert zk.sum_partials_batch(np.stack(parts), cid)[0] == plain
    assert got_dev == plain


@pytest.mark.parametrize("log_n", [18, 20])
def test_config4_bn254_ntt_vs_oracle(log_n, ctx, oracle_cpu):
    import torch
    cid = 1
    n = 1 << log_n
    x = _rand_scalars(n, 40 + log_n, bits62=59)           # Montgomery residues < 2^251 < r (BN254 r ~ 2^253.6)
    d = torch.from_numpy(x.view(np.int64)).cuda()
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    for kind, name in enumerate(("fft", "ifft", "coset_fft", "coset_ifft")):
        inp = d if kind != 2 else d[: n // 4]              # coset_fft as the prover uses it: n/4 coefficients on the 4x domain
        got = getattr(dom, name)(inp).cpu().numpy().view(np.uint64)
        exp = oracle_cpu.ntt(cid, kind, log_n, x if kind != 2 else x[: n // 4])
        assert np.array_equal(got, exp), name


def test_config4_bn254_table_msm_2_18(ctx, oracle_cpu):
    import torch
    cid, n = 1, 1 << 18
    pw_c, pw_m = tau_powers(oracle_cpu, cid, n)
    bases = srs_from_powers(ctx, cid, pw_c)
    scal = _rand_scalars(n, 418, bits62=59)
    k = sum_scalar_times_powers(oracle_cpu, cid, scal, pw_m)
    full = _full_range_scalars(cid, n, 0x3F18)
    k_full = sum_scalar_times_powers(oracle_cpu, cid, full, pw_m)
    ck = zk.CommitterKey(bases, cid, ctx).precompute()
    got = ck.msm(torch.from_numpy(scal.view(np.int64)).cuda())
    got_full = ck.msm(torch.from_numpy(full.view(np.int64)).cuda())
    ck.close()
    assert_is_scalar_times_g(got, k, cid)
    assert_is_scalar_times_g(got_full, k_full, cid)


def test_table_msm_full_range_scalars_2_20(ctx, oracle_cpu):
    """BLS12-381, 2^20 points on the window-table path (default window), scalars over the whole of [0, r)."""
    import torch
    cid, n = 0, 1 << 20
    pw_c, pw_m = tau_powers(oracle_cpu, cid, n)
    bases = srs_from_powers(ctx, cid, pw_c)
    full = _full_range_scalars(cid, n, 0x3F20)
    k_full = sum_scalar_times_powers(oracle_cpu, cid, full, pw_m)
    ck = zk.CommitterKey(bases, cid, ctx).precompute()
    got = ck.msm(torch.from_numpy(full.view(np.int64)).cuda())
    ck.close()
    assert_is_scalar_times_g(got, k_full, cid)


def test_config5_poseidon_size_point_2_25(ctx, oracle_cpu):
    """n = 2^25 (see the module docstring for the gate-count assumption): coset round trip at 4n = 2^27 (4 GiB per vector),
    fft/ifft round trip at n, and the KZG identity for an MSM of 2^25 points on the window-table path."""
    import torch
    cid, log_n = 0, 25
    n = 1 << log_n
    g = torch.Generator(device="cuda").manual_seed(25)
    a = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    dom4 = zk.Radix2EvaluationDomain.new(4 * n, cid, ctx)
    ev = dom4.coset_fft(a)                                 # n coefficients zero-extended to 4n (quotient_poly.rs:72)
    dom4.coset_ifft_in_place(ev)
    assert torch.equal(ev[:n], a) and not bool(ev[n:].any())
    del ev
    f = dom.fft(a)
    dom.ifft_in_place(f)
    assert torch.equal(f, a)
    del f, a, dom4
    torch.cuda.empty_cache()
    pw_c, pw_m = tau_powers(oracle_cpu, cid, n)
    bases = srs_from_powers(ctx, cid, pw_c)
    del pw_c
    scal = _rand_scalars(n, 2525)
    k = sum_scalar_times_powers(oracle_cpu, cid, scal, pw_m)
    del pw_m
    ck = zk.CommitterKey(bases, cid, ctx).precompute()
    del bases
    got = ck.msm(torch.from_numpy(scal.view(np.int64)).cuda())
    ck.close()
    assert_is_scalar_times_g(got, k, cid)


def test_config5_deferred_schedule_2_25(ctx):
    """Config 5's size point through the DEFAULT form of the per-proof schedule (eleven PC calls collected in five deferred rounds,
    sixteen jobs in the last one): round 5 returned ZK_ERR_OOM here -- 52.8 GiB of table + 87 GiB of the schedule's own polynomials +
    194 GiB of job buffer sets.  With the digits parked in the reference buffer, one staging area per round and at most eight rounds
    of lanes per job the sets hold about 41 GB, and a begin that still found no room would close the queued jobs early
    instead of failing.  The 29 points equal those of the blocking form (every call waits; at most seven jobs alive), proof for proof."""
    import torch
    from ark_plonk_amd.prover_schedule import ProofSchedule
    from test_deferred_gpu import _ck
    import gc
    gc.collect()
    torch.cuda.empty_cache()                      # this test needs 255 of the card's 288 GiB: nothing cached by earlier tests may linger
    free, total = torch.cuda.mem_get_info()
    if free < 258 << 30:                          # a smaller card, or one shared with another tenant: the size point does not fit at all
        pytest.skip(f"n = 2^25 needs 255 GiB of device memory; {free >> 30} of {total >> 30} GiB free")
    cv = zk.get_curve(0)
    log_n = 25
    ck = _ck(ctx, cv, 1 << log_n, seed=2525).precompute()
    assert ck.table_window_bits() == 20
    blocking = ProofSchedule(log_n, ctx, ck, cv, defer_calls=False)
    want = blocking.run_once(proof_id=0)
    del blocking
    torch.cuda.empty_cache()
    deferred = ProofSchedule(log_n, ctx, ck, cv)
    assert deferred.defer_calls
    got = deferred.run_once(proof_id=0)
    st = ctx.round_mem_stats()
    assert len(got) == 29 and got == want
    assert len(set(pt.xy().tobytes() for pt in got)) == 20          # 29 MSMs over 20 distinct polynomials (prover.rs:569-607 commits 9 of them again)
    assert st["set_bytes"] < 80 << 30, st                                                     # 194 GiB before the diet
    print("2^25 deferred:", {k: (v >> 20) for k, v in st.items() if k != "early_closes"}, "MiB; early closes", st["early_closes"])
    del deferred
    torch.cuda.empty_cache()
    ck.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_table_window_sizes_agree(cid, ctx, oracle_cpu):
    """zk_srs_precompute_ex: every table window c in 16..21 gives the commitment of the per-window path and of the CPU
    restatement -- uniform, heavily skewed (the benchmark circuit's repeated small wire values) and sparse scalars, odd and
    threshold lengths, single MSMs and round batches."""
    import torch
    n = 1 << 14
    cv = bo.CURVES[cid]
    pw_c, _ = tau_powers(oracle_cpu, cid, n)
    bases = srs_from_powers(ctx, cid, pw_c)
    bases_h = bases.cpu().numpy().view(np.uint64)
    rng = np.random.default_rng(7 + cid)
    polys = []
    for ln, mode in ((n, "uniform"), (n - 1, "skew"), (8193, "sparse"), (n, "max"), (8192, "uniform"), (n, "half")):
        p = _rand_scalars(ln, int(rng.integers(1 << 30)), bits62=59)
        if mode == "skew":
            small = zk.curves.fr_to_mont(cid, [6, 7, cv.r - 20, 1])
            p[: 3 * ln // 4] = np.tile(small, (ln // 4 + 1, 1))[: 3 * ln // 4]
        elif mode == "sparse":
            p[rng.random(ln) < 0.95] = 0
        elif mode == "max":
            p[:] = zk.curves.fr_to_mont(cid, [cv.r - 1])[0]
        elif mode == "half":
            # around (r - 1) / 2, where the 15-window form of the c = 17 table folds k to r - k (MsmGeom::neg), and the extremes
            h = (cv.r - 1) // 2
            edge = [h - 1, h, h + 1, h + 2, 1, cv.r - 1, cv.r - 2, (1 << (cv.r.bit_length() - 1)), (1 << (cv.r.bit_length() - 1)) - 1, 0]
            p[: 4 * len(edge)] = np.tile(zk.curves.fr_to_mont(cid, edge), (4, 1))
        polys.append(p)
    exp = [oracle_cpu.kzg_commit(cid, bases_h, p) for p in polys]
    d_polys = [torch.from_numpy(p.view(np.int64)).cuda() for p in polys]
    for c in (16, 17, 18, 19, 20, 21):
        ck = zk.CommitterKey(bases, cid, ctx).precompute(c)
        assert ck.table_window_bits() == c and 12 <= ck.table_windows() <= 16
        if c == 17:
            assert ck.table_windows() == 15      # BLS12-381: 16 without the folded scalars; BN254's 254 bits fit 15 either way
        batch = ck.commit_batch(d_polys)
        single = [ck.commit(p) for p in d_polys[:2]]
        ck.close()
        for j, (pt, (xy, inf)) in enumerate(zip(batch, exp)):
            assert pt.infinity == bool(inf) and np.array_equal(pt.xy(), xy), (c, j)
        assert single == batch[:2]


def test_folded_scalars_accept_unreduced_input(ctx, oracle_cpu):
    """The ABI asks for canonical scalars.  Where a table folds k to r - k (BLS12-381 at c = 17: `MsmGeom::neg`) the fold needs k < r,
    so that path reduces an unreduced scalar first instead of producing garbage: any k < 2^256 gives (k mod r) * P there.  (Paths
    without the fold keep the contract as it is: canonical scalars only.)"""
    import torch
    cid = 0
    n = 1 << 13
    cv = bo.CURVES[cid]
    pw_c, _ = tau_powers(oracle_cpu, cid, n)
    bases = srs_from_powers(ctx, cid, pw_c)
    bases_h = bases.cpu().numpy().view(np.uint64)
    rng = np.random.default_rng(17 + cid)
    for c, top in ((17, 256),):
        vals = [int.from_bytes(rng.bytes(32), "little") >> (256 - top) for _ in range(n)]     # uniform below 2^top: mostly >= r
        vals[:6] = [cv.r, cv.r + 1, 2 * cv.r - 1, 2 * cv.r, (1 << top) - 1, cv.r - 1]
        raw = zk.curves.ints_to_limbs(vals, 4)
        red = zk.curves.ints_to_limbs([v % cv.r for v in vals], 4)
        exp_xy, exp_inf = oracle_cpu.msm_g1(cid, bases_h, red)
        ck = zk.CommitterKey(bases, cid, ctx).precompute(c)
        got = ck.msm(torch.from_numpy(raw.view(np.int64)).cuda())
        ck.close()
        assert got.infinity == bool(exp_inf) and np.array_equal(got.xy(), exp_xy), c


def test_table_window_20_identity_2_20(ctx, oracle_cpu):
    import torch
    cid, n = 0, 1 << 20
    pw_c, pw_m = tau_powers(oracle_cpu, cid, n)
    bases = srs_from_powers(ctx, cid, pw_c)
    scal = _rand_scalars(n, 2020)
    scal[: n // 2] = np.tile(np.array([[6, 0, 0, 0], [7, 0, 0, 0]], dtype=np.uint64), (n // 4, 1))     # half the points in two buckets
    k = sum_scalar_times_powers(oracle_cpu, cid, scal, pw_m)
    ck = zk.CommitterKey(bases, cid, ctx).precompute(20)
    got = ck.msm(torch.from_numpy(scal.view(np.int64)).cuda())
    ck.close()
    assert_is_scalar_times_g(got, k, cid)


# ---- size edges: what a caller gets at the first sizes the round-3 library refused
def test_ntt_four_passes_2_28(ctx, oracle_cpu):
    """log N = 28 needs a fourth pass (three passes end at 2^27).  The reference admits any domain up to the field's two-adicity
    (prover.rs:169-173, error.rs:14-21).  Checked against the three-pass transform (itself checked against the CPU restatement):
    the 2^28-point fft of 2^20 coefficients, read at every 256th point, IS their 2^20-point fft -- e[256 k] = sum_j a_j
    w_{2^28}^(256 k j) = sum_j a_j w_{2^20}^(k j) -- and likewise on the coset; the classes 256 k + t, t != 0, against the CPU
    restatement through the same identity with twisted coefficients; then full-length round trips of all four kinds
    (8 GiB per vector, in place)."""
    import torch
    cid = 0
    g = torch.Generator(device="cuda").manual_seed(28)
    a = torch.randint(0, 1 << 62, (1 << 20, 4), dtype=torch.int64, device="cuda", generator=g)
    d20 = zk.Radix2EvaluationDomain.new(1 << 20, cid, ctx)
    d28 = zk.Radix2EvaluationDomain.new(1 << 28, cid, ctx)
    for name in ("fft", "coset_fft"):
        big = getattr(d28, name)(a)
        small = getattr(d20, name)(a)
        assert big.shape[0] == 1 << 28 and torch.equal(big[::256], small), name
        del big, small
    # four residue classes besides t = 0: e[256 k + t] = [coset_]fft_{2^20}(f_j w_{2^28}^(t j))_k, on full-range coefficients, each
    # class against one 2^20-point transform of the CPU restatement
    f = lr.full_range(cid, 1 << 20, 0x2828)
    d_f = torch.from_numpy(f.view(np.int64)).cuda()
    for kind, name in ((0, "fft"), (2, "coset_fft")):
        big = getattr(d28, name)(d_f)
        for t in (1, 128, 255, int(np.random.default_rng(28 + kind).integers(2, 255))):
            got = big[t::256].cpu().numpy().view(np.uint64)
            assert np.array_equal(got, lr.decimated(oracle_cpu, cid, kind, 28, 20, f, t)), (name, t)
        del big
    x = torch.randint(0, 1 << 62, (1 << 28, 4), dtype=torch.int64, device="cuda", generator=g)
    y = x.clone()
    d28.fft_in_place(y)
    assert not torch.equal(y, x)
    d28.ifft_in_place(y)
    assert torch.equal(y, x)
    d28.coset_fft_in_place(y)
    d28.coset_ifft_in_place(y)
    assert torch.equal(y, x)
    del x, y
    torch.cuda.empty_cache()
    # beyond the two-adicity: the reference's Error::InvalidEvalDomainSize
    assert zk.Radix2EvaluationDomain.new(1 << 33, cid, ctx) is None         # `GeneralEvaluationDomain::new` returns None there too


def test_msm_beyond_the_table_path_limit(ctx, oracle_cpu):
    """A table-path reference holds 26 bits of point index: MSMs of more than 2^26 points over an SRS WITH a table run the
    per-window path inside the same call instead of returning ZK_ERR_UNSUPPORTED (round 3).  The dispatch is exercised with the
    limit lowered through its test hook (a real 2^26-point table is 130 GiB): same commitment on both sides of the limit, single
    MSMs, blocking batches and deferred rounds."""
    import torch
    cid = 0
    n = (1 << 15) + 2
    pw_c, pw_m = tau_powers(oracle_cpu, cid, n)
    bases = srs_from_powers(ctx, cid, pw_c)
    scal = _rand_scalars(n, 2626)
    k = sum_scalar_times_powers(oracle_cpu, cid, scal, pw_m)
    d_s = torch.from_numpy(scal.view(np.int64)).cuda()
    ck = zk.CommitterKey(bases, cid, ctx).precompute()
    ctx.profile(1)
    ctx.profile_reset()
    want = ck.msm(d_s)                                            # table path
    assert ctx.profile_get("msm_accumulate_jobs")[1] == 1
    assert_is_scalar_times_g(want, k, cid)
    try:
        ctx.set_option("pre_max_log_n", 15)                            # n = 2^15 + 2 is now beyond the limit
        ctx.profile_reset()
        assert ck.msm(d_s) == want
        assert ck.commit_batch([d_s, d_s[: 1 << 14]], canonical=[True, True])[0] == want
        ck.commit_begin([d_s], canonical=[True])
        ck.commit_begin([d_s[: 1 << 14]], canonical=[True])           # this one still takes the table path
        got = ck.round_end(2)
        assert got[0] == want
        assert ctx.profile_get("msm_accumulate_jobs")[1] == 2          # only the two short jobs went through the merged table launch
        ctx.profile(0)
    finally:
        ctx.set_option("pre_max_log_n", 0)
        ctx.profile(0)
    ck.close()


def test_msm_2_26_plus_2_points_per_window_path(ctx, oracle_cpu):
    """The first size past the table path's limit at its real value: 2^26 + 2 points (6.4 GiB of bases) through zk_msm_g1_srs_dev --
    the per-window path, 16 windows x 67 M references -- against the KZG identity MSM(s, tau^i G) = (sum s_i tau^i) G."""
    import torch
    cid = 0
    n = (1 << 26) + 2
    pw_c, pw_m = tau_powers(oracle_cpu, cid, n)
    bases = srs_from_powers(ctx, cid, pw_c)
    del pw_c
    scal = _rand_scalars(n, 262626)
    k = sum_scalar_times_powers(oracle_cpu, cid, scal, pw_m)
    del pw_m
    ck = zk.CommitterKey(bases, cid, ctx)
    del bases
    got = ck.msm(torch.from_numpy(scal.view(np.int64)).cuda())
    ck.close()
    assert_is_scalar_times_g(got, k, cid)


@pytest.mark.parametrize("cid,log_n,G", [(0, 14, 3), (1, 14, 3), (1, 15, 5), (0, 19, 4)])
def test_window_shards_small_both_curves(cid, log_n, G, ctx, oracle_cpu):
    """Window-sharded tables on both curves and both digit paths (c = 16 below 2^19 points: int16 digits, 16 windows; c = 17 at 2^19:
    folded scalars, 15 windows), with a rank count that does not divide the windows: the G partials -- host form and device form
    (BN254's partial is 192 bytes) -- add up to the commitment of the whole table and of the CPU restatement; a vector too short for
    the table path is computed by the owner of window 0 only."""
    import torch
    n = 1 << log_n
    pw_c, pw_m = tau_powers(oracle_cpu, cid, n)
    bases = srs_from_powers(ctx, cid, pw_c)
    rng = np.random.default_rng(1000 + 10 * log_n + cid)
    poly = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    poly[:, 3] >>= 3                                        # Montgomery residues below both moduli
    short = poly[:100].copy()
    d_poly = torch.from_numpy(poly.view(np.int64)).cuda()
    d_short = torch.from_numpy(short.view(np.int64)).cuda()
    full = zk.CommitterKey(bases, cid, ctx).precompute()
    want = full.commit_batch([d_poly, d_short])
    windows = full.table_windows()
    full.close()
    if log_n <= 16:
        exp_xy, exp_inf = oracle_cpu.kzg_commit(cid, bases.cpu().numpy().view(np.uint64), poly)
        assert not want[0].infinity and np.array_equal(want[0].xy(), exp_xy)
    parts, dev = [], []
    for g in range(G):
        ckw = zk.CommitterKey(bases, cid, ctx).precompute(rows=(g, G))
        assert ckw.table_rows() == (g, G, (windows - g + G - 1) // G)
        parts.append(ckw.commit_batch_partial([d_poly, d_short]))
        pw = ckw.winsums_dev_words()
        assert pw == 2 * ckw.winsums_geometry()[2] * (32 if cid == 0 else 24)
        buf = torch.zeros((2, pw), dtype=torch.int64, device="cuda")
        ckw.commit_begin([d_poly])
        ckw.commit_begin([d_short])
        ckw.round_end_winsums_dev(buf, 2)
        dev.append(buf)
        if g == G - 1:
            got_dev = ckw.sum_winsums_dev(torch.stack(dev).reshape(G, 2 * pw).contiguous(), G, 2)
        ckw.close()
    assert zk.sum_partials_batch(np.stack(parts), cid) == want
    assert got_dev == want
