"""The NTT plans that no natural size below 2^28 reaches, run through the ctx option "ntt_passes" and compared whole with the C++
restatement (oracle/ark_cpu.cpp).  The pass count is a pure function of the size (one pass to 2^9, two to 2^18, three to 2^27, four
from 2^28), so without the option the four-pass chain of ntt.hip / ntt_pass.cuh -- the third non-final pass with its log_m / log_mprev
chain, the `s2` argument and the two-digit swap `rho_rev` of ntt_pass_final, the four-pass twiddle tables -- runs first at 8 GiB per
vector, and the radix-3 / radix-4 pass objects never run inside a multi-pass plan (ntt_pass_mid<F, 3> and <F, 4>, the partial last
window dit_window<F, 4, 1, 2, 3> in a non-final pass, idle lanes next to an inter-pass table: logc < 9 - S).  Every comparison is exact
equality of whole vectors; every transform's pass count is read back from the profile counter "ntt_passes", so a hook that did nothing
would fail here."""
import contextlib

import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib
import large_ref as lr

pytestmark = pytest.mark.gpu

KINDS = ("fft", "ifft", "coset_fft", "coset_ifft")

# passes -> log_n -> the radix exponents of the balanced rule (base = log_n // k, the first log_n % k passes get one more)
SHAPES = {
    2: {6: (3, 3), 7: (4, 3), 8: (4, 4), 9: (5, 4)},
    3: {9: (3, 3, 3), 10: (4, 3, 3), 11: (4, 4, 3), 12: (4, 4, 4), 13: (5, 4, 4)},
    4: {12: (3, 3, 3, 3), 13: (4, 3, 3, 3), 14: (4, 4, 3, 3), 15: (4, 4, 4, 3), 16: (4, 4, 4, 4), 20: (5, 5, 5, 5)},
}
BLS_CASES = [(0, k, log_n) for k, rows in SHAPES.items() for log_n in rows]
BN_CASES = [(1, 2, 7), (1, 3, 10), (1, 4, 12), (1, 4, 13), (1, 4, 14), (1, 4, 16)]


def balanced(log_n, k):
    return tuple(log_n // k + (1 if i < log_n % k else 0) for i in range(k))


def natural_passes(log_n):
    return 1 if log_n <= 9 else (log_n + 8) // 9


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def passes_run(ctx):
    return ctx.profile_get("ntt_passes")[1]


@contextlib.contextmanager
def forced(ctx, k):
    """Profiling on (the counter), "ntt_passes" = k; both back to their defaults afterwards, whatever happens."""
    ctx.profile(True)
    try:
        ctx.set_option("ntt_passes", k)
        yield
    finally:
        ctx.set_option("ntt_passes", 0)
        ctx.profile(False)


def counted(ctx, want, fn, *args):
    """fn(*args), which must launch exactly `want` passes"""
    before = passes_run(ctx)
    out = fn(*args)
    assert passes_run(ctx) - before == want, (passes_run(ctx) - before, want)
    return out


def test_the_table_is_the_balanced_rule():
    for k, rows in SHAPES.items():
        for log_n, radices in rows.items():
            assert balanced(log_n, k) == radices and sum(radices) == log_n and all(3 <= s <= 9 for s in radices)
    # every radix pair (first, second) and (second, third) that differs, and every radix 3, 4, 5 as a `quarter` first pass
    assert {rows[0] for k in SHAPES for rows in SHAPES[k].values()} == {3, 4, 5}
    assert SHAPES[4][14][1] != SHAPES[4][14][2]


@pytest.mark.parametrize("cid,k,log_n", BLS_CASES + BN_CASES)
def test_forced_shapes_against_the_oracle(cid, k, log_n, ctx, oracle_cpu):
    """All four kinds on n full-range elements, coset_fft on n/4 coefficients (the `quarter` first pass, here with radix 3, 4 and 5) and
    on n/4 + 1 (shortcut off), ifft on n - 1 (zero-extended); each transform launches exactly k passes.  2^14 under four passes is
    (4, 4, 3, 3): the second and third radix differ, which the swap of rho's two digits must get right."""
    n = 1 << log_n
    assert balanced(log_n, k) == SHAPES[k][log_n]
    x = lr.full_range(cid, n, 0x5A00 + 256 * cid + 32 * k + log_n)
    d = dev(x)
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    with forced(ctx, k):
        for kind, ln in [(kd, n) for kd in range(4)] + [(2, n // 4), (2, n // 4 + 1), (1, n - 1)]:
            got = host(counted(ctx, k, getattr(dom, KINDS[kind]), d[:ln]))
            assert np.array_equal(got, oracle_cpu.ntt(cid, kind, log_n, x[:ln])), (KINDS[kind], ln)


@pytest.mark.parametrize("cid,log_n", [(0, 12), (0, 16), (1, 12), (1, 16)])
def test_extreme_inputs_under_four_passes(cid, log_n, ctx, oracle_cpu):
    """Inputs in [r - 2^64, r) and all r - 1 through (3, 3, 3, 3) and (4, 4, 4, 4): the lazily reduced butterflies at their largest
    operands in every pass of the four, all four kinds."""
    n = 1 << log_n
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    with forced(ctx, 4):
        for name, x in (("near_r", lr.near_r(cid, n, 0x5A80 + log_n)), ("r-1", lr.r_minus_one(cid, n))):
            d = dev(x)
            for kind in range(4):
                got = host(counted(ctx, 4, getattr(dom, KINDS[kind]), d))
                assert np.array_equal(got, oracle_cpu.ntt(cid, kind, log_n, x)), (name, KINDS[kind])


@pytest.mark.parametrize("cid", [0, 1])
def test_batch_under_four_passes(cid, ctx, oracle_cpu):
    """One batch call of five polynomials with input lengths 0, 1, n/4, n/4 + 1 and n at 2^13, (4, 3, 3, 3): four launches for the five,
    each output equal to the single transform and to the oracle."""
    log_n = 13
    n = 1 << log_n
    x = lr.full_range(cid, n, 0x5AB0 + cid)
    d = dev(x)
    lens = (0, 1, n // 4, n // 4 + 1, n)
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    with forced(ctx, 4):
        for kind in (0, 2):
            outs = counted(ctx, 4, dom.batch, kind, [d[:ln] for ln in lens])
            assert len(outs) == len(lens)
            for ln, out in zip(lens, outs):
                single = host(counted(ctx, 4, getattr(dom, KINDS[kind]), d[:ln]))
                assert np.array_equal(host(out), single), (KINDS[kind], ln)
                assert np.array_equal(single, oracle_cpu.ntt(cid, kind, log_n, x[:ln])), (KINDS[kind], ln)


@pytest.mark.parametrize("cid", [0, 1])
def test_the_option_does_not_leak(cid, ctx, oracle_cpu):
    """One domain object at 2^12, prepared under the natural plan (two passes): natural, four passes, three, natural, four.  A plan
    built under one setting never serves another, the option takes effect at the next transform, and 0 restores the natural plan."""
    log_n = 12
    n = 1 << log_n
    x = lr.full_range(cid, n, 0x5AC0 + cid)
    d = dev(x)
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    assert _lib.lib().zk_ntt_prepare(ctx.handle, cid, log_n) == _lib.ZK_OK
    assert natural_passes(log_n) == 2
    with forced(ctx, 0):
        for kind in (0, 3):
            want = oracle_cpu.ntt(cid, kind, log_n, x)
            for k, ran in ((0, 2), (4, 4), (3, 3), (0, 2), (4, 4)):
                ctx.set_option("ntt_passes", k)
                assert ctx.get_option("ntt_passes") == k
                got = host(counted(ctx, ran, getattr(dom, KINDS[kind]), d))
                assert np.array_equal(got, want), (KINDS[kind], k)


@pytest.mark.parametrize("cid", [0, 1])
def test_refusals(cid, ctx, oracle_cpu):
    """A forced split with a radix outside [3, 9] -- four passes at 2^11 (3, 3, 3, 2), one at 2^10 (10), two at 2^19 (10, 9) -- is refused
    with the code the dispatch returns for such a radix, before anything is launched: the counter stands, the output buffer is
    unchanged, and the next natural transform on the ctx is correct.  Below 2^3 there are no passes and the option is ignored."""
    import torch
    for k, log_n in ((4, 11), (1, 10), (2, 19)):
        n = 1 << log_n
        x = lr.full_range(cid, n, 0x5AD0 + 32 * cid + log_n)
        d = dev(x)
        dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
        out = torch.full((n, 4), 0x5EED, dtype=torch.int64, device="cuda")
        with forced(ctx, k):
            before = passes_run(ctx)
            for kind in range(4):
                with pytest.raises(_lib.ZkError) as err:
                    dom._run(kind, d, out=out)
                assert err.value.code == _lib.ZK_ERR_UNSUPPORTED, (k, log_n, KINDS[kind])
            assert _lib.lib().zk_ntt_prepare(ctx.handle, cid, log_n) == _lib.ZK_ERR_UNSUPPORTED
            with pytest.raises(_lib.ZkError) as err:
                dom.batch(2, [d[: n // 4], d], outs=[out, torch.empty_like(out)])
            assert err.value.code == _lib.ZK_ERR_UNSUPPORTED
            torch.cuda.synchronize()
            assert passes_run(ctx) == before
            assert bool((out == 0x5EED).all()), (k, log_n)
            ctx.set_option("ntt_passes", 0)
            got = host(counted(ctx, natural_passes(log_n), dom.coset_fft, d))
            assert np.array_equal(got, oracle_cpu.ntt(cid, 2, log_n, x)), (k, log_n)
    with forced(ctx, 4):
        for log_n in (0, 1, 2):
            n = 1 << log_n
            x = lr.full_range(cid, n, 0x5AF0 + cid)
            dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
            for kind in range(4):
                for ln in (n, n - 1):
                    got = host(counted(ctx, 0, getattr(dom, KINDS[kind]), dev(x)[:ln]))
                    assert np.array_equal(got, oracle_cpu.ntt(cid, kind, log_n, x[:ln])), (log_n, KINDS[kind], ln)


def test_prover_end_to_end_under_two_passes(ctx, oracle_cpu):
    """The BLS12-381 2^7 case of test_proof_bytes_equal_the_cpu_restatement with every transform of the prover split in two: its
    domains are 2^7 and 2^9, (4, 3) and (5, 4).  Still the CPU restatement's proof bytes; and the prover's transforms ran two passes
    each: twice the launches of the same proof under the natural plan, where both domains take one."""
    from tests.test_prover_gpu import assert_proof_bytes_equal_the_cpu_restatement, run_case
    with forced(ctx, 0):
        before = passes_run(ctx)
        run_case(0, 7, ctx, oracle_cpu)
        natural = passes_run(ctx) - before
    assert natural > 0
    with forced(ctx, 2):
        before = passes_run(ctx)
        assert_proof_bytes_equal_the_cpu_restatement(0, 7, ctx, oracle_cpu)
        assert passes_run(ctx) - before == 2 * natural
