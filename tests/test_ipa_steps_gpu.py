"""The IPA opening's C ABI driven call by call (zk_ipa_round_dev / zk_ipa_fold_dev / zk_ipa_final_key_dev / zk_ipa_powers_dev,
ark_plonk_amd/csrc/ipa.hip) against the step oracle of tests/ipa_steps_ref.py, with challenges and vectors no transcript produces:
xi in {1, r - 1, 2, 2^-1}, challenges that send a folded key point to infinity or make the fold's last addition a doubling, the zero
vector, unit vectors, all-(r - 1) vectors, b the powers of {0, 1, r - 1, a root of unity}, h' at infinity, registered keys that hold
infinity, a first round over fewer points than the key has, and a window-sharded key.

Every comparison is exact: L and R after every round (affine integers or infinity), a[:m] and b[:m] after every fold, the final key
and c after the last.  The folded key is seen through the next round's L and R and through the final key; a is dense and random
wherever a case is about the key, so that every key point carries weight.  Keys are known-logarithm keys k_i G."""
import numpy as np
import pytest

import ipa_oracle as io
import ipa_steps_ref as sr
from oracle import bigint_oracle as bo
from test_ipa_gpu import points_of, rand_logs

pytestmark = pytest.mark.gpu
CURVES = {0: bo.BLS12_381, 1: bo.BN254}


class Driver:
    """Owns the buffers of one opening: a registered known-logarithm key, a and b as Montgomery limbs on the device, the workspace
    and h'.  hp: a logarithm (h' = hp G; 0 is infinity, sent as (0, 1)) or the 2L words themselves."""

    def __init__(self, ctx, cid, key_logs, a, b, hp, precompute=False, rows=None, inf_flags=None):
        import torch
        import ark_plonk_amd as zk
        from ark_plonk_amd import _lib
        self.ctx, self.cid, self.cv = ctx, cid, CURVES[cid]
        self.zk, self.lib, self._lib = zk, _lib.lib(), _lib
        self.L = zk.get_curve(cid).fq_limbs
        self.d1 = len(key_logs)
        bases = points_of(ctx, cid, key_logs)
        flags = None
        if inf_flags is not None:
            flags = torch.from_numpy(np.asarray(inf_flags, dtype=np.uint8)).cuda()
        self.key = zk.CommitterKey(bases, cid, ctx, infinity=flags)
        if precompute or rows is not None:
            self.key.precompute(rows=rows)
        self.a = a if isinstance(a, torch.Tensor) else self.upload(a)
        self.b = b if isinstance(b, torch.Tensor) else self.upload(b)
        nbytes = self.lib.zk_ipa_workspace_bytes(cid, self.d1)
        assert nbytes > 0
        self.work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        if isinstance(hp, int):
            P = bo.ec_mul(self.cv, hp % self.cv.r, (self.cv.gx, self.cv.gy))
            hp = self.inf_words() if P is None else zk.curves.fq_to_mont(cid, [P[0], P[1]]).reshape(-1)
        self.hp = np.ascontiguousarray(hp, dtype=np.uint64)
        assert self.hp.shape == (2 * self.L,)

    def upload(self, ints):
        import torch
        return torch.from_numpy(self.zk.curves.fr_to_mont(self.cid, ints).view(np.int64)).cuda()

    def inf_words(self):
        """(0, 1) in Montgomery form: GroupAffine::zero()"""
        w = np.zeros(2 * self.L, dtype=np.uint64)
        w[self.L:] = self.zk.curves.fq_to_mont(self.cid, [1]).reshape(-1)
        return w

    def point(self, words, flag):
        if flag:
            assert np.array_equal(words, self.inf_words()), "infinity is written as (0, 1)"
            return None
        x, y = self.zk.curves.fq_from_mont(self.cid, words.reshape(2, self.L))
        return (x, y)

    def round_rc(self, first, m, flags=True):
        L = self.L
        out = np.full(4 * L, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        oinf = np.full(2, 7, dtype=np.uint8)
        self.ctx.use_torch_stream()
        rc = self.lib.zk_ipa_round_dev(self.ctx.handle, self.key._h, first, m, self.a.data_ptr(), self.b.data_ptr(), self.work.data_ptr(),
                                       self.hp.ctypes.data, out.ctypes.data, oinf.ctypes.data if flags else None)
        return rc, out, oinf

    def round(self, first, m):
        rc, out, oinf = self.round_rc(first, m)
        self._lib.check(rc, "zk_ipa_round_dev")
        assert set(oinf.tolist()) <= {0, 1}
        return self.point(out[:2 * self.L], oinf[0]), self.point(out[2 * self.L:], oinf[1])

    def round_words(self, first, m):
        """the round with out_lr_inf = NULL: the 2 x 2L words alone"""
        rc, out, oinf = self.round_rc(first, m, flags=False)
        self._lib.check(rc, "zk_ipa_round_dev")
        assert oinf.tolist() == [7, 7]
        return out[:2 * self.L], out[2 * self.L:]

    def fold_rc(self, first, m, xi):
        xm = xi if isinstance(xi, np.ndarray) else self.zk.curves.fr_to_mont(self.cid, [xi])
        self.ctx.use_torch_stream()
        return self.lib.zk_ipa_fold_dev(self.ctx.handle, self.key._h, first, m, xm.ctypes.data, self.a.data_ptr(), self.b.data_ptr(),
                                        self.work.data_ptr())

    def fold(self, first, m, xi):
        self._lib.check(self.fold_rc(first, m, xi), "zk_ipa_fold_dev")

    def vectors(self, n):
        """a[:n], b[:n] read back as canonical integers"""
        f = self.zk.curves.fr_from_mont
        return (f(self.cid, self.a[:n].cpu().numpy().view(np.uint64).reshape(n, 4)),
                f(self.cid, self.b[:n].cpu().numpy().view(np.uint64).reshape(n, 4)))

    def final_key_words(self, flag=True):
        fk = np.full(2 * self.L, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        finf = np.full(1, 7, dtype=np.uint8)
        self.ctx.use_torch_stream()
        self._lib.check(self.lib.zk_ipa_final_key_dev(self.ctx.handle, self.cid, self.work.data_ptr(), fk.ctypes.data,
                                                      finf.ctypes.data if flag else None), "zk_ipa_final_key_dev")
        return fk, int(finf[0])

    def final_key(self):
        fk, finf = self.final_key_words()
        assert finf in (0, 1)
        return self.point(fk, finf)

    def close(self):
        self.key.close()


def walk(drv, a, b, key_logs, hp_log, challenge, two_m=None, refuse_in=()):
    """A whole opening over the first two_m (default: all) points, call by call next to the step oracle.  challenge(j, m, key) gives
    round j's xi from the oracle's key before the fold.  In the rounds of refuse_in, xi = 0 and xi = r are sent first: ZK_ERR_BAD_ARG,
    and a, b -- and, by the comparisons that follow, the key -- are what they were.  Returns the per-round records (ipa_steps_ref)."""
    cv = drv.cv
    r = cv.r
    st = sr.Steps(io.KnownLog(cv))
    KL = st.g
    two_m = two_m or len(key_logs)
    a, b, key = list(a[:two_m]), list(b[:two_m]), list(key_logs[:two_m])
    recs = []
    first, j = 1, 0
    while len(a) > 1:
        m = len(a) // 2
        Le, Re = st.round_(a, b, key, hp_log)
        Lp, Rp = KL.point(Le), KL.point(Re)
        assert drv.round(first, m) == (Lp, Rp), ("round", j, m)
        xi = challenge(j, m, key)
        if j in refuse_in:
            r_words = drv.zk.curves.ints_to_limbs([r], 4)
            assert drv.fold_rc(first, m, 0) == drv._lib.ZK_ERR_BAD_ARG
            assert drv.fold_rc(first, m, r_words) == drv._lib.ZK_ERR_BAD_ARG
            assert drv.vectors(2 * m) == (a, b), ("a refused fold touched a or b", j)
            assert drv.round(first, m) == (Lp, Rp), ("round after a refused fold", j, m)
        drv.fold(first, m, xi)
        a, b, key = st.fold(a, b, key, xi)
        assert drv.vectors(m) == (a, b), ("fold", j, m, xi)
        recs.append((Lp, Rp, xi, a, b, key))
        first, j = 0, j + 1
    assert drv.final_key() == KL.point(key[0]), "final key"
    return recs


def seeded(cv, seed):
    """an endless supply of random non-zero challenges"""
    vals = [x or 1 for x in rand_logs(cv, 40, seed)]
    return lambda j, m, key: vals[j]


# ---- chosen challenges
def chosen(cv, kind, m, key, seed=0):
    """The challenge of one kind for the key (logarithms) about to be folded to m points.  The three targeted kinds name their lane:
    index 0, index 1 (0 when m = 1), and the last lane of the first workgroup of the key fold (127, or m - 1 below 128 points)."""
    r = cv.r
    last = min(m, 128) - 1
    one = min(1, m - 1)
    xi = {
        "random": lambda: rand_logs(cv, 1, 7000 + seed + m)[0],
        "one": lambda: 1,
        "minus_one": lambda: r - 1,
        "two": lambda: 2,
        "half": lambda: pow(2, -1, r),
        "inf0": lambda: sr.xi_to_infinity(r, key[0], key[m]),
        "dbl1": lambda: sr.xi_to_doubling(r, key[one], key[one + m]),
        "inf_last": lambda: sr.xi_to_infinity(r, key[last], key[last + m]),
        "dbl_last": lambda: sr.xi_to_doubling(r, key[last], key[last + m]),
    }[kind]()
    assert 0 < xi < r, (kind, m)
    return xi


def claim_holds(cv, kind, m, key_before, key_after):
    """the targeted kinds do what they say in the oracle, on a lane whose two inputs are both finite"""
    last, one = min(m, 128) - 1, min(1, m - 1)
    i = {"inf0": 0, "dbl1": one, "inf_last": last, "dbl_last": last}.get(kind)
    if i is None:
        return True
    if key_before[i] == 0 or key_before[i + m] == 0:
        return False
    want = 0 if kind.startswith("inf") else 2 * key_before[i] % cv.r
    return key_after[i] == want


# Every schedule's rounds in order.  No single xi sends one lane to infinity AND makes its last addition a doubling (that needs
# 2 key_l[i] = 0), so "both at the last lane of a workgroup" is two challenges, "inf_last" and "dbl_last".  "inf0" stands in round 0 (the registered key, s->d_xy) and, as "inf0" or "inf_last", in a later
# round (the workspace key in place) with at least two rounds behind it; xi in {1, r - 1, 2^-1} stand in round 0 and in later rounds.
SCHEDULES_16 = [
    ["one", "minus_one", "half", "two"],
    ["minus_one", "half", "one", "random"],
    ["half", "two", "minus_one", "one"],
    ["inf0", "inf_last", "random", "dbl1"],
    ["dbl1", "inf0", "two", "dbl_last"],
    ["dbl_last", "dbl1", "inf_last", "half"],
    ["inf_last", "random", "dbl_last", "inf0"],
]
# d1 = 2048: m = 1024, 512, 256, 128 (the "last lane" is 127), 64, ..., 1
SCHEDULES_2048 = [
    ["inf0", "dbl_last", "inf_last", "dbl1", "one", "minus_one", "two", "half", "inf0", "random", "dbl1"],
    ["minus_one", "half", "one", "inf_last", "two", "inf0", "random", "dbl1", "dbl_last", "inf_last", "random"],
]


def chosen_walk(ctx, cid, d1, schedule, seed, pin_second_null=False):
    cv = CURVES[cid]
    r = cv.r
    logs = rand_logs(cv, d1 + 1, seed)
    logs, k_h = logs[:d1], logs[d1]
    if pin_second_null:
        # round 0's "inf0" also nulls index d1/4, the partner of index 0 in round 1: that lane then folds two null points whatever
        # the challenge, and the null point survives into round 2's key
        logs[d1 // 4] = logs[0] * logs[d1 // 4 + d1 // 2] % r * pow(logs[d1 // 2], -1, r) % r
    a = rand_logs(cv, d1, seed + 1)
    b = rand_logs(cv, d1, seed + 2)
    drv = Driver(ctx, cid, logs, a, b, k_h)
    seen = []

    def challenge(j, m, key):
        seen.append((schedule[j], m, list(key)))
        return chosen(cv, schedule[j], m, key, seed)

    recs = walk(drv, a, b, logs, k_h, challenge, refuse_in=(0, 1) if d1 == 16 else ())
    drv.close()
    assert len(recs) == len(schedule)
    for (kind, m, before), rec in zip(seen, recs):
        assert claim_holds(cv, kind, m, before, rec[5]), (kind, m)
    return seen, recs


@pytest.mark.parametrize("sched", range(len(SCHEDULES_16)))
@pytest.mark.parametrize("cid", [0, 1])
def test_chosen_challenges_one_workgroup(ctx, cid, sched):
    seen, recs = chosen_walk(ctx, cid, 16, SCHEDULES_16[sched], 100 * sched + cid)
    if sched == 3:                                           # a null point in the key of rounds 1, 2 and 3
        assert recs[0][5][0] == 0 and recs[1][5][3] == 0 and 0 in recs[1][5]


@pytest.mark.parametrize("sched", range(len(SCHEDULES_2048)))
@pytest.mark.parametrize("cid", [0, 1])
def test_chosen_challenges_across_workgroups(ctx, cid, sched):
    """d1 = 2048: round 0's scalar pass spans 4 workgroups of 256 lanes (4 partial sums added on the host), its key fold 8 of 128"""
    seen, recs = chosen_walk(ctx, cid, 2048, SCHEDULES_2048[sched], 5000 + 10 * sched + cid, pin_second_null=(sched == 0))
    if sched == 0:
        assert recs[0][5][0] == 0 and recs[0][5][512] == 0   # round 1 reads a key with two null points
        assert recs[1][5][0] == 0                            # ... folds them into one, which round 2 reads
        assert recs[2][5][127] == 0                          # ... and round 2's fold makes another at lane 127, in place
        assert recs[8][5][0] == 0 and len(recs[8][5]) == 4   # once more two rounds before the end
    kinds = {k for s in SCHEDULES_2048 + SCHEDULES_16 for k in s}
    assert kinds == {"random", "one", "minus_one", "two", "half", "inf0", "dbl1", "inf_last", "dbl_last"}


# ---- the final key at infinity
@pytest.mark.parametrize("cid", [0, 1])
def test_final_key_at_infinity(ctx, cid):
    cv = CURVES[cid]
    k0, k1, k_h = rand_logs(cv, 3, 60 + cid)
    a, b = rand_logs(cv, 2, 61 + cid), rand_logs(cv, 2, 62 + cid)
    drv = Driver(ctx, cid, [k0, k1], a, b, k_h)
    recs = walk(drv, a, b, [k0, k1], k_h, lambda j, m, key: sr.xi_to_infinity(cv.r, key[0], key[1]))
    assert recs[0][5] == [0]
    words, flag = drv.final_key_words()
    assert flag == 1 and np.array_equal(words, drv.inf_words())
    words, flag = drv.final_key_words(flag=False)
    assert flag == 7 and np.array_equal(words, drv.inf_words())
    drv.close()


# ---- degenerate vectors
def powers_dev(ctx, cid, z, n, guard=True):
    """zk_ipa_powers_dev into a buffer with one guard element behind the n-th: (return code, device tensor of n rows)"""
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib
    buf = torch.full((n + 1, 4), 0x5EED5EED5EED5EED, dtype=torch.int64, device="cuda")
    zm = z if isinstance(z, np.ndarray) else zk.curves.fr_to_mont(cid, [z])
    ctx.use_torch_stream()
    rc = _lib.lib().zk_ipa_powers_dev(ctx.handle, cid, zm.ctypes.data, n, buf.data_ptr())
    torch.cuda.synchronize()
    assert buf[n].tolist() == [0x5EED5EED5EED5EED] * 4, "the element behind the n-th was written"
    return rc, buf[:n]


def root_of_unity(cid, d1):
    w = bo.CURVES[cid].root_of_unity(d1.bit_length() - 1)
    r = CURVES[cid].r
    assert pow(w, d1, r) == 1 and (d1 == 1 or pow(w, d1 // 2, r) == r - 1)
    return w


DEGENERATE = ["a_zero", "a_e0", "a_elast", "all_minus_one", "b_pow_0", "b_pow_1", "b_pow_minus_one", "b_pow_root", "hp_zero_words", "hp_0_1",
              "no_flags"]


@pytest.mark.parametrize("case", DEGENERATE)
@pytest.mark.parametrize("d1", [16, 1024])
@pytest.mark.parametrize("cid", [0, 1])
def test_degenerate_vectors(ctx, cid, d1, case):
    import ark_plonk_amd as zk
    cv = CURVES[cid]
    r = cv.r
    st = sr.Steps(io.KnownLog(cv))
    logs = rand_logs(cv, d1 + 1, 300 + cid + d1)
    logs, k_h = logs[:d1], logs[d1]
    a = rand_logs(cv, d1, 301 + cid + d1)
    b = rand_logs(cv, d1, 302 + cid + d1)
    hp = k_h
    if case == "a_zero":
        a = [0] * d1
    elif case == "a_e0":
        a = [1] + [0] * (d1 - 1)
    elif case == "a_elast":
        a = [0] * (d1 - 1) + [1]
    elif case == "all_minus_one":
        a, b = [r - 1] * d1, [r - 1] * d1
    elif case.startswith("b_pow_"):
        z = {"0": 0, "1": 1, "minus_one": r - 1, "root": root_of_unity(cid, d1)}[case[6:]]
        b = st.powers(z, d1)
        rc, b_dev = powers_dev(ctx, cid, z, d1)
        assert rc == 0
        assert zk.curves.fr_from_mont(cid, b_dev.cpu().numpy().view(np.uint64)) == b, "zk_ipa_powers_dev"
    elif case == "no_flags":
        a = rand_logs(cv, d1 // 2, 303) + [0] * (d1 // 2)     # a_r = 0: L of round 0 is infinity
    drv = Driver(ctx, cid, logs, a, b_dev.contiguous() if case.startswith("b_pow_") else b, hp)
    if case == "hp_zero_words":
        drv.hp = np.zeros(2 * drv.L, dtype=np.uint64)
        hp = 0
    elif case == "hp_0_1":
        drv.hp = drv.inf_words()
        hp = 0
    if case == "no_flags":
        Lw, Rw = drv.round_words(1, d1 // 2)
        Le, Re = st.round_(a, b, logs, hp)
        assert Le == 0 and np.array_equal(Lw, drv.inf_words())
        assert drv.point(Rw, 0) == st.g.point(Re)
    recs = walk(drv, a, b, logs, hp, seeded(cv, 310 + cid + d1))
    drv.close()
    if case == "a_zero":
        assert all(rec[0] is None and rec[1] is None for rec in recs) and recs[-1][3] == [0]
    if case in ("hp_zero_words", "hp_0_1"):
        # the inner products carry no weight, and the key alone does not give these points to a walk with h'
        other = st.walk(a, b, logs, k_h, lambda j, *_: recs[j][2])
        assert [x[:2] for x in other] != [x[:2] for x in recs]


# ---- registered keys that hold infinity
def zero_sets(d1):
    m = d1 // 2
    return {"ends": [0, d1 - 1], "middle": [m - 1, m], "pair": [5, 5 + m], "all": [0, m - 1, m, d1 - 1, 5, 5 + m]}


def infinity_key_walk(ctx, cid, d1, zeros, precompute, flagged=()):
    cv = CURVES[cid]
    logs = rand_logs(cv, d1 + 1, 400 + cid + d1)
    logs, k_h = logs[:d1], logs[d1]
    for i in zeros:
        logs[i] = 0
    flags = None
    send = list(logs)
    if flagged:                                              # infinity by flag over the words of a finite point
        flags = np.zeros(d1, dtype=np.uint8)
        for i in flagged:
            assert logs[i] == 0
            flags[i] = 1
            send[i] = 12345 + i
    a = rand_logs(cv, d1, 401 + cid + d1)
    b = rand_logs(cv, d1, 402 + cid + d1)
    drv = Driver(ctx, cid, send, a, b, k_h, precompute=precompute, inf_flags=flags)
    recs = walk(drv, a, b, logs, k_h, seeded(cv, 403 + cid + d1))
    drv.close()
    return recs


@pytest.mark.parametrize("which", ["ends", "middle", "pair", "all"])
@pytest.mark.parametrize("cid", [0, 1])
def test_keys_holding_infinity_per_window_path(ctx, cid, which):
    d1 = 256
    zeros = zero_sets(d1)[which]
    recs = infinity_key_walk(ctx, cid, d1, zeros, precompute=False, flagged=zeros[:1] if which in ("ends", "all") else ())
    if which in ("pair", "all"):
        assert recs[0][5][5] == 0                            # both halves null: the folded key keeps a null point


@pytest.mark.parametrize("which", ["ends", "all"])
@pytest.mark.parametrize("cid", [0, 1])
def test_keys_holding_infinity_table_path(ctx, cid, which):
    """precompute() at d1 = 2^14: round 0's two MSMs are over 2^13 scalars each, the smallest count the window-table path takes
    (ZK_PRE_MIN_N, csrc/ctx.h, the bound of msm_plan.hip's geometry; test_precomputed_table_threshold_sizes runs the same count)"""
    d1 = 1 << 14
    recs = infinity_key_walk(ctx, cid, d1, zero_sets(d1)[which], precompute=True)
    assert len(recs) == 14


# ---- a first round over fewer points than the key holds
@pytest.mark.parametrize("two_m", [16, 2])
@pytest.mark.parametrize("cid", [0, 1])
def test_short_first_round(ctx, cid, two_m):
    cv = CURVES[cid]
    d1 = 64
    logs = rand_logs(cv, d1 + 1, 500 + cid)
    logs, k_h = logs[:d1], logs[d1]
    a = rand_logs(cv, two_m, 501 + cid)
    b = rand_logs(cv, two_m, 502 + cid)
    drv = Driver(ctx, cid, logs, a, b, k_h)
    recs = walk(drv, a, b, logs, k_h, seeded(cv, 503 + cid), two_m=two_m)
    drv.close()
    assert len(recs) == two_m.bit_length() - 1


@pytest.mark.parametrize("log_d1", [14, 15])
@pytest.mark.parametrize("cid", [0, 1])
def test_short_first_round_on_a_precomputed_key(ctx, cid, log_d1):
    """A first round over half the key, the key with its window table.  d1 = 2^14, 2m = 2^13: the two MSMs of 2^12 scalars are below
    ZK_PRE_MIN_N and take the per-window path over the registered points at offsets 0 and m.  d1 = 2^15, 2m = 2^14: 2^13 scalars,
    the window-table path at an SRS offset of m with a count below n."""
    cv = CURVES[cid]
    d1 = 1 << log_d1
    two_m = d1 // 2
    logs = rand_logs(cv, d1 + 1, 600 + cid + log_d1)
    logs, k_h = logs[:d1], logs[d1]
    a = rand_logs(cv, two_m, 601 + cid)
    b = rand_logs(cv, two_m, 602 + cid)
    drv = Driver(ctx, cid, logs, a, b, k_h, precompute=True)
    recs = walk(drv, a, b, logs, k_h, seeded(cv, 603 + cid), two_m=two_m)
    drv.close()
    assert len(recs) == log_d1 - 1


# ---- zk_ipa_powers_dev on its own
@pytest.mark.parametrize("cid", [0, 1])
def test_powers_on_its_own(ctx, cid):
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib
    cv = CURVES[cid]
    r = cv.r
    st = sr.Steps(io.KnownLog(cv))
    for z in (0, 1, 2, r - 1, rand_logs(cv, 1, 70 + cid)[0]):
        zm = zk.curves.fr_to_mont(cid, [z])
        assert _lib.lib().zk_ipa_powers_dev(ctx.handle, cid, zm.ctypes.data, 0, None) == 0
        for n in (1, 15, 16, 17, 4095, 4096, 4097):
            rc, out = powers_dev(ctx, cid, z, n)
            assert rc == 0
            assert zk.curves.fr_from_mont(cid, out.cpu().numpy().view(np.uint64)) == st.powers(z, n), (z, n)
    for bad in (r, (1 << 256) - 1):
        rc, out = powers_dev(ctx, cid, zk.curves.ints_to_limbs([bad], 4), 17)
        assert rc == _lib.ZK_ERR_BAD_ARG
        assert out.tolist() == [[0x5EED5EED5EED5EED] * 4] * 17, "a refused call wrote"


# ---- a window-sharded key
@pytest.mark.parametrize("cid", [0, 1])
def test_window_sharded_key_is_refused_and_still_answers_an_msm(ctx, cid):
    """2^14 points in G = 3 window shards, the smallest shape of test_window_shards_small_both_curves: the first round is
    ZK_ERR_UNSUPPORTED on every shard, the fold before nothing, and the handles' partial MSMs afterwards are what they were before
    and add up to the MSM over the whole key"""
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib
    cv = CURVES[cid]
    d1, G = 1 << 14, 3
    logs = rand_logs(cv, d1 + 1, 800 + cid)
    logs, k_h = logs[:d1], logs[d1]
    a = rand_logs(cv, d1, 801 + cid)
    b = rand_logs(cv, d1, 802 + cid)
    scal = torch.from_numpy(zk.curves.ints_to_limbs(a, 4).view(np.int64)).cuda()
    parts = []
    for g in range(G):
        drv = Driver(ctx, cid, logs, a, b, k_h, rows=(g, G))
        assert drv.key.table_rows()[:2] == (g, G)
        before = drv.key.msm_partial(scal)
        rc, out, oinf = drv.round_rc(1, d1 // 2)
        assert rc == _lib.ZK_ERR_UNSUPPORTED
        assert drv.vectors(d1) == (a, b)
        after = drv.key.msm_partial(scal)
        assert zk.sum_partials(before[None], cid) == zk.sum_partials(after[None], cid)      # Jacobian partials: compared as points
        parts.append(after)
        drv.close()
    total = zk.sum_partials(np.stack(parts), cid)
    want = io.KnownLog(cv).point(sum(x * y for x, y in zip(logs, a)) % cv.r)
    assert not total.infinity and tuple(zk.curves.fq_from_mont(cid, np.stack([total.x, total.y]))) == want
