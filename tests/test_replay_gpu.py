"""The verifier's stage 2 on the device (csrc/replay.hip, zk_proof_replay_batch_dev, verifier.replay_batch_dev) against the host replay
(csrc/wire.hip zk_proof_replay_batch), which tests/test_verifier_host.py pins to the oracle: challenges, evaluations, point encodings
and statuses bit for bit -- on the valid proof, in every phase of the sponge's byte cursor, on malformed bytes, on offsets that lie --
and the batch verifier end to end by both routes.  The proofs are test_verifier_host's `Case`: one valid 32-row proof per curve."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ark_plonk_amd as zk  # noqa: E402
from ark_plonk_amd import _lib, verifier  # noqa: E402
from ark_plonk_amd.curves import fr_from_mont, fr_to_mont  # noqa: E402
from oracle import bigint_oracle as bo  # noqa: E402
from oracle import wire_oracle as wo  # noqa: E402
from tests.test_verifier_host import CH_NAMES, Case, drop_label, layout  # noqa: E402

pytestmark = pytest.mark.gpu
NCH, NEV = verifier.N_CHALLENGES, verifier.N_EVALS


@pytest.fixture(scope="module")
def cases():
    return {cid: Case(cid) for cid in (0, 1)}


# ------------------------------------------------------------------------------------------------------------------ both routes, raw
def flatten(cid, pis):
    """[[(position, integer value)] in the order GIVEN] -> (offsets, positions, Montgomery values): nothing is sorted or dropped here"""
    off = np.zeros(len(pis) + 1, dtype=np.uint64)
    pos, vals = [], []
    for j, pi in enumerate(pis):
        for p, v in pi:
            pos.append(p)
            vals.append(v)
        off[j + 1] = len(pos)
    p = np.array(pos if pos else [0], dtype=np.uint64)
    v = fr_to_mont(cid, vals) if vals else np.zeros((1, 4), dtype=np.uint64)
    return off, p, np.ascontiguousarray(v, dtype=np.uint64), len(pos)


def host_replay(case, datas, pis):
    """zk_proof_replay_batch through ctypes: (challenges, evaluations, points, status)"""
    B = len(datas)
    g = wo.fq_flag_bytes(case.cv)
    off, pos, vals, _ = flatten(case.cid, pis)
    bufs = (ctypes.c_char_p * B)(*datas)
    lens = (ctypes.c_size_t * B)(*[len(d) for d in datas])
    ch, ev = np.zeros((B, NCH, 4), np.uint64), np.zeros((B, NEV, 4), np.uint64)
    pts, st = np.zeros((B, 15, g), np.uint8), np.full(B, 0xff, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)          # noqa: E731
    rc = _lib.lib().zk_proof_replay_batch(case.seeded._h, case.cid, B, bufs, lens, p(off), p(pos), p(vals), p(ch), p(ev), p(pts), p(st))
    assert rc == _lib.ZK_OK
    return ch, ev, pts, st


def dev_replay(case, ctx, blob, poff, off, pos, vals, n_bytes=None, n_pi=None, with_points=True):
    """zk_proof_replay_batch_dev over the arrays as given -- offsets included, so they may lie"""
    import torch
    B = len(poff) - 1
    g = wo.fq_flag_bytes(case.cv)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype).copy()).cuda()   # noqa: E731
    d_blob = up(np.frombuffer(blob + b"\x00", dtype=np.uint8))           # never empty; the pad byte is outside proofs_bytes
    d_poff, d_off, d_pos, d_vals = up(np.asarray(poff, dtype=np.uint64)), up(off), up(pos), up(vals)
    ch = torch.full((B, NCH, 4), -1, dtype=torch.int64, device="cuda")
    ev = torch.full((B, NEV, 4), -1, dtype=torch.int64, device="cuda")
    pts = torch.full((B, 15, g), 0xEE, dtype=torch.uint8, device="cuda")
    st = torch.full((B,), 0xff, dtype=torch.uint8, device="cuda")
    ctx.use_torch_stream()
    rc = _lib.lib().zk_proof_replay_batch_dev(ctx.handle, case.seeded._h, case.cid, B, d_blob.data_ptr(), len(blob) if n_bytes is None else n_bytes,
                                              d_poff.data_ptr(), d_off.data_ptr(), d_pos.data_ptr(), d_vals.data_ptr(),
                                              int(off[-1]) if n_pi is None else n_pi, ch.data_ptr(), ev.data_ptr(),
                                              pts.data_ptr() if with_points else None, st.data_ptr())
    assert rc == _lib.ZK_OK
    torch.cuda.synchronize()
    return ch.cpu().numpy().view(np.uint64), ev.cpu().numpy().view(np.uint64), pts.cpu().numpy(), st.cpu().numpy()


def dev_of(case, ctx, datas, pis, **kw):
    off, pos, vals, _ = flatten(case.cid, pis)
    poff = np.zeros(len(datas) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in datas], out=poff[1:])
    return dev_replay(case, ctx, b"".join(datas), poff, off, pos, vals, **kw)


def assert_same(got, want, what=""):
    for name, g, w in zip(("challenges", "evaluations", "points", "status"), got, want):
        bad = [j for j in range(len(w)) if not np.array_equal(g[j], w[j])]
        assert not bad, (what, name, bad[:8])


def assert_rejected_rows(ch, ev, pts, st):
    """what a rejected proof leaves: zero rows, fifteen infinity encodings"""
    for j in np.nonzero(st)[0]:
        assert not ch[j].any() and not ev[j].any() and not pts[j, :, :-1].any() and (pts[j, :, -1] == 0x40).all(), j


# ------------------------------------------------------------------------------------------------------------------ 1 parity
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("n_pi", [0, 1, 3])
def test_device_replay_equals_the_host_replay(cases, cid, n_pi, ctx):
    import torch
    case = cases[cid]
    n = 32
    pub = dict(list(zip((0, 7, n - 1), bo.seeded_scalars(case.cv, 0x77 + n_pi, 3)))[:n_pi])
    for p in (pub, case.pub):
        pi = sorted(p.items())
        want = host_replay(case, [case.data], [pi])
        got = dev_of(case, ctx, [case.data], [pi])
        assert want[3].tolist() == [verifier.PROOF_OK]
        assert_same(got, want)
        _, ch = case.oracle_replay(case.data, p)
        assert fr_from_mont(cid, got[0][0]) == [ch[k] for k in CH_NAMES]
        # a second call gives the same rows: the seeded handle is not consumed
        assert_same(dev_of(case, ctx, [case.data], [pi]), want, "second call")
    assert all(ch[k] == case.prover_ch[k] for k in CH_NAMES)                 # the proof's own public inputs: what its prover drew
    # the Python entry point: device tensors, the same content; without the points the other three do not change
    pi_m = {i: fr_to_mont(cid, [v])[0] for i, v in case.pub.items()}
    t = verifier.replay_batch_dev(case.seeded, [case.data, case.data[:-1]], [pi_m, pi_m], cid, ctx)
    torch.cuda.synchronize()
    assert all(x.is_cuda for x in t)
    want2 = host_replay(case, [case.data, case.data[:-1]], [sorted(case.pub.items())] * 2)
    assert_same((t[0].cpu().numpy().view(np.uint64), t[1].cpu().numpy().view(np.uint64), t[2].cpu().numpy(), t[3].cpu().numpy()), want2)
    got = dev_of(case, ctx, [case.data], [sorted(case.pub.items())], with_points=False)
    assert_same(got[:2], want[:2])
    assert (got[2] == 0xEE).all() and got[3].tolist() == [0]


# ------------------------------------------------------------------------------------------------------------------ 2 phases
def with_extra_custom(cv, data, label, value):
    """the proof with one more custom evaluation (label, value) at the end, the count fixed up"""
    _, f, _, cnt = layout(cv)
    k = int.from_bytes(data[cnt:cnt + 8], "little")
    return data[:cnt] + (k + 1).to_bytes(8, "little") + data[cnt + 8:] + len(label).to_bytes(8, "little") + label + value.to_bytes(f, "little")


@pytest.mark.parametrize("cid", [0, 1])
def test_every_phase_of_the_sponge(cases, cid, ctx):
    """The rate is 166 bytes.  k = 0 .. 82 non-zero public inputs make messages of 8 + 40 k bytes -- gcd(40, 166) = 2: 83 distinct
    cursor phases, one of them a message that ends exactly on the rate boundary -- and an extra custom evaluation whose label has
    0 .. 167 bytes reaches the other parity and, from 166, spans a permutation inside one label.  One call: the lanes of a wave are
    out of phase with each other."""
    case = cases[cid]
    vals = bo.seeded_scalars(case.cv, 0x9a5e, 83)
    assert all(vals)
    datas, pis = [], []
    for k in range(83):
        datas.append(case.data)
        pis.append([(i, vals[i]) for i in range(k)])
    assert len({(8 + 40 * k) % 166 for k in range(83)}) == 83
    v = bo.seeded_scalars(case.cv, 0x1abe1, 1)[0]
    for ll in range(168):
        datas.append(with_extra_custom(case.cv, case.data, bytes((97 + i % 26) for i in range(ll)), v))
        pis.append(sorted(case.pub.items()))
    want = host_replay(case, datas, pis)
    assert not want[3].any()
    assert len({want[0][j].tobytes() for j in range(83)}) == 83 and len({want[0][83 + j].tobytes() for j in range(168)}) == 168
    assert_same(dev_of(case, ctx, datas, pis), want)


# ------------------------------------------------------------------------------------------------------------------ 3 malformed
def malformed(case):
    """(name, bytes, public inputs, expected status)"""
    cv, d = case.cv, case.data
    g, f, ev0, cnt = layout(cv)
    k = int.from_bytes(d[cnt:cnt + 8], "little")
    pub = sorted(case.pub.items())
    V = verifier
    out = [("truncated", d[:-1], pub, V.PROOF_TRUNCATED),
           ("trailing", d + b"\x00", pub, V.PROOF_TRAILING),
           ("option", d[:14 * g] + b"\x01" + d[14 * g + 1:], pub, V.PROOF_BAD_OPTION),
           ("second option", d[:15 * g + 1] + b"\x01" + d[15 * g + 2:], pub, V.PROOF_BAD_OPTION),
           ("eval = r", d[:ev0 + 3 * f] + cv.r.to_bytes(f, "little") + d[ev0 + 4 * f:], pub, V.PROOF_FR_NOT_REDUCED),
           ("custom eval = r", d[:-f] + cv.r.to_bytes(f, "little"), pub, V.PROOF_FR_NOT_REDUCED),
           ("label removed", drop_label(cv, d, b"q_c_eval"), pub, V.PROOF_MISSING_LABEL),
           ("count inflated", d[:cnt] + (k + 1).to_bytes(8, "little") + d[cnt + 8:], pub, V.PROOF_BAD_COUNT),
           ("count 2^63", d[:cnt] + (1 << 63).to_bytes(8, "little") + d[cnt + 8:], pub, V.PROOF_BAD_COUNT),
           ("empty", b"", pub, V.PROOF_TRUNCATED),
           ("5 bytes", d[:5], pub, V.PROOF_TRUNCATED),
           ("cut inside the count", d[:cnt + 3], pub, V.PROOF_TRUNCATED),
           # a repeated label with two values: well-formed, the last one counts
           ("repeated label", with_extra_custom(cv, d, b"q_l_eval", 12345), pub, V.PROOF_OK)]
    enc = bytearray((5).to_bytes(g, "little"))
    enc[-1] |= 0x40
    for idx in (0, 5, 12):                                      # infinity with stray x bits: replayed in canonical form
        out.append((f"stray infinity {idx}", d[:idx * g] + bytes(enc) + d[(idx + 1) * g:], pub, V.PROOF_OK))
    out.append(("zero public input", d, sorted({**case.pub, 9: 0}.items()), V.PROOF_OK))
    out.append(("descending positions", d, [(5, 1), (3, 2)], V.PROOF_BAD_PUBLIC_INPUTS))
    return out


@pytest.mark.parametrize("cid", [0, 1])
def test_malformed_bytes_are_statuses(cases, cid, ctx):
    case = cases[cid]
    bad = malformed(case)
    good_pi = sorted(case.pub.items())
    good = host_replay(case, [case.data], [good_pi])
    assert good[3].tolist() == [0]
    for name, data, pi, status in bad:                          # B = 1: each alone
        want = host_replay(case, [data], [pi])
        assert want[3].tolist() == [status], name
        got = dev_of(case, ctx, [data], [pi])
        assert_same(got, want, name)
        assert_rejected_rows(*got)
    rep = host_replay(case, [bad[12][1]], [bad[12][2]])          # the repeated label changed the row and the challenges behind it
    assert not np.array_equal(rep[1], good[1]) and not np.array_equal(rep[0][0, 12:], good[0][0, 12:])
    for B in (63, 64, 65, 130):                                  # interleaved with valid proofs: every third slot (65: the last lane too)
        datas, pis = [case.data] * B, [good_pi] * B
        slots = list(range(1, B, 3))
        assert len(slots) >= len(bad) and (B < 65 or 64 in slots)
        for k, j in enumerate(slots):
            _, datas[j], pis[j], _ = bad[k % len(bad)]
        want = host_replay(case, datas, pis)
        got = dev_of(case, ctx, datas, pis)
        assert_same(got, want, B)
        assert_rejected_rows(*got)
        assert [int(s) for s in got[3][slots]] == [bad[k % len(bad)][3] for k in range(len(slots))]
        for j in set(range(B)) - set(slots):                     # the valid neighbours are undisturbed
            assert got[3][j] == 0 and np.array_equal(got[0][j], good[0][0]) and np.array_equal(got[1][j], good[1][0]), (B, j)


# ------------------------------------------------------------------------------------------------------------------ 4 offsets
@pytest.mark.parametrize("cid", [0, 1])
def test_offsets_are_data(cases, cid, ctx):
    """The offsets live on the device, so the kernel vets them: a range that descends or leaves its buffer is that proof's status,
    the call returns ZK_OK and the neighbours get what their own bytes deserve."""
    case = cases[cid]
    d, pi = case.data, sorted(case.pub.items())
    n, B = len(d), 6
    blob = d * B
    off, pos, vals, m = flatten(cid, [pi] * B)
    assert m == B * len(pi) and m > 0
    good = host_replay(case, [d], [pi])

    flat = [pv for _ in range(B) for pv in pi]                 # (position, value) behind every index of the flattened arrays
    T, P = verifier.PROOF_TRUNCATED, verifier.PROOF_BAD_PUBLIC_INPUTS

    def check(poff, n_bytes, pioff, n_pi, lying):
        """lying: {proof: status} of the ranges that lie; every other proof must get the host's replay of what its ranges name"""
        got = dev_replay(case, ctx, blob, poff, pioff, pos, vals, n_bytes=n_bytes, n_pi=n_pi)
        assert_rejected_rows(*got)
        for j in range(B):
            p0, p1, o0, o1 = int(poff[j]), int(poff[j + 1]), int(pioff[j]), int(pioff[j + 1])
            if p1 < p0 or p1 > n_bytes:
                assert lying[j] == T == got[3][j], j
                continue
            pi_ok = o0 <= o1 <= n_pi
            w = host_replay(case, [blob[p0:p1]], [flat[o0:o1] if pi_ok else []])
            if w[3][0] == 0 and not pi_ok:
                assert lying[j] == P == got[3][j], j
            else:
                assert j not in lying or not pi_ok, j
                assert all(np.array_equal(g[j], x[0]) for g, x in zip(got, w)), j
        return got[3].tolist()

    straight = np.arange(B + 1, dtype=np.uint64) * np.uint64(n)
    assert check(straight, B * n, off, m, {}) == [0] * B
    # a proof range that descends: proof 1 is [n, n - 7); proof 2 then starts 7 bytes early: whatever those bytes deserve
    poff = straight.copy()
    poff[2] = n - 7
    st = check(poff, B * n, off, m, {1: T})
    assert st[0] == 0 and st[2] != 0 and st[3:] == [0, 0, 0]
    # a range that ends past proofs_bytes: by the last offset, and by a smaller proofs_bytes than the offsets claim
    poff = straight.copy()
    poff[B] += np.uint64(9)
    assert check(poff, B * n, off, m, {B - 1: T}) == [0] * (B - 1) + [T]
    assert check(straight, B * n - 1, off, m, {B - 1: T}) == [0] * (B - 1) + [T]
    assert check(straight, 3 * n + 5, off, m, {3: T, 4: T, 5: T}) == [0, 0, 0, T, T, T]
    poff = straight.copy()
    poff[3] = np.uint64((1 << 64) - 8)                           # near 2^64: no sum with it may wrap into the buffer
    assert check(poff, B * n, off, m, {2: T, 3: T}) == [0, 0, T, T, 0, 0]
    # a public-input range past n_pi_total, and one that descends
    pioff = off.copy()
    pioff[B] += np.uint64(1)
    assert check(straight, B * n, pioff, m, {B - 1: P}) == [0] * (B - 1) + [P]
    assert check(straight, B * n, off, m - 1, {B - 1: P}) == [0] * (B - 1) + [P]
    pioff = off.copy()
    pioff[2] = 0                                                 # proof 1's range descends; proof 2 gets [0, off[3]): positions that repeat
    st = check(straight, B * n, pioff, m, {1: P})
    assert st == [0, P, P, 0, 0, 0]
    # a malformed proof keeps the status of its bytes whatever its public-input range says
    poff, pioff = straight.copy(), off.copy()
    poff[B] -= np.uint64(1)
    pioff[B] += np.uint64(1)
    assert check(poff, B * n, pioff, m, {}) == [0] * (B - 1) + [T]


# ------------------------------------------------------------------------------------------------------------------ 5 arguments
def test_argument_errors(cases, ctx):
    import torch
    L, bad = _lib.lib(), _lib.ZK_ERR_BAD_ARG
    case = cases[0]
    seeded, h = case.seeded._h, ctx.handle
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")           # inputs at 0 (all zero: every offset is 0), outputs apart
    p, q = buf.data_ptr(), buf.data_ptr() + 8192
    full = [h, seeded, 0, 1, p + 1024, 8, p, p + 256, p + 512, p + 768, 0, q, q + 4096, q + 8192, q + 16384]
    assert "zk_proof_replay_batch_dev" in _lib.SYMBOLS
    assert L.zk_proof_replay_batch_dev(None, seeded, 0, 0, *([None, 0] + [None] * 4 + [0] + [None] * 4)) == bad
    assert L.zk_proof_replay_batch_dev(h, None, 0, 0, *([None, 0] + [None] * 4 + [0] + [None] * 4)) == bad
    assert L.zk_proof_replay_batch_dev(h, seeded, 7, 0, *([None, 0] + [None] * 4 + [0] + [None] * 4)) == bad          # unknown curve
    assert L.zk_proof_replay_batch_dev(h, seeded, 0, 0, *([None, 0] + [None] * 4 + [0] + [None] * 4)) == _lib.ZK_OK   # an empty batch
    for k in (4, 6, 7, 11, 12, 14):                              # proofs, proof offsets, pi offsets, challenges, evaluations, status
        args = list(full)
        args[k] = None
        assert L.zk_proof_replay_batch_dev(*args) == bad, k
    for k in (8, 9):                                             # positions / values: needed only when there are public inputs
        args = list(full)
        args[k] = None
        args[10] = 1
        assert L.zk_proof_replay_batch_dev(*args) == bad, k
    args = list(full)
    args[3] = 1 << 31
    assert L.zk_proof_replay_batch_dev(*args) == _lib.ZK_ERR_UNSUPPORTED
    # one proof of 8 zero bytes: a status, and the points may be left out
    args = list(full)
    buf[1] = 8
    args[13] = None
    assert L.zk_proof_replay_batch_dev(*args) == _lib.ZK_OK
    torch.cuda.synchronize()
    assert int(buf[(8192 + 16384) // 8]) & 0xff == verifier.PROOF_TRUNCATED
    with pytest.raises(ValueError):
        zk.BatchVerifier({}, 32, case.seeded, np.zeros(4, np.uint64), np.zeros(4, np.uint64), 0, ctx, replay="gpu")


# ------------------------------------------------------------------------------------------------------------------ 6 end to end
def test_batch_verifier_by_both_routes(ctx, oracle_cpu):
    """B = 65 with one evaluation tampered, one proof truncated and one point off the curve: the device replay and the host replay
    under the same weights give equal statuses, equal resident rows and equal (L, R); tau L == R on the range without the tampered
    proof; locate_invalid names the same proofs."""
    import torch
    from tests.test_verifier_gpu import eval_plus_one, off_curve, point_replaced, tamper_case, tau_relation, weights_for
    real = tamper_case(ctx, oracle_cpu)
    data, pub = real.proofs[0]
    B = 65
    datas = [data] * B
    datas[7] = eval_plus_one(real, data, 2)
    datas[40] = data[:-1]
    datas[64] = point_replaced(real, data, 5, off_curve(real))
    pis = [real.pi(pub)] * B
    ws = weights_for(B, 4242)
    m = lambda v: fr_to_mont(real.cid, [v])[0]                  # noqa: E731
    out = {}
    for route in ("host", "device"):
        bv = zk.BatchVerifier(real.vk, 1 << real.log_n, real.seeded(), m(real.ca), m(real.cd), real.cid, ctx, replay=route)
        try:
            assert bv.replay_on_device(B) == (route == "device")
            L, R, st = bv.fold(datas, pis, ws)
            torch.cuda.synchronize()
            rows = [t.cpu().numpy().copy() for t in bv.rows()]
            Lr, Rr = bv.fold_range(8, 40)
            assert tau_relation(real, Lr, Rr) and not Lr.infinity
            Lh, Rh = bv.fold_range(0, 8)
            assert not tau_relation(real, Lh, Rh)                # the tampered evaluation is in here
            found = bv.locate_invalid(datas, pis, lambda L, R: tau_relation(real, L, R), ws)
            out[route] = (L, R, st.tolist(), rows, (Lr, Rr), found)
        finally:
            bv.close()
    h, d = out["host"], out["device"]
    assert h[2] == d[2] and h[2][40] == verifier.PROOF_TRUNCATED and h[2][64] == verifier.VERIFY_BAD_POINT + verifier.G1_NOT_ON_CURVE
    assert sum(1 for s in h[2] if s) == 2
    assert all(np.array_equal(a, b) for a, b in zip(h[3], d[3]))
    assert h[0] == d[0] and h[1] == d[1] and h[4] == d[4]
    assert h[5] == d[5] == [7, 40, 64]
    auto = zk.BatchVerifier(real.vk, 1 << real.log_n, real.seeded(), m(real.ca), m(real.cd), real.cid, ctx)
    try:
        assert auto.replay == "auto" and not auto.replay_on_device(1)
        if verifier.REPLAY_ON_DEVICE_FROM is not None:
            assert auto.replay_on_device(verifier.REPLAY_ON_DEVICE_FROM) and not auto.replay_on_device(verifier.REPLAY_ON_DEVICE_FROM - 1)
    finally:
        auto.close()
