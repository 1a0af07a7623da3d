"""GPU suite of circuit compilation: zk_perm_sigma_dev / zk_fr_gather_dev through the C ABI and `ark_plonk_amd.compile` end to end.
Every comparison is exact equality of limbs or of u32 positions.  The first two cases are expected outputs the reference itself
holds (plonk-core/src/permutation/mod.rs:970-1203, tests/golden/sigma_reference_cases.json)."""
import ctypes
import json
import os

import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib, permutation, prover, transcript
from ark_plonk_amd import compile as zc
from ark_plonk_amd.curves import fr_from_mont, fr_to_mont
from oracle import bigint_oracle as bo
from oracle import verifier_oracle as vo
from oracle import wire_oracle as wo
from tests import compile_ref as cr
from tests.conftest import TAU, srs_from_powers, tau_powers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "sigma_reference_cases.json")))["cases"]


def i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)).cuda()


def dev_fr(cid, ints):
    import torch
    return torch.from_numpy(fr_to_mont(cid, ints).view(np.int64)).cuda()


def run_sigma(ctx, cid, log_n, ins_var, ins_pos, num_vars, want_pos=True, want_evals=True, m=None):
    """raw call: (rc, positions as int64 numpy or None, [4 x (n, 4) uint64 numpy] or None)"""
    import torch
    n = 1 << log_n
    dv, dp = i32(ins_var), i32(ins_pos)
    pos = torch.empty(4 * n, dtype=torch.int32, device="cuda") if want_pos else None
    ev = [torch.empty((n, 4), dtype=torch.int64, device="cuda") for _ in range(4)] if want_evals else None
    ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ev]) if want_evals else None
    ctx.use_torch_stream()
    rc = _lib.lib().zk_perm_sigma_dev(ctx.handle, cid, log_n, dv.data_ptr() if dv.numel() else None, dp.data_ptr() if dp.numel() else None,
                                      len(ins_var) if m is None else m, num_vars, None if pos is None else pos.data_ptr(), ptrs)
    torch.cuda.synchronize()
    return (rc, None if pos is None else pos.cpu().numpy().view(np.uint32).astype(np.int64),
            None if ev is None else [t.cpu().numpy().view(np.uint64) for t in ev])


def omega_tables(oracle_cpu, cid, log_n):
    """[K_w * omega^i as Montgomery limbs, i < n] for w in 0..3, by doubling on the CPU restatement's vectorised Fr product"""
    cv = bo.CURVES[cid]
    n = 1 << log_n
    w = cv.root_of_unity(log_n)
    pw = np.empty((n, 4), dtype=np.uint64)
    pw[0] = fr_to_mont(cid, [1])[0]
    k = 1
    while k < n:
        step = fr_to_mont(cid, [pow(w, k, cv.r)])
        pw[k:2 * k] = oracle_cpu.fr_op(cid, "mul", pw[:k], np.broadcast_to(step, (k, 4)).copy())
        k *= 2
    return [pw if kk == 1 else oracle_cpu.fr_op(cid, "mul", pw, np.broadcast_to(fr_to_mont(cid, [kk]), (n, 4)).copy()) for kk in cr.K]


def expected_evals(tables, n, sigma):
    s = np.asarray(sigma, dtype=np.int64)
    flat = np.concatenate(tables, axis=0)               # row w * n + i = K_w omega^i: the position itself is the index
    return [flat[s[w * n:(w + 1) * n]] for w in range(4)]


def skewed_input(rng, n, num_vars=None, holes=True, m=None):
    """half of all positions on variable 0, many variables with exactly one position, the largest id used, holes in used rows"""
    m = (4 * n - (n // 4 if holes else 0)) if m is None else m
    num_vars = 4 * n if num_vars is None else num_vars
    var = rng.integers(1, num_vars, size=m)
    var[rng.random(m) < 0.5] = 0
    if m:
        var[m // 2] = num_vars - 1
    pos = rng.permutation(4 * n)[:m] if holes else np.arange(4 * n)[:m]
    return var, pos


# ---- 1. the reference's own expected outputs
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("k", [0, 1])
def test_reference_held_cases(cid, k, ctx):
    case = CASES[k]
    n = case["n"]
    ins_var, ins_pos = cr.canonical_insertions(n, *zip(*case["gates"]))
    rc, pos, ev = run_sigma(ctx, cid, 2, ins_var, ins_pos, case["num_vars"])
    assert rc == 0
    assert pos.tolist() == [p for wire in case["sigma_pos"] for p in wire]
    cv = bo.CURVES[cid]
    w = cv.root_of_unity(2)
    assert np.array_equal(zk.Radix2EvaluationDomain.new(n, cid).group_gen(), fr_to_mont(cid, [w])[0])
    for wire in range(4):
        want = fr_to_mont(cid, [cr.K[kk] * pow(w, e, cv.r) % cv.r for kk, e in case["sigma_enc"][wire]])
        assert np.array_equal(ev[wire], want), (case["source"], wire)


# ---- 2. against the restated definition, 2^3 .. 2^16
@pytest.mark.parametrize("cid", [0, 1])
def test_sigma_matches_the_definition_small_sizes(cid, ctx, oracle_cpu):
    rng = np.random.default_rng(100 + cid)
    for log_n in range(3, 17):
        n = 1 << log_n
        tables = omega_tables(oracle_cpu, cid, log_n)
        inputs = [skewed_input(rng, n) + (4 * n,)]
        # non-row order: Left(r), Right(r), Fourth(r), then Output(r - 1) (logic.rs:212-218); the last row's output is never inserted
        g = n - 2
        iv, ip = [], []
        ids = rng.integers(0, n, size=(g, 4))
        for r in range(g):
            iv += [ids[r, 0], ids[r, 1], ids[r, 3]]
            ip += [r, n + r, 3 * n + r]
            if r:
                iv.append(ids[r, 2])
                ip.append(2 * n + r - 1)
        inputs.append((np.array(iv), np.array(ip), n))
        inputs.append((np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 1))      # m = 0: the identity
        inputs.append((np.zeros(4 * n, dtype=np.int64), rng.permutation(4 * n), 1))        # one variable owns everything: no radix pass
        for var, pos, nv in inputs:
            rc, got, ev = run_sigma(ctx, cid, log_n, var, pos, nv)
            assert rc == 0, (log_n, rc)
            want = cr.sigma_numpy(n, var, pos)
            if log_n <= 8:
                assert want.tolist() == cr.sigma_dict(n, var, pos)
            assert np.array_equal(got, want), log_n
            for wire, (a, b) in enumerate(zip(ev, expected_evals(tables, n, want))):
                assert np.array_equal(a, b), (log_n, wire)


# ---- 3. large sizes, whole vectors, and the structure of the device output alone
@pytest.mark.parametrize("cid,log_n", [(0, 20), (0, 22), (1, 20)])
def test_sigma_large(cid, log_n, ctx, oracle_cpu):
    n = 1 << log_n
    rng = np.random.default_rng(7 * log_n + cid)
    var, pos = skewed_input(rng, n)
    rc, got, ev = run_sigma(ctx, cid, log_n, var, pos, 4 * n)
    assert rc == 0
    want = cr.sigma_numpy(n, var, pos)
    assert np.array_equal(got, want)
    tables = omega_tables(oracle_cpu, cid, log_n)
    for wire, (a, b) in enumerate(zip(ev, expected_evals(tables, n, want))):
        assert np.array_equal(a, b), wire
    # on the device output alone
    assert np.array_equal(np.sort(got), np.arange(4 * n))                                  # a bijection of [0, 4n)
    var_of = np.full(4 * n, -1, dtype=np.int64)
    var_of[pos] = var
    never = var_of < 0
    var_of[never] = -1 - np.nonzero(never)[0]                                              # a never-inserted cell is its own class
    assert np.array_equal(var_of[got], var_of)
    assert cr.cycle_count(got) == np.unique(var).shape[0] + int(never.sum())


def test_sigma_digit_count_scan_second_top_chunk(ctx):
    """m = 2^24 + 8192 insertions at n = 2^23: the digit counts of a radix pass, 256 per tile of 4096 keys, are 256 * 4098 > 1024^2
    values, so the scan's single top workgroup (csrc/dev_scan.cuh, 1024 sums a chunk) goes round its loop a second time -- the
    smallest such shape.  Three radix passes; positions only (nothing here depends on the field).  Variable v is inserted at calls v
    and v + m/2, at the positions pos[k] = (5k + 3) mod 2^25 (a bijection: no cell twice), so sigma swaps pos[v] and pos[v + m/2]
    and fixes every other cell; whole vectors are compared, the expected one built on the device."""
    import torch
    log_n, m = 23, (1 << 24) + 8192
    h, n_pos = m // 2, 4 << log_n
    k = torch.arange(m, dtype=torch.int64, device="cuda")
    pos = (5 * k + 3) % n_pos
    ins_var, ins_pos = (k % h).to(torch.int32), pos.to(torch.int32)
    got = torch.empty(n_pos, dtype=torch.int32, device="cuda")
    ctx.use_torch_stream()
    rc = _lib.lib().zk_perm_sigma_dev(ctx.handle, 0, log_n, ins_var.data_ptr(), ins_pos.data_ptr(), m, h, got.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    want = torch.arange(n_pos, dtype=torch.int64, device="cuda")
    want[pos[:h]] = pos[h:]
    want[pos[h:]] = pos[:h]
    assert torch.equal(got.to(torch.int64), want)


# ---- 4. bad input is a code, and the ctx works afterwards
@pytest.mark.parametrize("cid", [0, 1])
def test_bad_input_is_refused(cid, ctx):
    log_n, n = 6, 64
    rng = np.random.default_rng(3)
    var, pos = skewed_input(rng, n, holes=False)
    bad = []
    v, p = var.copy(), pos.copy()
    p[17] = p[200]
    bad.append((v, p, 4 * n, None))                                # a position inserted twice
    v, p = var.copy(), pos.copy()
    p[5] = 4 * n
    bad.append((v, p, 4 * n, None))                                # position = 4n
    v, p = var.copy(), pos.copy()
    v[9] = 4 * n
    bad.append((v, p, 4 * n, None))                                # variable = num_vars
    bad.append((np.zeros(4 * n + 1, dtype=np.int64), np.arange(4 * n + 1) % (4 * n), 1, 4 * n + 1))      # m = 4n + 1
    for v, p, nv, m in bad:
        rc, _, _ = run_sigma(ctx, cid, log_n, v, p, nv, m=m)
        assert rc == _lib.ZK_ERR_BAD_ARG
    import torch
    one = torch.zeros(8, dtype=torch.int32, device="cuda")
    rc = _lib.lib().zk_perm_sigma_dev(ctx.handle, cid, bo.CURVES[cid].two_adicity + 1, one.data_ptr(), one.data_ptr(), 1, 1, one.data_ptr(), None)
    assert rc == _lib.ZK_ERR_DOMAIN_TOO_LARGE
    rc, got, _ = run_sigma(ctx, cid, log_n, var, pos, 4 * n, want_evals=False)
    assert rc == 0 and np.array_equal(got, cr.sigma_numpy(n, var, pos))


# ---- 5. the gather
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("log_n", [10, 20])
def test_gather(cid, log_n, ctx):
    import torch
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    vals = rng.integers(0, 1 << 62, size=(n // 2 + 3, 4), dtype=np.uint64)
    idx = rng.integers(0, vals.shape[0], size=n)
    idx[0], idx[-1] = vals.shape[0] - 1, 0
    d_vals = torch.from_numpy(vals.view(np.int64)).cuda()
    out = zc.gather(d_vals, i32(idx), cid, ctx)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), vals[idx])
    idx[n // 3] = vals.shape[0]
    with pytest.raises(_lib.ZkError) as e:
        zc.gather(d_vals, i32(idx), cid, ctx)
    assert e.value.code == _lib.ZK_ERR_BAD_ARG


# ---- the circuit of 6 - 9: given by variables
def variable_circuit(cid, log_n, seed, device="cuda"):
    """Gates by variable ids: a, b, d of an arithmetic gate are earlier outputs or variable 0, c a fresh variable set to
    q_m ab + q_l a + q_r b + q_4 d + q_c (+ the public input of the row); one third of the rows look a row of the table up (fresh
    variables holding that row); the table has n / 4 rows; public inputs on rows 1 and 3.  Returns (description, values as integers,
    public inputs as integers, the id of one arithmetic output)."""
    cv = bo.CURVES[cid]
    p, n = cv.r, 1 << log_n
    g = n - 3
    rng = np.random.default_rng(seed)
    rnd = lambda k, s: bo.seeded_scalars(cv, seed * 1000 + s, k)  # noqa: E731
    rows = max(n // 4, 2)
    tcols = [rnd(rows, 10 + k) for k in range(4)]
    qs = {name: rnd(g, 20 + k) for k, name in enumerate(("q_m", "q_l", "q_r", "q_4", "q_c"))}
    fresh = rnd(4 * g, 30)
    sel = {name: [0] * g for name in prover.SELECTORS}
    values, outs = [0], []
    w = [[0] * g for _ in range(4)]
    pub = {1: rnd(1, 40)[0], 3: rnd(1, 41)[0]}

    def new(v):
        values.append(v % p)
        return len(values) - 1
    for i in range(g):
        if i % 3 == 2 and i > 4:
            j = int(rng.integers(0, rows))
            for k in range(4):
                w[k][i] = new(tcols[k][j])
            sel["q_lookup"][i] = 1
            continue
        pick = lambda t: (outs[int(rng.integers(0, len(outs)))] if outs and rng.integers(0, 4) else (0 if outs else new(fresh[4 * i + t])))  # noqa: E731
        a, b, d = pick(0), pick(1), pick(2)
        for name in qs:
            sel[name][i] = qs[name][i]
        sel["q_o"][i], sel["q_arith"][i] = p - 1, 1
        va, vb, vd = values[a], values[b], values[d]
        c = new(qs["q_m"][i] * va * vb + qs["q_l"][i] * va + qs["q_r"][i] * vb + qs["q_4"][i] * vd + qs["q_c"][i] + pub.get(i, 0))
        outs.append(c)
        w[0][i], w[1][i], w[2][i], w[3][i] = a, b, c, d
    desc = zc.CircuitDescription.from_gates({k: dev_fr(cid, v) for k, v in sel.items()}, *w, num_vars=len(values),
                                            table_cols=[dev_fr(cid, t) for t in tcols],
                                            public_inputs={i: fr_to_mont(cid, [v])[0] for i, v in pub.items()}, curve=cid, device=device)
    return desc, values, pub, outs[len(outs) // 2]


def committer(ctx, oracle_cpu, cid, n):
    pw_canon, _ = tau_powers(oracle_cpu, cid, n + 8)
    return zk.CommitterKey(srs_from_powers(ctx, cid, pw_canon), cid, ctx)


# ---- 6. the closing property of the reference's own test (mod.rs:1243-1380) at 2^20
def test_grand_product_closes_over_compiled_sigma(ctx):
    import torch
    cid, log_n = 0, 20
    n = 1 << log_n
    rng = np.random.default_rng(11)
    nv = n
    ids = rng.integers(1, nv, size=(4, n))
    ids[rng.random((4, n)) < 0.4] = 0
    desc = zc.CircuitDescription.from_gates({}, *ids, num_vars=nv, curve=cid)
    vals = torch.from_numpy(rng.integers(0, 1 << 62, size=(nv, 4), dtype=np.uint64).view(np.int64)).cuda()
    vals[:, 3] &= (1 << 60) - 1
    vals[0] = 0
    wires = zc.assign(desc, vals, ctx)
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    sig = zc.sigma_evals(dom, desc.ins_var, desc.ins_pos, nv, ctx)
    beta, gamma = fr_to_mont(cid, [0x1234567], )[0], fr_to_mont(cid, [0x89ABCDE])[0]
    _, last = permutation.permutation_evals(dom, wires, sig, beta, gamma, return_last=True)
    assert np.array_equal(last, fr_to_mont(cid, [1])[0])
    row = int(np.nonzero(ids[1] != 0)[0][0])
    wires[1][row, 0] ^= 1                                      # one wire cell changed after assign
    _, last = permutation.permutation_evals(dom, wires, sig, beta, gamma, return_last=True)
    assert not np.array_equal(last, fr_to_mont(cid, [1])[0])


# ---- 7 + 8. end to end through compile / assign / prove, and consistency with today's key path
@pytest.mark.parametrize("cid,log_n", [(0, 5), (0, 10), (1, 7), (0, 14)])
def test_compile_assign_prove_verifies(cid, log_n, ctx, oracle_cpu):
    import torch
    from tests.test_prover_gpu import dlogs, oracle_points
    cv = bo.CURVES[cid]
    n = 1 << log_n
    desc, values, pub, an_output = variable_circuit(cid, log_n, 50 + log_n + cid)
    assert desc.size() == n and desc.n_gates < n
    ck = committer(ctx, oracle_cpu, cid, n)
    pk, vk, pre = zc.compile(desc, ck, b"end to end", cid, ctx)
    assert vk.n == n and pk.domain.size() == n
    ca, cd = bo.seeded_scalars(cv, 0x51, 2)
    pub_m = {i: fr_to_mont(cid, [v])[0] for i, v in pub.items()}

    def prove(vals):
        wires = zc.assign(desc, dev_fr(cid, vals), ctx)
        return prover.prove(pk, ck, wires, pub_m, pre, fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0])
    proof = prove(values)
    assert prover.check_identity(pk, proof, pub_m)
    vk_pts = oracle_points(cid, vk)
    dlog = dlogs(cid, ctx, pk, proof)
    for k, pt in vk_pts.items():
        assert pt == bo.ec_mul(cv, dlog[k], (cv.gx, cv.gy)), k
    t = vo.seed_transcript(cv, wo.PlonkTranscript(b"end to end", cv), vk_pts, n)
    ok, _, det = vo.verify_with_trapdoor(cv, log_n, proof.to_bytes(), t, pub, dlog, TAU, ca, cd)
    assert ok, det
    # one assigned value off by one (an arithmetic output: a wrong looked-up value is refused earlier, as ElementNotIndexed): rejected
    wrong = list(values)
    wrong[an_output] = (wrong[an_output] + 1) % cv.r
    bad = prove(wrong)
    t = vo.seed_transcript(cv, wo.PlonkTranscript(b"end to end", cv), vk_pts, n)
    ok, _, _ = vo.verify_with_trapdoor(cv, log_n, bad.to_bytes(), t, pub, dlogs(cid, ctx, pk, bad), TAU, ca, cd)
    assert not ok and not prover.check_identity(pk, bad, pub_m)
    # 8: today's path fed the same sigma evaluations gives the same 20 points and the same first challenge
    old = pk.verifier_key(ck)
    assert dict(vk) == old
    t_old = transcript.seed_transcript(transcript.Transcript(b"end to end", cid), old, n)
    t_rt = zc.VerifierKey.from_bytes(vk.to_bytes(), cid).seed(transcript.Transcript(b"end to end", cid))
    c0 = pre.clone().challenge_scalar(b"x")
    assert np.array_equal(t_old.challenge_scalar(b"x"), c0) and np.array_equal(t_rt.challenge_scalar(b"x"), c0)
    # the sigma the key holds is the definition's
    ins_var, ins_pos = desc.ins_var.cpu().numpy(), desc.ins_pos.cpu().numpy()
    want = expected_evals(omega_tables(oracle_cpu, cid, log_n), n, cr.sigma_numpy(n, ins_var, ins_pos))
    for a, b in zip(pk.sigma_evals, want):
        assert np.array_equal(a.cpu().numpy().view(np.uint64), b)
    torch.cuda.synchronize()
    ck.close()


# ---- 9. an open deferred round
def test_open_round(ctx, oracle_cpu):
    cid, log_n = 0, 6
    n = 1 << log_n
    desc, values, _, _ = variable_circuit(cid, log_n, 77)
    ck = committer(ctx, oracle_cpu, cid, n)
    polys = [dev_fr(cid, bo.seeded_scalars(bo.CURVES[cid], 900 + k, n)) for k in range(2)]
    want = ck.commit_batch(polys)
    ck.commit_begin(polys)
    assert ck.round_pending() == 2
    with pytest.raises(RuntimeError):
        zc.compile(desc, ck, b"x", cid, ctx)
    assert ck.round_pending() == 2                             # nothing was queued
    # the two entry points use memory of their own: they run inside the open round (include/ark_plonk_amd.h)
    dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
    sig, pos = zc.sigma_evals(dom, desc.ins_var, desc.ins_pos, desc.num_vars, ctx, positions=True)
    assert np.array_equal(pos.cpu().numpy().view(np.uint32).astype(np.int64),
                          cr.sigma_numpy(n, desc.ins_var.cpu().numpy(), desc.ins_pos.cpu().numpy()))
    wires = zc.assign(desc, dev_fr(cid, values), ctx)
    assert len(wires) == 4 and ck.round_pending() == 2
    assert ck.round_end(2) == want                             # the caller's round ends with its own points
    pk, vk, _ = zc.compile(desc, ck, b"x", cid, ctx)
    assert ck.round_pending() == 0 and vk.n == n
    # assign refuses a non-zero value of the zero variable
    values[0] = 5
    with pytest.raises(ValueError):
        zc.assign(desc, dev_fr(cid, values), ctx)
    ck.close()
