"""The opening witness (kzg.hip: 64-coefficient chunks, one 1024-lane scan) and the batched evaluations past their scan thresholds,
element by element against the C++ restatement's synthetic division: m = 65 536 (one chunk per lane), 65 537 (two per lane, then
empty lanes), 3 * 65 536 + 65 (four per lane, a one-element last chunk), 2^20 + 6 and 2^22 + 3, on full-range ragged polynomials."""
import numpy as np
import pytest

import ark_plonk_amd as zk
import large_ref as lr
from ark_plonk_amd import linearisation
from oracle import bigint_oracle as bo

pytestmark = pytest.mark.gpu

LENGTHS = (1 << 16, (1 << 16) + 1, 3 * (1 << 16) + 65, (1 << 20) + 6, (1 << 22) + 3)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def _points(oracle_cpu, cid, m, seed):
    """(name, Montgomery limbs): random z, 0, 1, -1, the limb vector r - 1, a primitive 64th root (z^CHUNK = 1) and z w, w the root of
    the domain the prover's polynomials of m coefficients live on."""
    cv = bo.CURVES[cid]
    z = lr.full_range(cid, 1, seed)
    zi = oracle_cpu.limbs_to_ints(oracle_cpu.convert(cid, "fr", False, z))[0]
    w = cv.root_of_unity((m - 7).bit_length())
    vals = lr.mont(oracle_cpu, cid, [0, 1, cv.r - 1, cv.root_of_unity(6), zi * w % cv.r])
    return [("z", z[0]), ("0", vals[0]), ("1", vals[1]), ("-1", vals[2]), ("limbs r-1", lr.r_minus_one(cid, 1)[0]),
            ("root64", vals[3]), ("z*w", vals[4])]


def _rlc(oracle_cpu, cid, polys, chi):
    """sum_k chi^k p_k over the longest length, with the restatement's Fr ops."""
    m = max(p.shape[0] for p in polys)
    comb = np.zeros((m, 4), dtype=np.uint64)
    chi_pow = lr.mont(oracle_cpu, cid, [1])
    for p in polys:
        term = lr.fr_op(oracle_cpu, cid, "mul", p, np.broadcast_to(chi_pow, p.shape))
        comb[: p.shape[0]] = lr.fr_op(oracle_cpu, cid, "add", comb[: p.shape[0]], term)
        chi_pow = oracle_cpu.fr_op(cid, "mul", chi_pow, chi.reshape(1, 4))
    return comb


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("m", LENGTHS)
def test_witness_and_evaluations_vs_restatement(cid, m, ctx, oracle_cpu):
    """zk.msm.kzg_witness whole (canonical output) against the restatement's witness of the random linear combination, for one polynomial
    and for 11 ragged ones (the longest not first), at seven points; linearisation.evaluate_batch at the same points, every value
    against p(z) = p_0 + z w_0 with w the restatement's witness of p alone; and a cancelling batch (p, p, chi = -1): exactly zero."""
    seed = 0x0B00 + 16 * cid + LENGTHS.index(m)
    lens = (m - 5, m // 2, m, m - 1, 3, m, m - 64, m - 63, 1, m // 3, m - 2)
    polys = [lr.full_range(cid, ln, seed * 16 + k) for k, ln in enumerate(lens)]
    polys[5][:64] = lr.near_r(cid, 64, seed)
    d_polys = [dev(p) for p in polys]
    chi = lr.full_range(cid, 1, seed + 1)[0]
    pts = _points(oracle_cpu, cid, m, seed + 2)
    combs = {"one": polys[2], "eleven": _rlc(oracle_cpu, cid, polys, chi)}
    batches = {"one": [d_polys[2]], "eleven": d_polys}
    exp = lr.witnesses(oracle_cpu, cid, [(combs[b], z) for b in combs for _, z in pts])
    for b in combs:
        for name, z in pts:
            got = host(zk.msm.kzg_witness(batches[b], z, chi, cid, ctx))
            want = oracle_cpu.convert(cid, "fr", False, exp.pop(0))
            assert got.shape == (m - 1, 4) and np.array_equal(got, want), (b, name)
    # evaluations: every (polynomial, point) pair of the batch
    pairs = [(k, name, z) for k in range(len(polys)) for name, z in pts]
    want = lr.evaluations(oracle_cpu, cid, [(polys[k], z) for k, _, z in pairs])
    vals = linearisation.evaluate_batch([d_polys[k] for k, _, _ in pairs], np.stack([z for _, _, z in pairs]), cid, ctx)
    for (k, name, _), v, e in zip(pairs, vals, want):
        assert np.array_equal(v, e), (k, lens[k], name)
    # (p - p) / (X - z) = 0: the canonical output is all-zero limbs
    minus_one = lr.mont(oracle_cpu, cid, [bo.CURVES[cid].r - 1])[0]
    zero = host(zk.msm.kzg_witness([d_polys[2], d_polys[2]], pts[0][1], minus_one, cid, ctx))
    assert zero.shape == (m - 1, 4) and not zero.any()
