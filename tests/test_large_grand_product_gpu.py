"""The grand products past one 256-position tile per lane of the tile-total scan (grand_product.hip: 1024 lanes, so several tiles per lane
above n = 2^18), every element checked on full-range columns: z[0] = 1, z[i+1] D_i = z[i] N_i for every row and the returned last value
closes the product.  With every D_i nonzero that fixes z exactly; N and D come from the C++ restatement's Fr ops (tests/large_ref.py)."""
import numpy as np
import pytest

import ark_plonk_amd as zk
import large_ref as lr
from ark_plonk_amd import permutation

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("n", [1 << 18, (1 << 18) + 257, 1 << 20, 1 << 22])
def test_grand_products_every_row(cid, n, ctx, oracle_cpu):
    """permutation_evals on the 2^18 (1024 tiles), 2^20 and 2^22 domains; lookup_permutation_evals at the same sizes and at 2^18 + 257
    (1026 tiles, the last one partial)."""
    seed = 0x6900 + 8 * cid + n.bit_length()
    cols = [lr.full_range(cid, n, seed * 16 + k) for k in range(8)]
    cols[0][:256] = lr.near_r(cid, 256, seed)
    cols[5][-300:] = lr.r_minus_one(cid, 300)
    ch = lr.full_range(cid, 4, seed + 1)
    d = [dev(c) for c in cols]
    if n & (n - 1) == 0:
        log_n = n.bit_length() - 1
        dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
        z, last = permutation.permutation_evals(dom, d[:4], d[4:], ch[0], ch[1], return_last=True)
        num, den = lr.perm_terms(oracle_cpu, cid, log_n, cols[:4], cols[4:], ch[0], ch[1])
        row = lr.check_product(oracle_cpu, cid, host(z), last, num, den)
        assert row is None, ("permutation", row)
    p, last = permutation.lookup_permutation_evals(ctx, cid, d[0], d[1], d[2], d[3], ch[2], ch[3], return_last=True)
    num, den = lr.lookup_terms(oracle_cpu, cid, cols[0], cols[1], cols[2], cols[3], ch[2], ch[3])
    row = lr.check_product(oracle_cpu, cid, host(p), last, num, den)
    assert row is None, ("lookup", row)
