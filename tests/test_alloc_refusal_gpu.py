"""What happens after the HIP runtime refuses an allocation.

The runtime keeps the last error of the calling thread until hipGetLastError() reads it (ROCm 7), and the library checks
hipGetLastError() behind its kernel launches: an allocation error that was handled but not read away would come back from the next
launch check, for work that was queued without fault.  The first test measures that behaviour of the runtime on the card -- it is
what tests/sanitize/fake_hip.cpp models -- and the others drive the library through its public ABI across a refused zk_dev_alloc.

Nothing here exhausts memory or faults anything: the one refused request asks for twice the card's total memory, which the runtime
answers with an error code without touching memory anyone uses."""
import ctypes

import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib
from tests.conftest import srs_from_powers, tau_powers

pytestmark = pytest.mark.gpu

N_TABLE = 1 << 13          # the smallest length of the window-table path (ZK_PRE_MIN_N)


def _total_memory():
    import torch
    return int(torch.cuda.mem_get_info()[1])


def _refused_dev_alloc(ctx):
    """zk_dev_alloc of twice the card's memory: ZK_ERR_OOM and a null pointer (a runtime that grants it: freed at once, and a failure)."""
    p = ctypes.c_void_p(0xDEAD)
    rc = _lib.lib().zk_dev_alloc(ctx.handle, 2 * _total_memory(), ctypes.byref(p))
    if rc == _lib.ZK_OK:
        _lib.lib().zk_dev_free(ctx.handle, p)
        pytest.fail("the runtime granted an allocation of twice the card's total memory")
    assert rc == _lib.ZK_ERR_OOM and not p.value


def test_runtime_last_error_is_kept_until_read(ctx):
    """hipMalloc refused -> a later hipMalloc / hipFree that succeed do not clear the error -> the first hipGetLastError() returns the
    refusal's code, the second hipSuccess.  Called on the libamdhip64 the process already holds (the instance the project's library is
    bound to, not a second copy)."""
    _lib.lib()
    with open("/proc/self/maps") as f:
        paths = [line.split()[-1] for line in f if "libamdhip64" in line]
    assert paths, "no libamdhip64 is mapped into the process"
    hip = ctypes.CDLL(paths[0])
    hip.hipMalloc.restype, hip.hipMalloc.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.restype, hip.hipFree.argtypes = ctypes.c_int, [ctypes.c_void_p]
    hip.hipGetLastError.restype, hip.hipGetLastError.argtypes = ctypes.c_int, []
    hip.hipGetLastError()                                   # whatever an earlier test left behind
    p = ctypes.c_void_p()
    refused = hip.hipMalloc(ctypes.byref(p), 2 * _total_memory())
    if refused == 0:
        hip.hipFree(p)
        pytest.fail("the runtime granted an allocation of twice the card's total memory")
    q = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(q), 256) == 0 and q.value
    assert hip.hipFree(q) == 0
    first, second = hip.hipGetLastError(), hip.hipGetLastError()
    print(f"hipMalloc refused with {refused}; hipGetLastError() after a successful hipMalloc + hipFree: {first}, then {second}")
    assert first == refused, "a successful call reset the last error (or it was never recorded)"
    assert second == 0, "reading the last error did not reset it"


@pytest.fixture(scope="module")
def table_keys(ctx, oracle_cpu):
    """Per curve: a key of 2^13 points tau^i G with its window table, the points on the host, scalars and the oracle's MSM of them."""
    out = {}
    for cid in (0, 1):
        bases = srs_from_powers(ctx, cid, tau_powers(oracle_cpu, cid, N_TABLE)[0])
        bases_h = bases.cpu().numpy().view(np.uint64)
        ck = zk.CommitterKey(bases, cid, ctx).precompute()
        assert ck.table_windows() > 0
        scal = np.random.default_rng(130 + cid).integers(0, 1 << 63, size=(N_TABLE, 4), dtype=np.uint64)
        scal[:, 3] &= np.uint64((1 << 60) - 1)               # canonical on both curves
        out[cid] = (ck, bases_h, scal, oracle_cpu.msm_g1(cid, bases_h, scal))
    yield out
    for ck, *_ in out.values():
        ck.close()


def _assert_point(got, exp, cid):
    exp_xy, exp_inf = exp
    assert got.infinity == bool(exp_inf) and np.array_equal(got.xy(), exp_xy), cid


@pytest.mark.parametrize("cid", [0, 1])
def test_refused_alloc_leaves_the_ctx_usable(cid, ctx, oracle_cpu, golden, table_keys):
    """After a refused zk_dev_alloc, and without anyone reading the runtime's error in between, the next calls of the same thread --
    one of each family that checks hipGetLastError() behind its launches -- return ZK_OK with the oracle's results.  Host arrays in
    and out: no other user of the runtime runs between the refusal and the calls."""
    ck, _, scal, want_table = table_keys[cid]
    rng = np.random.default_rng(17 + cid)
    x = rng.integers(0, 1 << 63, size=(8, 4), dtype=np.uint64)
    x[:, 3] &= np.uint64((1 << 60) - 1)
    want_ntt = oracle_cpu.ntt(cid, 0, 3, x)
    b33, s33 = golden[cid]["srs_1024"][:33], golden[cid]["msm_srs_33_scalars"]
    want_33 = oracle_cpu.msm_g1(cid, b33, s33)
    dom = zk.Radix2EvaluationDomain.new(8, cid, ctx)

    calls = (lambda: np.array_equal(dom.fft(x), want_ntt),                                                       # forward NTT of 8 elements
             lambda: _assert_point(zk.VariableBaseMSM.multi_scalar_mul(b33, s33, cid, ctx=ctx), want_33, cid) or True,      # per-window MSM, 33 points
             lambda: _assert_point(ck.msm(scal), want_table, cid) or True)                                       # table path at 2^13 points
    _refused_dev_alloc(ctx)
    for call in calls:                  # one refusal, then the three families in turn
        assert call()
    for call in calls[1:]:              # ... and each of the other two as the FIRST call behind a refusal
        _refused_dev_alloc(ctx)
        assert call()


def test_refused_alloc_inside_an_open_round(ctx, table_keys):
    """Two jobs of 2^13 queued in a deferred round, the refusal, then the round closed: the two points of the blocking batch."""
    import torch
    ck, _, scal, _ = table_keys[0]
    polys = [torch.from_numpy(np.roll(scal, k, axis=0).view(np.int64)).cuda() for k in (0, 1)]
    want = ck.commit_batch(polys)
    assert want[0] != want[1]
    try:
        assert ck.commit_begin(polys) == 2
        _refused_dev_alloc(ctx)
        assert ck.round_end(2) == want
    finally:
        if ck.round_pending():
            ck.round_abort()
