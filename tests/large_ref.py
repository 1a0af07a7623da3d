"""Vectorised references for the large-size GPU tests: field-wide random operands, powers of a field element, the decimation
identity of the NTT, and the grand products' per-row numerators and denominators.  Every O(n) step runs on numpy or on the C++
restatement's Fr ops (`oracle.cpu.fr_op`), never on per-element Python integers, so the helpers work up to 2^27 elements.
Checked against `oracle/bigint_oracle.py` at small n by tests/test_large_ref.py."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import bigint_oracle as bo

U64 = np.uint64
_ALL = np.iinfo(np.uint64).max


def r_limbs(cid) -> np.ndarray:
    r = bo.CURVES[cid].r
    return np.array([(r >> (64 * k)) & _ALL for k in range(4)], dtype=U64)


def _lt(a, b):
    """a < b, limb-lexicographic (most significant limb last), for (n, 4) a and (4,) b."""
    lt = np.zeros(a.shape[0], dtype=bool)
    eq = np.ones(a.shape[0], dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (a[:, k] < b[k])
        eq &= a[:, k] == b[k]
    return lt


def is_canonical(cid, a) -> bool:
    """Every row of the (n, 4) limbs a is below r."""
    a = np.asarray(a, dtype=U64).reshape(-1, 4)
    return bool(_lt(a, r_limbs(cid)).all())


def full_range(cid, n, seed) -> np.ndarray:
    """n elements uniform over [0, r) as (n, 4) uint64 limbs (read as Montgomery residues, uniform over the field too): random
    words with the top limb cut to r's bit length, the rows that reach r redrawn."""
    rl = r_limbs(cid)
    shift = U64(64 - int(rl[3]).bit_length())
    rng = np.random.default_rng(seed)

    def draw(k):
        w = rng.bit_generator.random_raw(4 * k).reshape(k, 4)
        w[:, 3] >>= shift
        return w

    out = draw(n)
    bad = np.flatnonzero(out[:, 3] >= rl[3])
    bad = bad[~_lt(out[bad], rl)]
    while bad.size:
        out[bad] = draw(bad.size)
        bad = bad[~_lt(out[bad], rl)]
    return out


def near_r(cid, n, seed) -> np.ndarray:
    """n elements uniform over [r - 2^64, r): r - 1 - u with u a uniform 64-bit word."""
    rl = r_limbs(cid)
    u = np.random.default_rng(seed).integers(0, _ALL, size=n, dtype=U64, endpoint=True)
    out = np.empty((n, 4), dtype=U64)
    top = rl[0] - U64(1)                           # r is odd: no borrow out of the low limb here
    out[:, 0] = top - u
    borrow = (u > top).astype(U64)
    for k in (1, 2, 3):
        out[:, k] = rl[k] - borrow
        borrow = borrow & (rl[k] == 0)
    return out


def r_minus_one(cid, n) -> np.ndarray:
    """n copies of r - 1 (the Montgomery residue of -R^-1: the largest canonical limb vector)."""
    v = r_limbs(cid).copy()
    v[0] -= U64(1)
    return np.tile(v, (n, 1))


_P64 = ctypes.POINTER(ctypes.c_uint64)
_PAR_MIN = 1 << 15


def _ptr(a):
    return a.ctypes.data_as(_P64)


def _workers(oracle_cpu):
    return max(1, oracle_cpu.num_threads())


def fr_op(oracle_cpu, cid, op, a, b) -> np.ndarray:
    """oracle_cpu.fr_op cut into row blocks run on the restatement's thread count (the C++ loop is serial; ctypes drops the GIL)."""
    x = np.ascontiguousarray(a, dtype=U64).reshape(-1, 4)
    y = np.ascontiguousarray(b, dtype=U64).reshape(-1, 4)
    n = x.shape[0]
    assert y.shape[0] == n
    if n < _PAR_MIN:
        return oracle_cpu.fr_op(cid, op, x, y)
    out = np.empty_like(x)
    code = {"mul": 0, "add": 1, "sub": 2}[op]
    L = oracle_cpu.lib()
    step = -(-n // (4 * _workers(oracle_cpu)))
    with ThreadPoolExecutor(_workers(oracle_cpu)) as ex:
        jobs = [ex.submit(L.ora_fr_op, cid, code, _ptr(x[lo:]), _ptr(y[lo:]), min(step, n - lo), _ptr(out[lo:]))
                for lo in range(0, n, step)]
        assert all(j.result() == 0 for j in jobs)
    return out


def witnesses(oracle_cpu, cid, jobs) -> list:
    """oracle_cpu.kzg_witness(cid, coeffs, z) for every (coeffs, z) of jobs, several at a time (each division is a serial Horner loop)."""
    with ThreadPoolExecutor(_workers(oracle_cpu)) as ex:
        return list(ex.map(lambda j: oracle_cpu.kzg_witness(cid, j[0], j[1]), jobs))


def evaluations(oracle_cpu, cid, jobs) -> np.ndarray:
    """p(z) = p_0 + z w_0 (Montgomery limbs) for every (p, z) of jobs, w the restatement's witness of p; one witness alive per thread."""
    def one(j):
        p, z = j
        w = oracle_cpu.kzg_witness(cid, p, z)
        if w.shape[0] == 0:
            return p[0]
        return oracle_cpu.fr_op(cid, "add", p[:1], oracle_cpu.fr_op(cid, "mul", np.asarray(z, dtype=U64).reshape(1, 4), w[:1]))[0]
    with ThreadPoolExecutor(_workers(oracle_cpu)) as ex:
        return np.stack(list(ex.map(one, jobs)))


def mont(oracle_cpu, cid, vals) -> np.ndarray:
    """Python ints (canonical) -> (len, 4) Montgomery limbs."""
    return oracle_cpu.convert(cid, "fr", True, oracle_cpu.ints_to_limbs([v % bo.CURVES[cid].r for v in vals], 4))


def powers(oracle_cpu, cid, base, n) -> np.ndarray:
    """Montgomery limbs of base^i, i < n, by doubling: pw[k:2k] = pw[0:k] * base^k (as conftest.tau_powers does for tau)."""
    r = bo.CURVES[cid].r
    pw = np.empty((n, 4), dtype=U64)
    if n == 0:
        return pw
    pw[0] = mont(oracle_cpu, cid, [1])[0]
    k = 1
    while k < n:
        m = min(k, n - k)
        step = mont(oracle_cpu, cid, [pow(base, k, r)])
        pw[k:k + m] = fr_op(oracle_cpu, cid, "mul", pw[:m], np.broadcast_to(step, (m, 4)))
        k *= 2
    return pw


def decimated(oracle_cpu, cid, kind, log_n, log_m, x, t) -> np.ndarray:
    """Outputs t, t + s, t + 2s, ... (s = 2^(log_n - log_m)) of the 2^log_n-point fft (kind 0) or coset_fft (kind 2) of x, len(x) <= 2^log_m:
    y[s k + t] = sum_j x_j g^j w_n^((s k + t) j) = [coset_]fft_{2^log_m}(x_j w_n^(t j))_k, with w_n^s = w_m the smaller domain's root."""
    assert kind in (bo.KIND_FFT, bo.KIND_COSET_FFT) and x.shape[0] <= 1 << log_m <= 1 << log_n
    cv = bo.CURVES[cid]
    tw = powers(oracle_cpu, cid, pow(cv.root_of_unity(log_n), t, cv.r), x.shape[0])
    return oracle_cpu.ntt(cid, kind, log_m, fr_op(oracle_cpu, cid, "mul", x, tw))


def _bcast(c, n):
    return np.broadcast_to(np.asarray(c, dtype=U64).reshape(1, 4), (n, 4))


def _prod(oracle_cpu, cid, terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = fr_op(oracle_cpu, cid, "mul", acc, t)
    return acc


def perm_terms(oracle_cpu, cid, log_n, wires, sigmas, beta, gamma):
    """(N, D), (n, 4) Montgomery: N_i = prod_k (w_k[i] + beta K_k w^i + gamma), D_i = prod_k (w_k[i] + beta sigma_k[i] + gamma)
    (permutation/mod.rs:626-647, as bo.perm_product).  wires, sigmas: Montgomery columns; beta, gamma: Montgomery (4,) limbs."""
    cv = bo.CURVES[cid]
    n = 1 << log_n
    op = functools.partial(fr_op, oracle_cpu)
    b, g = _bcast(beta, n), _bcast(gamma, n)
    roots = powers(oracle_cpu, cid, cv.root_of_unity(log_n), n)
    broots = op(cid, "mul", roots, b)
    num, den = [], []
    for k in range(4):
        kb = op(cid, "mul", broots, _bcast(mont(oracle_cpu, cid, [bo.PERM_K[k]])[0], n)) if bo.PERM_K[k] != 1 else broots
        num.append(op(cid, "add", op(cid, "add", wires[k], kb), g))
        den.append(op(cid, "add", op(cid, "add", wires[k], op(cid, "mul", sigmas[k], b)), g))
    return _prod(oracle_cpu, cid, num), _prod(oracle_cpu, cid, den)


def lookup_terms(oracle_cpu, cid, f, t, h1, h2, delta, eps):
    """(N, D), (n, 4) Montgomery, i + 1 taken mod n (mod.rs:771-772, as bo.lookup_product):
    N_i = (1 + delta)(eps + f_i)(eps(1 + delta) + t_i + delta t_{i+1}),  D_i = (eps(1 + delta) + h1_i + delta h2_i)(eps(1 + delta) + h2_i + delta h1_{i+1})."""
    n = f.shape[0]
    op = functools.partial(fr_op, oracle_cpu)
    one = mont(oracle_cpu, cid, [1])
    opd = op(cid, "add", one, np.asarray(delta, dtype=U64).reshape(1, 4))
    e1d = op(cid, "mul", np.asarray(eps, dtype=U64).reshape(1, 4), opd)
    d, e, o, e1 = _bcast(delta, n), _bcast(eps, n), _bcast(opd, n), _bcast(e1d, n)
    t_n, h1_n = np.roll(t, -1, axis=0), np.roll(h1, -1, axis=0)
    num = _prod(oracle_cpu, cid, [o, op(cid, "add", e, f), op(cid, "add", op(cid, "add", e1, t), op(cid, "mul", d, t_n))])
    den = op(cid, "mul", op(cid, "add", op(cid, "add", e1, h1), op(cid, "mul", d, h2)),
             op(cid, "add", op(cid, "add", e1, h2), op(cid, "mul", d, h1_n)))
    return num, den


def check_product(oracle_cpu, cid, z, last, num, den):
    """z[0] = 1, z[i+1] D_i = z[i] N_i for i < n - 1 and last D_{n-1} = z[n-1] N_{n-1}; every z and last canonical.  With every D_i
    nonzero this fixes z and last exactly.  Returns the first failing row or None."""
    n = z.shape[0]
    zz = np.concatenate([z, np.asarray(last, dtype=U64).reshape(1, 4)])
    assert is_canonical(cid, zz), "non-canonical product values"
    assert not (den == 0).all(axis=1).any(), "zero denominator"
    assert np.array_equal(z[0], mont(oracle_cpu, cid, [1])[0]), "z[0] != 1"
    lhs = fr_op(oracle_cpu, cid, "mul", zz[1:], den)
    rhs = fr_op(oracle_cpu, cid, "mul", zz[:n], num)
    bad = np.flatnonzero((lhs != rhs).any(axis=1))
    return int(bad[0]) if bad.size else None
