"""Inner-product-argument polynomial commitment: ark-poly-commit 0.3 `ipa_pc::InnerProductArgPC`, the reference's second
`HomomorphicCommitment` (plonk-core/src/commitment.rs:50-91), without hiding and degree bounds -- what ark-plonk uses
(prover.rs:582-618 passes no rng and no degree bounds).

    pp = IpaUniversalParams.setup(max_degree, "bls12_381", digest="blake2b")   # PC::setup: the generators hashed to the curve, on the device
    ck = pp.trim(supported_degree)                      # PC::trim: a prefix of d + 1 = 2^k points (d + 1 = 2n for a circuit of n)
    ck = IpaCommitterKey(comm_key, h, "bls12_381")      # ... or a key of the caller's own points
    comms = ck.commit(polys)
    proof = ck.open(polys, comms, z, chi, digest="blake2b")
    assert ck.check(comms, z, values, proof, chi, digest="blake2b")
    assert ck.batch_check([IpaOpening(comms, z, values, proof, chi), ...])     # any number of openings, ONE MSM over the key
    bad = ck.locate_invalid(openings)                                          # which ones fail, by bisection
    proof = prover.prove(pk, ck, ...)                                          # a PLONK proof over this commitment (prover.py)
    ok = IpaBatchVerifier(vk, n, seeded, ca, cd, ck).verify(proofs, pis)       # ... and its verification (verifier.py)

Every group operation and every O(n) vector pass runs in libark_plonk_amd.so: commit and the verifier's final-key MSM are the SRS
MSM over the registered key, the opening's rounds are zk_ipa_round_dev / zk_ipa_fold_dev (include/ark_plonk_amd.h).  The device
never hashes a transcript: every challenge is derived here, by `transcript_hash`, the ONE place that holds the byte encodings of the
Fiat-Shamir transcript.  The key's generators are hashed on the device (zk_ipa_sample_generators_dev, csrc/h2c.cuh); the host
statement of that rule -- `generator_preimage`, `from_random_bytes`, `sample_generators_host` -- is the ONE place on this side that
holds its encodings.  Parity with the Rust crate is unpinned for both (its source is not vendored): those functions state what they
assume.

Points cross this module as Python tuples (x, y) of canonical base-field integers, None for the point at infinity; field
elements as canonical integers.
"""
from __future__ import annotations

import ctypes
import hashlib
import secrets
from dataclasses import dataclass, field

import numpy as np

from ._lib import check, lib
from .context import Context, default_context, ptr_of
from .curves import fq_from_mont, fq_to_mont, fr_from_mont, fr_to_mont, get_curve, ints_to_limbs
from .msm import CommitterKey, segments_msm, sum_partials

DIGESTS = {"blake2b": hashlib.blake2b, "blake2s": hashlib.blake2s}


def transcript_hash(curve, digest: str, items) -> int:
    """The Fiat-Shamir hash of ipa_pc (`compute_random_oracle_challenge` over `to_bytes!`), AS RECALLED -- every encoding-dependent
    choice of this module lives here, so that a comparison against the Rust crate corrects them in one place.

    items: a sequence of ("fr", int) and ("g1", (x, y) | None) in transcript order.  Assumed encodings:
      * an Fr element: its canonical value, 32 bytes little-endian;
      * an affine point: x || y, each canonical little-endian in the base field's byte length (48 on BLS12-381, 32 on BN254), then
        one byte for the infinity flag; the point at infinity is (x = 0, y = 1, flag = 1);
      * H(bytes): for i = 0, 1, ...: D(bytes || u64_le(i)); the first 32 bytes little-endian, bits from MODULUS_BITS up cleared (one
        for BLS12-381 Fr, two for BN254 Fr); the first value below r is the challenge.
    digest: "blake2b" (the reference's test_full and benchmarks) or "blake2s" (its batch_test!)."""
    cv = get_curve(curve)
    fq_len = 8 * cv.fq_limbs
    buf = bytearray()
    for kind, v in items:
        if kind == "fr":
            buf += int(v).to_bytes(32, "little")
        elif kind == "g1":
            if v is None:
                buf += (0).to_bytes(fq_len, "little") + (1).to_bytes(fq_len, "little") + b"\x01"
            else:
                buf += int(v[0]).to_bytes(fq_len, "little") + int(v[1]).to_bytes(fq_len, "little") + b"\x00"
        else:
            raise ValueError(f"unknown transcript item {kind!r}")
    h = DIGESTS[digest]
    mask = (1 << cv.r.bit_length()) - 1
    i = 0
    while True:
        out = h(bytes(buf) + i.to_bytes(8, "little")).digest()
        x = int.from_bytes(out[:32], "little") & mask
        if x < cv.r:
            return x
        i += 1


def g1_compress(curve, p) -> bytes:
    """ark-serialize 0.3 `GroupAffine::serialize` of (x, y) | None: x little-endian in the base field's byte length, bit 7 of the last
    byte set when y is the larger of (y, -y), bit 6 for infinity (x = 0) -- the rules zk_g1_decompress_batch_dev reads."""
    cv = get_curve(curve)
    g = 8 * cv.fq_limbs
    if p is None:
        return bytes(g - 1) + b"\x40"
    b = bytearray(int(p[0]).to_bytes(g, "little"))
    if int(p[1]) > cv.q - int(p[1]):
        b[-1] |= 0x80
    return bytes(b)


# ---- ipa_pc::setup: the generators of a committer key, hashed to the curve
GENERATOR_TAG = b"PC-DL-2020"
G1_COFACTOR = {"bls12_381": 0x396c8c005555e1568c00aaab0000aaab, "bn254": 1}
DIGEST_IDS = {"blake2s": 0, "blake2b": 1}                 # ZK_H2C_BLAKE2S, ZK_H2C_BLAKE2B
# per-point statuses (include/ark_plonk_amd.h)
ZK_G1_OK, ZK_G1_BAD_FLAGS, ZK_G1_X_NOT_REDUCED, ZK_G1_NOT_ON_CURVE, ZK_G1_NOT_IN_SUBGROUP, ZK_G1_INF_FLAG_X_NONZERO, ZK_H2C_EXHAUSTED = range(7)
H2C_DEFAULT_MAX_TRIES = 1024


def generator_preimage(i: int, j: int | None = None) -> bytes:
    """What `ipa_pc::sample_generators` hashes for generator i, AS RECALLED (ark-poly-commit 0.3; unpinned against the crate, like
    `transcript_hash`): the protocol name and `to_bytes!(i as u64)` -- a u64 little-endian -- for the first attempt, and the same
    followed by `to_bytes!(j as u64)` for the retries j = 0, 1, ... after a digest that is no point."""
    out = GENERATOR_TAG + int(i).to_bytes(8, "little")
    return out if j is None else out + int(j).to_bytes(8, "little")


def from_random_bytes(curve, data: bytes):
    """`GroupAffine::from_random_bytes` over `Fp::from_random_bytes_with_flags::<SWFlags>`, AS RECALLED (ark-ec / ark-ff 0.3):
    (status, point) with point (x, y), or None for the point at infinity (status ZK_G1_OK) and for no point (any other status).
      * min(len, G) bytes are copied into a zeroed buffer of G bytes, G the byte length of a compressed point;
      * the flags are the top two bits of byte G - 1: bit 7 "y is the larger of (y, -y)", bit 6 "infinity";
      * x is the buffer little-endian with every bit from MODULUS_BITS up cleared; x >= q is no point (ZK_G1_X_NOT_REDUCED), and is
        found before the flags are looked at; both flags are no point (ZK_G1_BAD_FLAGS);
      * the infinity flag gives infinity with x = 0 and no point otherwise (ZK_G1_INF_FLAG_X_NONZERO);
      * else y = sqrt(x^3 + b), a non-residue being no point (ZK_G1_NOT_ON_CURVE), and of (y, -y) the one the flag names, by ark's
        order on canonical integers.  There is no subgroup check."""
    cv = get_curve(curve)
    g = 8 * cv.fq_limbs
    buf = bytearray(g)
    data = bytes(data)[:g]
    buf[:len(data)] = data
    flags = buf[g - 1] >> 6
    x = int.from_bytes(buf, "little") & ((1 << cv.q.bit_length()) - 1)
    if x >= cv.q:
        return ZK_G1_X_NOT_REDUCED, None
    if flags == 3:
        return ZK_G1_BAD_FLAGS, None
    if flags & 1:
        return (ZK_G1_OK, None) if x == 0 else (ZK_G1_INF_FLAG_X_NONZERO, None)
    rhs = (x * x * x + cv.b) % cv.q
    y = pow(rhs, (cv.q + 1) // 4, cv.q)                 # both base fields are 3 mod 4
    if y * y % cv.q != rhs:
        return ZK_G1_NOT_ON_CURVE, None
    if (y > cv.q - y) != bool(flags & 2):
        y = cv.q - y
    return ZK_G1_OK, (x, y)


def _g1_mul_any(cv, k: int, p):
    """k * p for ANY point of the curve (not only of the subgroup) by affine double-and-add over Python integers"""
    q = cv.q

    def plus(p1, p2):
        if p1 is None:
            return p2
        if p2 is None:
            return p1
        (x1, y1), (x2, y2) = p1, p2
        if x1 == x2:
            if (y1 + y2) % q == 0:
                return None
            lam = 3 * x1 * x1 * pow(2 * y1, -1, q) % q
        else:
            lam = (y2 - y1) * pow(x2 - x1, -1, q) % q
        x3 = (lam * lam - x1 - x2) % q
        return x3, (lam * (x1 - x3) - y1) % q

    acc = None
    for bit in bin(k)[2:]:
        acc = plus(acc, acc)
        if bit == "1":
            acc = plus(acc, p)
    return acc


def sample_generators_host(curve, n: int, first_index: int = 0, digest: str = "blake2b", max_tries: int = 0) -> list:
    """`ipa_pc::sample_generators` on Python integers, the host statement of what zk_ipa_sample_generators_dev computes: for every
    index first_index <= i < first_index + n the triple (status, generator, attempts).  The generator is affine(cofactor * P) -- the
    full cofactor of G1 -- for the first digest P = from_random_bytes(D(generator_preimage(i[, j]))) that is a point; max_tries (0:
    1024) caps the attempts, and an index that runs out has status ZK_H2C_EXHAUSTED.  Milliseconds per point: for checks, never on a
    compute path."""
    cv = get_curve(curve)
    h, cap = DIGESTS[digest], max_tries or H2C_DEFAULT_MAX_TRIES
    out = []
    for i in range(first_index, first_index + n):
        res = (ZK_H2C_EXHAUSTED, None, cap)
        for a in range(cap):
            st, p = from_random_bytes(cv, h(generator_preimage(i, None if a == 0 else a - 1)).digest())
            if st == ZK_G1_OK:
                res = (ZK_G1_OK, None if p is None else _g1_mul_any(cv, G1_COFACTOR[cv.name], p), a + 1)
                break
        out.append(res)
    return out


def next_power_of_two(k: int) -> int:
    return 1 if k <= 1 else 1 << (k - 1).bit_length()


def _sample_generators_raw(curve, n: int, first_index: int, digest: str, ctx, max_tries: int):
    """zk_ipa_sample_generators_dev with every output: (xy (n, 2L) int64, inf, tries int32, status, wave_rounds int32), device tensors"""
    import torch
    cv = get_curve(curve)
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    L = cv.fq_limbs
    xy = torch.empty((n, 2 * L), dtype=torch.int64, device=dev)
    inf = torch.empty(n, dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    tries = torch.empty(n, dtype=torch.int32, device=dev)
    rounds = torch.empty(lib().zk_ipa_sample_generators_waves(n), dtype=torch.int32, device=dev)
    ctx.use_torch_stream()
    check(lib().zk_ipa_sample_generators_dev(ctx.handle, cv.curve_id, DIGEST_IDS[digest], first_index, n, max_tries, ptr_of(xy), ptr_of(inf),
                                             ptr_of(tries), ptr_of(st), ptr_of(rounds)), "zk_ipa_sample_generators_dev")
    return xy, inf, tries, st, rounds


def sample_generators(curve, n: int, first_index: int = 0, digest: str = "blake2b", ctx: Context | None = None, max_tries: int = 0):
    """Generators first_index .. first_index + n of `ipa_pc::sample_generators` derived on the device: (xy, inf), device tensors in the
    layout CommitterKey registers from ((n, 2L) affine Montgomery limbs, n infinity flags).  Ranks or chunks may each derive a range.
    Raises when an index has a non-zero status (max_tries attempts, 0: 1024, and no point)."""
    xy, inf, _, st, _ = _sample_generators_raw(curve, n, first_index, digest, ctx, max_tries)
    if n and int(st.max()) != 0:
        bad = int((st != 0).nonzero()[0])
        raise RuntimeError(f"sample_generators: index {first_index + bad} has status {int(st[bad])}")
    return xy, inf


class IpaUniversalParams:
    """`ipa_pc::UniversalParams` (PC::setup): comm_key of d + 1 generators for d = next_power_of_two(max_degree + 1) - 1, and h and s,
    the two `pop()`s of sample_generators(d + 3): h is generator d + 2 and s generator d + 1.  s (the hiding generator) is derived and
    carried; nothing here uses it.  The generators stay on the device; `trim` registers a prefix of them from there."""

    def __init__(self, curve, max_degree: int, generators, ctx: Context | None = None, digest: str = "blake2b"):
        """generators: the d + 3 points, as (xy, inf) device tensors (`setup`) or as a host list of (x, y) | None"""
        self.curve = get_curve(curve)
        self.ctx = ctx
        self.digest = digest
        self.max_degree = self.degree_bound(max_degree)
        d = self.max_degree
        self._gens = generators
        if self._on_host():
            if len(generators) != d + 3:
                raise ValueError("setup takes d + 3 generators")
            self.s, self.h = generators[d + 1], generators[d + 2]
        else:
            xy, inf = generators
            if xy.shape[0] != d + 3 or inf.shape[0] != d + 3:
                raise ValueError("setup takes d + 3 generators")
            tail_xy, tail_inf = xy[d + 1:].cpu().numpy().view(np.uint64), inf[d + 1:].cpu().numpy()
            self.s, self.h = (_pt_from_limbs(self.curve, tail_xy[k], tail_inf[k]) for k in range(2))

    def _on_host(self) -> bool:
        return isinstance(self._gens, list)

    @staticmethod
    def degree_bound(degree: int) -> int:
        """the degree a key is rounded up to: next_power_of_two(degree + 1) - 1"""
        return next_power_of_two(int(degree) + 1) - 1

    @classmethod
    def setup(cls, max_degree: int, curve="bls12_381", digest: str = "blake2b", ctx: Context | None = None) -> "IpaUniversalParams":
        ctx = ctx or default_context(0)
        d = cls.degree_bound(max_degree)
        return cls(curve, d, sample_generators(curve, d + 3, 0, digest, ctx), ctx, digest)

    @property
    def comm_key(self):
        """generators [0, d]: (xy, inf) views of the device tensors, or the host list"""
        d1 = self.max_degree + 1
        return self._gens[:d1] if self._on_host() else (self._gens[0][:d1], self._gens[1][:d1])

    def trim_size(self, supported_degree: int) -> int:
        """points of the key `trim` returns: next_power_of_two(supported_degree + 1); beyond max_degree + 1 is an error"""
        t = self.degree_bound(supported_degree)
        if t > self.max_degree:
            raise ValueError(f"trim: supported degree {supported_degree} rounds to {t}, beyond the setup's {self.max_degree}")
        return t + 1

    def trim(self, supported_degree: int) -> "IpaCommitterKey":
        """PC::trim: the key of comm_key[0 .. t + 1) with the same h (and s), registered from the device copy: no second derivation,
        and the points do not pass through host memory"""
        k = self.trim_size(supported_degree)
        if self._on_host():
            xy, inf = _pts_to_limbs(self.curve, self._gens[:k])
            key = CommitterKey(xy, self.curve, self.ctx, infinity=inf)
        else:
            key = CommitterKey(self._gens[0][:k], self.curve, self.ctx, infinity=self._gens[1][:k])
        ck = IpaCommitterKey(key, self.h, self.curve)
        ck.s = self.s
        return ck


# statuses of ipa_proof_parse
IPA_PROOF_OK, IPA_PROOF_TRUNCATED, IPA_PROOF_BAD_COUNT, IPA_PROOF_BAD_OPTION, IPA_PROOF_C_NOT_REDUCED = range(5)


def ipa_proof_bytes(proof: "IpaProof", curve) -> bytes:
    """`ipa_pc::Proof` as ark-serialize 0.3 derives it, AS RECALLED (ark-poly-commit 0.3; parity with the crate is unpinned, like the
    transcript's encodings above): l_vec and r_vec as a u64 count and compressed points each, final_comm_key compressed, c as 32 bytes
    little-endian, then hiding_comm and rand as one `None` byte (0) each.  The ONE place that holds this layout, with its inverse
    `ipa_proof_parse`; a `Proof<F, IPA>` is the KZG layout of proof.rs:41-103 with each kzg10::Proof replaced by these bytes."""
    out = bytearray()
    for vec in (proof.l_vec, proof.r_vec):
        out += len(vec).to_bytes(8, "little")
        for p in vec:
            out += g1_compress(curve, p)
    out += g1_compress(curve, proof.final_comm_key) + int(proof.c).to_bytes(32, "little") + b"\x00\x00"
    return bytes(out)


def ipa_proof_parse(data: bytes, curve, log_d: int, pos: int = 0):
    """The inverse of `ipa_proof_bytes` on bytes that are DATA: reads one proof of a key of 2^log_d points at data[pos:] and returns
    (status, fields, end).  fields: (l_vec encodings, r_vec encodings, final_comm_key encoding, c) -- the points stay compressed
    (whether they decode is the device's check: zk_g1_decompress_batch_dev) -- and end the offset behind the proof; both None unless
    status is IPA_PROOF_OK.  A count other than log_d, bytes that end inside a field, an option byte other than `None`, c >= r: a
    status, never an exception."""
    cv = get_curve(curve)
    g = 8 * cv.fq_limbs
    data = bytes(data)
    vecs = []
    for _ in range(2):
        if pos + 8 > len(data):
            return IPA_PROOF_TRUNCATED, None, None
        if int.from_bytes(data[pos:pos + 8], "little") != log_d:
            return IPA_PROOF_BAD_COUNT, None, None
        pos += 8
        if pos + log_d * g > len(data):
            return IPA_PROOF_TRUNCATED, None, None
        vecs.append([data[pos + k * g:pos + (k + 1) * g] for k in range(log_d)])
        pos += log_d * g
    if pos + g + 32 + 2 > len(data):
        return IPA_PROOF_TRUNCATED, None, None
    key = data[pos:pos + g]
    c = int.from_bytes(data[pos + g:pos + g + 32], "little")
    pos += g + 32
    if data[pos] != 0 or data[pos + 1] != 0:
        return IPA_PROOF_BAD_OPTION, None, None
    if c >= cv.r:
        return IPA_PROOF_C_NOT_REDUCED, None, None
    return IPA_PROOF_OK, (vecs[0], vecs[1], key, c), pos + 2


def check_poly_eval(curve, log_d: int, xis, z: int) -> int:
    """s(z) = prod_j (1 + xi_j z^(2^(log_d - 1 - j))): the last b of an opening at z."""
    r = get_curve(curve).r
    out = 1
    for j, x in enumerate(xis):
        out = out * (1 + x * pow(z, 1 << (log_d - 1 - j), r)) % r
    return out


@dataclass
class IpaProof:
    """ipa_pc::Proof without hiding: l_vec, r_vec, final_comm_key, c (hiding_comm = rand = None)."""
    l_vec: list = field(default_factory=list)
    r_vec: list = field(default_factory=list)
    final_comm_key: tuple | None = None
    c: int = 0


@dataclass
class IpaOpening:
    """The arguments of `IpaCommitterKey.check` as one record: an element of a batch (`batch_check`, `locate_invalid`)."""
    commitments: list
    point: int
    values: list
    proof: IpaProof
    opening_challenge: int


@dataclass
class _PreparedBatch:
    """What a batch's per-opening host work leaves for the range evaluations: opening j owns rows [row_off[j], row_off[j + 1]) of the
    proof-point MSM (none if it is malformed) and row j of the device challenges and weights (zeros if it is malformed)."""
    n: int
    malformed: list
    row_off: list
    pts_xy: np.ndarray          # (rows, 2L) Montgomery
    pts_inf: np.ndarray         # (rows,)
    scalars: np.ndarray         # (rows, 4) canonical
    h_scalars: list             # u_j xi_{j,0} (v_j - c_j s_j(z_j)) per opening, 0 for a malformed one
    d_xis: object               # (n, log_d, 4) Montgomery, device
    d_key_weights: object       # (n, 4) Montgomery, device: -u'_j


def batch_inverse(vals, r: int) -> list:
    """1 / v for every v (all non-zero mod r) with ONE modular inversion."""
    prefix, acc = [], 1
    for v in vals:
        prefix.append(acc)
        acc = acc * v % r
    inv = pow(acc, -1, r) if vals else 1
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * prefix[i] % r
        inv = inv * vals[i] % r
    return out


def _pt_from_limbs(curve, xy, inf) -> tuple | None:
    cv = get_curve(curve)
    if int(inf):
        return None
    L = cv.fq_limbs
    x, y = fq_from_mont(cv, np.asarray(xy, dtype=np.uint64).reshape(2, L))
    return (x, y)


def _pts_to_limbs(curve, pts):
    cv = get_curve(curve)
    L = cv.fq_limbs
    xy = np.zeros((len(pts), 2 * L), dtype=np.uint64)
    inf = np.zeros(len(pts), dtype=np.uint8)
    for i, p in enumerate(pts):
        if p is None:
            inf[i] = 1
        else:
            xy[i] = fq_to_mont(cv, [p[0], p[1]]).reshape(-1)
    return xy, inf


class IpaCommitterKey:
    """`ipa_pc::CommitterKey` without hiding: comm_key (d + 1 = 2^k affine G1 points, (n, 2L) Montgomery limbs as CommitterKey takes
    them) and h, on the device as a registered SRS (CommitterKey).  `IpaUniversalParams.setup(...).trim(...)` derives one by ipa_pc's
    PC-DL-2020 hash-to-curve, on the device; a caller may equally bring its own points.  A key whose points have KNOWN logarithms
    (k_i * G: what the tests and tools build where they need the integer reference verifier) is good for checking this library and
    for nothing else: whoever knows the k_i opens any commitment to any value."""

    def __init__(self, comm_key, h, curve="bls12_381", ctx: Context | None = None):
        self.curve = get_curve(curve)
        self.key = comm_key if isinstance(comm_key, CommitterKey) else CommitterKey(comm_key, self.curve, ctx)
        self.ctx = self.key.ctx
        self.d1 = self.key.n
        if self.d1 < 1 or self.d1 & (self.d1 - 1):
            raise ValueError("an IPA committer key holds 2^k points")
        self.log_d = self.d1.bit_length() - 1
        self.h = h

    def precompute(self, window_bits: int = 0):
        self.key.precompute(window_bits)
        return self

    def close(self):
        self.key.close()

    # -- device helpers
    def _torch(self):
        import torch
        return torch

    def _msm_host(self, pts, scalars):
        """affine(sum scalars[i] pts[i]) on the device (zk_msm_g1: ad-hoc bases)."""
        cv = self.curve
        xy, inf = _pts_to_limbs(cv, pts)
        sc = ints_to_limbs([s % cv.r for s in scalars], 4)
        out = np.zeros(2 * cv.fq_limbs, dtype=np.uint64)
        oinf = np.zeros(1, dtype=np.uint8)
        check(lib().zk_msm_g1(self.ctx.handle, cv.curve_id, ptr_of(xy), ptr_of(inf), ptr_of(sc), len(pts), ptr_of(out), ptr_of(oinf)),
              "zk_msm_g1")
        return _pt_from_limbs(cv, out, oinf[0])

    def commit(self, polys) -> list:
        """PC::commit without hiding: MSM(comm_key[0 .. len), coeffs.into_repr()) per polynomial (Montgomery coefficients, host arrays
        or device tensors), the SRS MSM over the registered key."""
        out = []
        for p in polys:
            g = self.key.commit(p)
            out.append(None if g.infinity else tuple(fq_from_mont(self.curve, np.stack([g.x, g.y]))))
        return out

    def _combine(self, polys, chi: int):
        """a = sum chi^k p_k (Montgomery, zero-padded to d + 1) on the device, and its evaluation-independent coefficients."""
        torch = self._torch()
        cv = self.curve
        dev = torch.device("cuda", self.ctx.device)
        tens = [p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p, dtype=np.uint64).view(np.int64)).to(dev)
                for p in polys]
        for t in tens:
            if t.shape[0] > self.d1:
                raise ValueError("polynomial longer than the committer key")
        k = len(tens)
        ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tens])
        lens = (ctypes.c_size_t * k)(*[t.shape[0] for t in tens])
        coeffs = fr_to_mont(cv, [pow(chi, i, cv.r) for i in range(k)])
        a = torch.zeros((self.d1, 4), dtype=torch.int64, device=dev)
        self.ctx.use_torch_stream()
        check(lib().zk_poly_lincomb_dev(self.ctx.handle, cv.curve_id, k, ptrs, lens, ptr_of(coeffs), a.data_ptr(), self.d1),
              "zk_poly_lincomb_dev")
        return a

    def open(self, polys, commitments, point: int, opening_challenge: int, digest: str = "blake2b", between_rounds=None) -> IpaProof:
        """PC::open of the polynomials (Montgomery coefficients) at `point` with opening challenge chi, no hiding, no degree bounds.
        between_rounds(j), if given, runs after round j's fold: the opening's state is in its own buffers, so other work may use the
        ctx there."""
        torch = self._torch()
        cv = self.curve
        r = cv.r
        L = cv.fq_limbs
        cid = cv.curve_id
        z = point % r
        a = self._combine(polys, opening_challenge)
        # v = p(z), C = affine(sum chi^k C_k)
        zm = fr_to_mont(cv, [z])
        vm = np.zeros(4, dtype=np.uint64)
        aptr = (ctypes.c_void_p * 1)(a.data_ptr())
        alen = (ctypes.c_size_t * 1)(self.d1)
        check(lib().zk_poly_evaluate_dev(self.ctx.handle, cid, 1, aptr, alen, ptr_of(zm), ptr_of(vm)), "zk_poly_evaluate_dev")
        v = fr_from_mont(cv, vm.reshape(1, 4))[0]
        C = self._msm_host(commitments, [pow(opening_challenge, i, r) for i in range(len(commitments))])
        xi = transcript_hash(cv, digest, [("g1", C), ("fr", z), ("fr", v)])
        h_prime = self._msm_host([self.h], [xi])
        proof = IpaProof()
        if self.d1 == 1:
            proof.final_comm_key = self._first_key()
            proof.c = fr_from_mont(cv, a.cpu().numpy().view(np.uint64).reshape(1, 4))[0]
            return proof
        b = torch.empty((self.d1, 4), dtype=torch.int64, device=a.device)
        check(lib().zk_ipa_powers_dev(self.ctx.handle, cid, ptr_of(zm), self.d1, b.data_ptr()), "zk_ipa_powers_dev")
        work = torch.empty(lib().zk_ipa_workspace_bytes(cid, self.d1), dtype=torch.uint8, device=a.device)
        hp_xy, _ = _pts_to_limbs(cv, [h_prime])
        out = np.zeros(4 * L, dtype=np.uint64)
        oinf = np.zeros(2, dtype=np.uint8)
        m, first = self.d1 // 2, 1
        while m >= 1:
            check(lib().zk_ipa_round_dev(self.ctx.handle, self.key._h, first, m, a.data_ptr(), b.data_ptr(), work.data_ptr(),
                                         ptr_of(hp_xy), ptr_of(out), ptr_of(oinf)), "zk_ipa_round_dev")
            Lp = _pt_from_limbs(cv, out[:2 * L], oinf[0])
            Rp = _pt_from_limbs(cv, out[2 * L:], oinf[1])
            proof.l_vec.append(Lp)
            proof.r_vec.append(Rp)
            xi = transcript_hash(cv, digest, [("fr", xi), ("g1", Lp), ("g1", Rp)])
            xm = fr_to_mont(cv, [xi])
            check(lib().zk_ipa_fold_dev(self.ctx.handle, self.key._h, first, m, ptr_of(xm), a.data_ptr(), b.data_ptr(), work.data_ptr()),
                  "zk_ipa_fold_dev")
            if between_rounds is not None:
                between_rounds(len(proof.l_vec) - 1)
            m //= 2
            first = 0
        fk = np.zeros(2 * L, dtype=np.uint64)
        finf = np.zeros(1, dtype=np.uint8)
        check(lib().zk_ipa_final_key_dev(self.ctx.handle, cid, work.data_ptr(), ptr_of(fk), ptr_of(finf)), "zk_ipa_final_key_dev")
        proof.final_comm_key = _pt_from_limbs(cv, fk, finf[0])
        proof.c = fr_from_mont(cv, a[:1].cpu().numpy().view(np.uint64).reshape(1, 4))[0]
        return proof

    def _first_key(self):
        """comm_key[0] (the final key of a one-point key) read back through a one-term MSM."""
        torch = self._torch()
        one = torch.from_numpy(ints_to_limbs([1], 4).view(np.int64)).cuda(self.ctx.device)
        g = self.key.msm(one)
        return None if g.infinity else tuple(fq_from_mont(self.curve, np.stack([g.x, g.y])))

    def final_key_msm(self, xis):
        """MSM(comm_key, s) with s_k the coefficients of the check polynomial (zk_ipa_check_coeffs_dev), over the registered key."""
        torch = self._torch()
        cv = self.curve
        s = torch.empty((self.d1, 4), dtype=torch.int64, device=torch.device("cuda", self.ctx.device))
        xm = fr_to_mont(cv, list(xis)) if len(xis) else np.zeros((1, 4), dtype=np.uint64)
        self.ctx.use_torch_stream()
        check(lib().zk_ipa_check_coeffs_dev(self.ctx.handle, cv.curve_id, len(xis), ptr_of(xm), s.data_ptr()), "zk_ipa_check_coeffs_dev")
        g = self.key.msm(s)
        return None if g.infinity else tuple(fq_from_mont(cv, np.stack([g.x, g.y])))

    def check(self, commitments, point: int, values, proof: IpaProof, opening_challenge: int, digest: str = "blake2b") -> bool:
        """PC::check of one opening: the succinct check and the final-key MSM, both on the device."""
        cv = self.curve
        r = cv.r
        if len(proof.l_vec) != self.log_d or len(proof.r_vec) != self.log_d:
            return False
        z = point % r
        C = self._msm_host(commitments, [pow(opening_challenge, i, r) for i in range(len(commitments))])
        v = sum(pow(opening_challenge, i, r) * int(x) for i, x in enumerate(values)) % r
        xi = transcript_hash(cv, digest, [("g1", C), ("fr", z), ("fr", v)])
        h_prime = self._msm_host([self.h], [xi])
        xis = []
        for Lp, Rp in zip(proof.l_vec, proof.r_vec):
            xi = transcript_hash(cv, digest, [("fr", xi), ("g1", Lp), ("g1", Rp)])
            xis.append(xi)
        pts = [C, h_prime] + list(proof.l_vec) + list(proof.r_vec)
        sc = [1, v] + [pow(x, -1, r) for x in xis] + xis
        lhs = self._msm_host(pts, sc)
        sz = check_poly_eval(cv, self.log_d, xis, z)
        rhs = self._msm_host([proof.final_comm_key, h_prime], [proof.c, proof.c * sz % r])
        if lhs != rhs:
            return False
        return self.final_key_msm(xis) == proof.final_comm_key

    # -- a batch of openings under one equation
    @staticmethod
    def random_weights(n_open: int) -> list:
        """128-bit non-zero weight pairs from the operating system's randomness: what the soundness of the batch rests on"""
        return [(secrets.randbits(128) or 1, secrets.randbits(128) or 1) for _ in range(n_open)]

    def _well_formed(self, o: IpaOpening) -> bool:
        """What a batch refuses before any arithmetic: l_vec / r_vec of another length than log_d, a number of values other than the
        number of commitments, c or a value that is not an integer below r, a coordinate that is not below q."""
        cv = self.curve
        pr = o.proof
        if len(pr.l_vec) != self.log_d or len(pr.r_vec) != self.log_d or len(o.values) != len(o.commitments):
            return False
        if not all(isinstance(x, int) and 0 <= x < cv.r for x in [pr.c] + list(o.values)):
            return False
        pts = list(o.commitments) + list(pr.l_vec) + list(pr.r_vec) + [pr.final_comm_key]
        return all(p is None or (0 <= p[0] < cv.q and 0 <= p[1] < cv.q) for p in pts)

    def _combined_commitments(self, openings) -> list:
        """C_j = sum_k chi_j^k C_{j,k} of every opening, as points, in ONE launch: a segment per opening over the batch's commitments
        (msm.segments_msm)."""
        torch = self._torch()
        cv = self.curve
        if not openings:
            return []
        pts, sc, off = [], [], [0]
        for o in openings:
            pts += list(o.commitments)
            sc += [pow(o.opening_challenge, i, cv.r) for i in range(len(o.commitments))]
            off.append(len(pts))
        dev = torch.device("cuda", self.ctx.device)
        xy, inf = _pts_to_limbs(cv, pts)
        out_xy, out_inf, st = segments_msm(torch.from_numpy(xy.view(np.int64)).to(dev), torch.from_numpy(inf).to(dev),
                                           torch.tensor(off, dtype=torch.int64, device=dev),
                                           torch.arange(len(pts), dtype=torch.int32, device=dev),
                                           torch.from_numpy(ints_to_limbs(sc, 4).view(np.int64)).to(dev).view(-1, 4), cv, self.ctx)
        if int(st.max()) != 0:
            raise RuntimeError("segments_msm: a segment of the batch's own layout was refused")
        out_xy, out_inf = out_xy.cpu().numpy().view(np.uint64), out_inf.cpu().numpy()
        return [_pt_from_limbs(cv, out_xy[j], out_inf[j]) for j in range(len(openings))]

    def _prepare(self, openings, weights, digest: str) -> _PreparedBatch:
        """The per-opening host work of a batch, done once: C_j (a point: it is hashed), v_j, the challenges through transcript_hash,
        their inverses with one inversion for the batch, s_j(z_j); then the rows of the proof-point MSM
            u_j C_j + (u'_j - u_j c_j) U_j + sum_k u_j (xi_{j,k}^-1 L_{j,k} + xi_{j,k} R_{j,k}),
        the scalar of h, and the challenges and key weights -u'_j on the device."""
        torch = self._torch()
        cv = self.curve
        r = cv.r
        B = len(openings)
        if weights is None:
            weights = self.random_weights(B)
        if len(weights) != B:
            raise ValueError("one pair of weights per opening")
        malformed, heads, xis_all = [], [None] * B, [[0] * self.log_d for _ in range(B)]
        formed = [j for j, o in enumerate(openings) if self._well_formed(o)]
        combined = dict(zip(formed, self._combined_commitments([openings[j] for j in formed])))
        for j, o in enumerate(openings):
            if j not in combined:
                malformed.append(j)
                continue
            chi, z = o.opening_challenge, o.point % r
            C = combined[j]
            v = sum(pow(chi, i, r) * x for i, x in enumerate(o.values)) % r
            xi0 = xi = transcript_hash(cv, digest, [("g1", C), ("fr", z), ("fr", v)])
            xis = []
            for Lp, Rp in zip(o.proof.l_vec, o.proof.r_vec):
                xi = transcript_hash(cv, digest, [("fr", xi), ("g1", Lp), ("g1", Rp)])
                xis.append(xi)
            if 0 in xis:                                   # a challenge with no inverse: nothing can be checked against it
                malformed.append(j)
                continue
            heads[j] = (C, v, xi0, z)
            xis_all[j] = xis
        inv = iter(batch_inverse([x for j in range(B) if heads[j] is not None for x in xis_all[j]], r))
        pts, sc, row_off, h_scalars, key_w = [], [], [0], [0] * B, [0] * B
        for j in range(B):
            if heads[j] is not None:
                C, v, xi0, z = heads[j]
                pr = openings[j].proof
                u, u2 = int(weights[j][0]) % r, int(weights[j][1]) % r
                xis = xis_all[j]
                pts += [C, pr.final_comm_key] + list(pr.l_vec) + list(pr.r_vec)
                sc += [u, (u2 - u * pr.c) % r] + [u * next(inv) % r for _ in xis] + [u * x % r for x in xis]
                h_scalars[j] = u * xi0 % r * (v - pr.c * check_poly_eval(cv, self.log_d, xis, z)) % r
                key_w[j] = -u2 % r
            row_off.append(len(pts))
        xy, inf = _pts_to_limbs(cv, pts)
        dev = torch.device("cuda", self.ctx.device)
        flat = [x for xs in xis_all for x in xs]
        d_xis = torch.from_numpy(fr_to_mont(cv, flat).view(np.int64)).to(dev) if flat else torch.zeros((0, 4), dtype=torch.int64, device=dev)
        d_w = torch.from_numpy(fr_to_mont(cv, key_w).view(np.int64)).to(dev) if B else torch.zeros((0, 4), dtype=torch.int64, device=dev)
        return _PreparedBatch(B, malformed, row_off, xy, inf, ints_to_limbs(sc, 4), h_scalars, d_xis.view(B, self.log_d, 4), d_w)

    def _combine_dev(self, prep: _PreparedBatch, lo: int, hi: int):
        """t = -sum_{lo <= j < hi} u'_j s_j: the canonical scalars of the range's ONE key MSM (zk_ipa_check_combine_dev)"""
        torch = self._torch()
        cid = self.curve.curve_id
        dev = torch.device("cuda", self.ctx.device)
        t = torch.empty((self.d1, 4), dtype=torch.int64, device=dev)
        work = torch.empty(max(lib().zk_ipa_check_combine_workspace_bytes(cid, self.log_d, hi - lo), 1), dtype=torch.uint8, device=dev)
        self.ctx.use_torch_stream()
        check(lib().zk_ipa_check_combine_dev(self.ctx.handle, cid, self.log_d, hi - lo, prep.d_xis[lo:].data_ptr(),
                                             prep.d_key_weights[lo:].data_ptr(), work.data_ptr(), t.data_ptr()), "zk_ipa_check_combine_dev")
        return t

    def _proof_points_partial(self, prep: _PreparedBatch, lo: int, hi: int) -> np.ndarray:
        """The range's terms over the proofs' points and h as ONE zk_msm_g1, as a Jacobian partial (3L limbs, Z = 0 for infinity)"""
        cv = self.curve
        L = cv.fq_limbs
        a, b = prep.row_off[lo], prep.row_off[hi]
        h_xy, h_inf = _pts_to_limbs(cv, [self.h])
        xy = np.concatenate([prep.pts_xy[a:b], h_xy])
        inf = np.concatenate([prep.pts_inf[a:b], h_inf])
        sc = np.concatenate([prep.scalars[a:b], ints_to_limbs([sum(prep.h_scalars[lo:hi]) % cv.r], 4)])
        out = np.zeros(3 * L, dtype=np.uint64)
        oinf = np.zeros(1, dtype=np.uint8)
        check(lib().zk_msm_g1(self.ctx.handle, cv.curve_id, ptr_of(xy), ptr_of(inf), ptr_of(sc), xy.shape[0], ptr_of(out), ptr_of(oinf)),
              "zk_msm_g1")
        if oinf[0]:
            out[:] = 0
        else:
            out[2 * L:] = fq_to_mont(cv, [1]).reshape(-1)
        return out

    def _batch_equation(self, prep: _PreparedBatch, lo: int, hi: int) -> bool:
        """The batch equation over the well-formed openings of [lo, hi):
            sum_j u_j [C_j + sum_k (xi_{j,k}^-1 L_{j,k} + xi_{j,k} R_{j,k}) - c_j U_j] + (sum_j u_j xi_{j,0} (v_j - c_j s_j(z_j))) h
              + sum_j u'_j U_j - MSM(comm_key, sum_j u'_j s_j) = O
        as two MSMs (the proofs' points; the registered key under the combined check vector) whose partial sums are added."""
        if lo == hi:
            return True
        parts = np.stack([self._proof_points_partial(prep, lo, hi), self.key.msm_partial(self._combine_dev(prep, lo, hi))])
        return sum_partials(parts, self.curve).infinity

    def batch_check(self, openings, weights=None, digest: str = "blake2b") -> bool:
        """PC::batch_check: True iff every opening would pass `check` (up to a soundness error of about 2^-128 under weights the
        provers cannot predict).  The key is read by ONE MSM for the batch.  weights: one pair (u, u') per opening -- for tests; None
        draws them from the operating system.  u weighs an opening's succinct check, u' its final-key check: under one shared weight
        an error in the first could cancel one in the second.  A malformed opening (vector lengths, a value not below r) makes the
        result False and takes no part in the sums."""
        openings = list(openings)
        prep = self._prepare(openings, weights, digest)
        if prep.malformed:
            return False
        return self._batch_equation(prep, 0, prep.n)

    def locate_invalid(self, openings, digest: str = "blake2b") -> list:
        """Indices of the openings that do not verify: the malformed ones, and those a bisection with the batch equation over ranges
        finds (a range whose left half passes needs no check of its right half).  The per-opening host work is done once; a range costs
        the combine and the two MSMs, at most 1 + 2 k ceil(log2 B) times for k failing openings."""
        openings = list(openings)
        prep = self._prepare(openings, None, digest)
        bad = set(prep.malformed)

        def ok(lo, hi):
            return self._batch_equation(prep, lo, hi)

        def search(lo, hi):                      # [lo, hi) is known to fail
            if hi - lo == 1:
                bad.add(lo)
                return
            mid = (lo + hi) // 2
            if ok(lo, mid):
                search(mid, hi)
                return
            search(lo, mid)
            if not ok(mid, hi):
                search(mid, hi)

        if prep.n and not ok(0, prep.n):
            search(0, prep.n)
        return sorted(bad)
