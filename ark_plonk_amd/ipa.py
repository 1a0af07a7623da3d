"""Inner-product-argument polynomial commitment: ark-poly-commit 0.3 `ipa_pc::InnerProductArgPC`, the reference's second
`HomomorphicCommitment` (plonk-core/src/commitment.rs:50-91), without hiding and degree bounds -- what ark-plonk uses
(prover.rs:582-618 passes no rng and no degree bounds).

    ck = IpaCommitterKey(comm_key, h, "bls12_381")      # d + 1 = 2^k points (PC::trim rounds up: d + 1 = 2n for a circuit of n)
    comms = ck.commit(polys)
    proof = ck.open(polys, comms, z, chi, digest="blake2b")
    assert ck.check(comms, z, values, proof, chi, digest="blake2b")

Every group operation and every O(n) vector pass runs in libark_plonk_amd.so: commit and the verifier's final-key MSM are the SRS
MSM over the registered key, the opening's rounds are zk_ipa_round_dev / zk_ipa_fold_dev (include/ark_plonk_amd.h).  The device
never hashes: every challenge is derived here, by `transcript_hash`, the ONE place that holds the byte encodings of the
Fiat-Shamir transcript.  Parity with the Rust crate is unpinned (its source is not vendored): that function states what it assumes.

Points cross this module as Python tuples (x, y) of canonical base-field integers, None for the point at infinity; field
elements as canonical integers.
"""
from __future__ import annotations

import ctypes
import hashlib
from dataclasses import dataclass, field

import numpy as np

from ._lib import check, lib
from .context import Context, ptr_of
from .curves import fq_from_mont, fq_to_mont, fr_from_mont, fr_to_mont, get_curve, ints_to_limbs
from .msm import CommitterKey

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
    them) and h, on the device as a registered SRS (CommitterKey).  Key generation (PC-DL-2020 hash-to-curve) is the caller's."""

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
