"""The KZG pairing check e(L, [tau]H) e(-R, H) = 1: csrc/pairing.hip behind `PairingKey`.

`ark_ec::PairingEngine::product_of_pairings` as `kzg10::KZG10::check` calls it.  Both G2 points belong to the verifier key, so a
`PairingKey` validates them and prepares their Miller-loop line tables once, on the host; after that

  * `check(L, R)` is ONE check on the host (milliseconds; no context, no GPU): the form for a fold of a whole batch and for each step
    of a bisection (`BatchVerifier.verify`, `BatchVerifier.locate_invalid`);
  * `check_batch(...)` is B independent checks in one launch, one per lane: per-proof verdicts (`BatchVerifier.verdicts`).

`gt` / `gt_batch` return the GT value itself, e(P, Q)^c with the curve's constant `GT_POWER[curve]` (3 on BLS12-381, 1 on BN254): what
the tests compare with an independent definition of the pairing.

Field elements are uint64 Montgomery limbs, as everywhere in this package; a G2 coordinate is an Fq2 value (c0, c1), Fq2 = Fq[u]/(u^2 + 1).
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import check, lib
from .context import Context, default_context, ptr_of
from .curves import fq_to_mont, g2_mul, get_curve
from .msm import G1Affine

# gt() returns e(P, Q)^GT_POWER for the reduced pairing e with the exponent (q^12 - 1) / r (ZK_PAIRING_GT_POWER_* in csrc/pairing.cuh)
GT_POWER = {"bls12_381": 3, "bn254": 1}


class G2Affine:
    """A point of the twist: x and y as (2, L) uint64 Montgomery limbs, (c0, c1) each.  No infinity: a verifier key has none."""

    __slots__ = ("x", "y", "curve")

    def __init__(self, x, y, curve="bls12_381"):
        cv = get_curve(curve)
        self.x = np.ascontiguousarray(x, dtype=np.uint64).reshape(2, cv.fq_limbs).copy()
        self.y = np.ascontiguousarray(y, dtype=np.uint64).reshape(2, cv.fq_limbs).copy()
        self.curve = cv.name

    @classmethod
    def from_ints(cls, x, y, curve="bls12_381"):
        """x = (x0, x1), y = (y0, y1): canonical integers"""
        cv = get_curve(curve)
        return cls(fq_to_mont(cv, x), fq_to_mont(cv, y), cv)

    def limbs(self) -> np.ndarray:
        """x.c0 x.c1 y.c0 y.c1, L limbs each: the layout of zk_pairing_key_new"""
        return np.concatenate([self.x.reshape(-1), self.y.reshape(-1)])

    def __eq__(self, o):
        return isinstance(o, G2Affine) and self.curve == o.curve and np.array_equal(self.x, o.x) and np.array_equal(self.y, o.y)


def _g1_args(p, cv):
    """a G1Affine, or None for infinity -> (2L limbs, flag)"""
    if p is None:
        return np.zeros(2 * cv.fq_limbs, dtype=np.uint64), 1
    return np.ascontiguousarray(p.xy(), dtype=np.uint64).reshape(-1), 1 if p.infinity else 0


class PairingKey:
    """The G2 side of a KZG verifier key, prepared: h = H and tau_h = [tau]H as `G2Affine`.

    Raises `ZkError` (ZK_ERR_BAD_ARG) for a point with an unreduced coordinate, off the twist, or outside the r-torsion."""

    def __init__(self, h: G2Affine, tau_h: G2Affine, curve="bls12_381"):
        self.curve = cv = get_curve(curve)
        self._h = None
        handle = ctypes.c_void_p()
        a, b = np.ascontiguousarray(h.limbs()), np.ascontiguousarray(tau_h.limbs())
        check(lib().zk_pairing_key_new(cv.curve_id, ptr_of(a), ptr_of(b), ctypes.byref(handle)), "zk_pairing_key_new")
        self._h = handle

    @classmethod
    def from_trapdoor(cls, tau: int, curve="bls12_381"):
        """The key of the SRS whose trapdoor is `tau`: (H, [tau]H) for the standard generator H.  For tests, tools and examples only:
        whoever knows tau can forge openings, so a real key's G2 points come from the ceremony that made its SRS."""
        cv = get_curve(curve)
        return cls(G2Affine.from_ints(cv.g2x, cv.g2y, cv), G2Affine.from_ints(*g2_mul(cv, tau), cv), cv)

    def close(self):
        if self._h is not None:
            lib().zk_pairing_key_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise RuntimeError("the pairing key is closed")
        return self._h

    def check(self, L: G1Affine, R: G1Affine) -> bool:
        """e(L, [tau]H) e(-R, H) == 1, on the host.  Raises `ZkError` (ZK_ERR_BAD_ARG) for a point that is not flagged as infinity
        and has a coordinate that is not below q: the verdict would depend on the representation of R.y."""
        cv = self.curve
        (l, li), (r, ri) = _g1_args(L, cv), _g1_args(R, cv)
        ok = ctypes.c_int(0)
        check(lib().zk_kzg_pairing_check(self._handle(), ptr_of(l), li, ptr_of(r), ri, ctypes.byref(ok)), "zk_kzg_pairing_check")
        return bool(ok.value)

    def gt(self, P: G1Affine, which: int) -> np.ndarray:
        """e(P, which ? [tau]H : H)^GT_POWER as (12, L) uint64 Montgomery limbs in tower order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ...).
        An unreduced coordinate is a `ZkError`, as in `check`."""
        cv = self.curve
        p, pi = _g1_args(P, cv)
        out = np.zeros((12, cv.fq_limbs), dtype=np.uint64)
        check(lib().zk_pairing_gt(self._handle(), int(which), ptr_of(p), pi, ptr_of(out)), "zk_pairing_gt")
        return out

    def _dev_points(self, xy, inf, ctx, what):
        import torch
        L2 = 2 * self.curve.fq_limbs
        if not torch.is_tensor(xy) or not xy.is_cuda or xy.device.index != ctx.device or xy.dtype != torch.int64 or not xy.is_contiguous() \
                or xy.numel() % L2:
            raise ValueError(f"{what}: expected a contiguous int64 tensor of (n, {L2}) limbs on device {ctx.device}")
        n = xy.numel() // L2
        if inf is not None and (not torch.is_tensor(inf) or not inf.is_cuda or inf.device.index != ctx.device or inf.dtype != torch.uint8
                                or not inf.is_contiguous() or inf.numel() != n):
            raise ValueError(f"{what}: expected {n} contiguous uint8 infinity flags on device {ctx.device}")
        return n

    def check_batch(self, d_L, d_L_inf, d_R, d_R_inf, ctx: Context | None = None):
        """n checks in one launch: d_L, d_R (n, 2L) int64 device tensors (Montgomery affine), d_L_inf, d_R_inf (n,) uint8 or None.
        Returns the (n,) uint8 device tensor of verdicts; queued on the current torch stream, nothing is waited for.  The coordinates
        are the library's own device outputs, reduced; the kernels do not look (unreduced input is outside the contract here)."""
        import torch
        ctx = ctx or default_context(d_L.device.index)
        n = self._dev_points(d_L, d_L_inf, ctx, "d_L")
        if self._dev_points(d_R, d_R_inf, ctx, "d_R") != n:
            raise ValueError("as many R as L")
        ok = torch.empty((n,), dtype=torch.uint8, device=d_L.device)
        ctx.use_torch_stream()
        check(lib().zk_kzg_pairing_check_batch_dev(ctx.handle, self._handle(), ptr_of(d_L), None if d_L_inf is None else ptr_of(d_L_inf),
                                                   ptr_of(d_R), None if d_R_inf is None else ptr_of(d_R_inf), n, ptr_of(ok)),
              "zk_kzg_pairing_check_batch_dev")
        return ok

    def gt_batch(self, d_P, d_inf, which: int, ctx: Context | None = None):
        """`gt` of n points in one launch: d_P (n, 2L) int64, d_inf (n,) uint8 or None -> (n, 12, L) int64 device tensor; queued."""
        import torch
        ctx = ctx or default_context(d_P.device.index)
        n = self._dev_points(d_P, d_inf, ctx, "d_P")
        out = torch.empty((n, 12, self.curve.fq_limbs), dtype=torch.int64, device=d_P.device)
        ctx.use_torch_stream()
        check(lib().zk_pairing_gt_batch_dev(ctx.handle, self._handle(), int(which), ptr_of(d_P), None if d_inf is None else ptr_of(d_inf), n,
                                            ptr_of(out)), "zk_pairing_gt_batch_dev")
        return out
