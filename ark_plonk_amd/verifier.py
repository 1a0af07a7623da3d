"""Batch verification of proofs of one circuit: the two pairing inputs and the pairing check (section 6i).

`Proof::verify` (proof_system/proof.rs:110-425) ends in two KZG checks, e(C - v G, H) = e(W, tau H - z H) each.  Everything in front of
them is G1 and Fr arithmetic, and with unpredictable weights it folds across proofs: B proofs of one verifier key go in, TWO points
come out,

    L = sum_j (u_j W_aw,j + u'_j W_saw,j)
    R = sum_j (u_j (sum_k chi^k (C_k - v_k G) + z W_aw) + u'_j (sum_k chi'^k (C'_k - v'_k G) + z w W_saw))_j

and every proof of the batch is valid iff e(L, [tau]H) = e(R, H), except with probability about 2^-128 over the weights.  That check
is `pairing.PairingKey` (the G2 side of the verifier key, prepared once): given one, `BatchVerifier.verify` answers yes or no with
one check on the host, `locate_invalid` bisects with it, and `verdicts` gives every proof its own answer with no bisection -- every
(L_j, R_j) from one segmented MSM, then one launch of B checks, one per lane.  Stages, each one entry point of the C ABI:

  1  zk_g1_decompress_batch_dev   the 15 points of every proof decoded and checked on the device (one lane per point)
  2  zk_proof_replay_batch        host, serial: bytes parsed, the transcript replayed -> 14 challenges and 23 evaluations per proof
     zk_proof_replay_batch_dev    the same parse and replay on the device, one proof per lane, the rows and the 15 point encodings
                                  left where stages 1 and 3 read them (csrc/replay.hip; the walk is ONE piece of code for both)
  3  zk_verify_scalars_dev        per proof: 20 scalars over the verifier key's bases and G, 15 over its own points, 2 for L
  4  zk_fr_column_sum_dev + the existing MSM over the decoded points (zk_srs_register_dev, zk_msm_g1_srs_partial_dev,
     zk_g1_sum_partials), over any range [lo, hi) of the batch: the per-proof rows stay resident, another range costs only this stage
  5  zk_kzg_pairing_check         host: e(L, [tau]H) e(-R, H) = 1 for one fold
     zk_msm_g1_segments_dev + zk_kzg_pairing_check_batch_dev   per-proof (L_j, R_j) and their B checks, one per lane

`BatchVerifier(replay=...)` chooses stage 2: "host" decodes the points (1) while the host replays (2); "device" makes one upload and
queues 2, 1, 3 behind it with no host synchronisation before the statuses come back; "auto" takes the device from
REPLAY_ON_DEVICE_FROM proofs.  The two give bit-identical rows, statuses and (L, R).

Field elements are 4 x uint64 Montgomery limbs and points `G1Affine`, as everywhere in this package.
"""
from __future__ import annotations

import ctypes
import secrets

import numpy as np

from ._lib import check, lib
from .context import Context, default_context, ptr_of
from .curves import fq_from_mont, fq_to_mont, fr_from_mont, get_curve, ints_to_limbs, limbs_to_ints
from .ipa import IPA_PROOF_OK, IPA_PROOF_TRUNCATED, IpaOpening, IpaProof, ipa_proof_parse
from .msm import CommitterKey, G1Affine, segments_msm, sum_partials

N_CHALLENGES, N_EVALS, N_KEY_BASES, N_PROOF_BASES = 14, 23, 20, 15
CHALLENGES = ("zeta", "beta", "gamma", "delta", "epsilon", "alpha", "range", "logic", "fixed", "var", "lookup", "z", "aw", "saw")
# the evaluation row: the proof's 16 in its own order (transcript.PROOF_EVAL_FIELDS), then the seven custom ones the verifier reads
EVALS = ("a_eval", "b_eval", "c_eval", "d_eval", "left_sigma_eval", "right_sigma_eval", "out_sigma_eval", "permutation_eval",
         "q_lookup_eval", "z2_next_eval", "h1_eval", "h1_next_eval", "h2_eval", "f_eval", "table_eval", "table_next_eval",
         "a_next_eval", "b_next_eval", "d_next_eval", "q_arith_eval", "q_c_eval", "q_l_eval", "q_r_eval")
# the verifier key's commitments behind the key-base row (names of ProverKey.verifier_key); the 20th base is the generator G
KEY_BASES = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add", "q_lookup",
             "left_sigma", "right_sigma", "out_sigma", "fourth_sigma", "table_1", "table_2", "table_3", "table_4")
# the proof-base row: the commitments in the proof's order (transcript.PROOF_COMMITMENTS), then the two openings
PROOF_BASES = ("a_comm", "b_comm", "c_comm", "d_comm", "z_comm", "f_comm", "h_1_comm", "h_2_comm", "z_2_comm", "t_1_comm", "t_2_comm",
               "t_3_comm", "t_4_comm", "aw_opening", "saw_opening")

# stage 1 (per point), stage 2 (per proof), and the per-proof status stage 3 leaves
G1_OK, G1_BAD_FLAGS, G1_X_NOT_REDUCED, G1_NOT_ON_CURVE, G1_NOT_IN_SUBGROUP = range(5)
(PROOF_OK, PROOF_TRUNCATED, PROOF_TRAILING, PROOF_BAD_OPTION, PROOF_FR_NOT_REDUCED, PROOF_MISSING_LABEL, PROOF_BAD_COUNT,
 PROOF_BAD_PUBLIC_INPUTS) = range(8)
VERIFY_OK, VERIFY_BAD_POINT, VERIFY_Z_ON_DOMAIN = 0, 16, 32
# BatchVerifier(replay="auto"): batches of at least this many proofs replay on the device.  The smallest B of the grid
# {1, 8, 16, 32, 64, 128, 256, 1024, 4096} from which the device path's whole fold stays below the host path's
# (profiles/verify/notes.md, the table of tools/verify_bench.py --replay host device); None: the device path never won
REPLAY_ON_DEVICE_FROM = 1024


def _torch():
    import torch
    return torch


def decompress_batch(encodings, curve="bls12_381", ctx: Context | None = None):
    """Stage 1.  encodings: n compressed G1 points as bytes / a (n, g) uint8 array or device tensor.  Returns device tensors
    (points (n, 2L) int64 Montgomery affine, infinity flags (n,) uint8, status (n,) uint8 of G1_*); queued, not waited for."""
    torch = _torch()
    cv = get_curve(curve)
    g = lib().zk_g1_compressed_size(cv.curve_id)
    ctx = ctx or default_context(0)
    if isinstance(encodings, (bytes, bytearray)):
        encodings = np.frombuffer(bytes(encodings), dtype=np.uint8)
    if not torch.is_tensor(encodings):
        encodings = torch.from_numpy(np.array(encodings, dtype=np.uint8))        # a copy: the caller's buffer may be read-only
    dev = torch.device("cuda", ctx.device)
    d_in = encodings.to(dev).contiguous().view(-1)
    if d_in.dtype != torch.uint8 or d_in.numel() % g:
        raise ValueError(f"expected uint8 encodings of {g} bytes each")
    n = d_in.numel() // g
    pts = torch.empty((n, 2 * cv.fq_limbs), dtype=torch.int64, device=dev)
    inf = torch.empty((n,), dtype=torch.uint8, device=dev)
    st = torch.empty((n,), dtype=torch.uint8, device=dev)
    ctx.use_torch_stream()
    check(lib().zk_g1_decompress_batch_dev(ctx.handle, cv.curve_id, ptr_of(d_in), n, ptr_of(pts), ptr_of(inf), ptr_of(st)),
          "zk_g1_decompress_batch_dev")
    return pts, inf, st


def _flatten_public_inputs(public_inputs, n_proofs):
    """[{position: 4 Montgomery limbs}] -> (offsets (B + 1,), positions, values (m, 4)), positions ascending inside a proof"""
    if public_inputs is None:
        public_inputs = [{}] * n_proofs
    if len(public_inputs) != n_proofs:
        raise ValueError("one public-input map per proof")
    off = np.zeros(n_proofs + 1, dtype=np.uint64)
    pos, vals = [], []
    for j, pi in enumerate(public_inputs):
        for k in sorted(pi):
            pos.append(int(k))
            vals.append(np.asarray(pi[k], dtype=np.uint64).reshape(4))
        off[j + 1] = len(pos)
    p = np.array(pos, dtype=np.uint64) if pos else np.zeros(1, dtype=np.uint64)
    v = np.ascontiguousarray(np.stack(vals), dtype=np.uint64) if vals else np.zeros((1, 4), dtype=np.uint64)
    return off, p, v


def replay_batch(seeded, proofs, public_inputs=None, curve="bls12_381", with_points=False):
    """Stage 2 (host).  seeded: the `transcript.Transcript` after the verifier key was seeded into it (left untouched); proofs: B byte
    strings; public_inputs: B maps {position: 4 Montgomery limbs}.  Returns (challenges (B, 14, 4), evaluations (B, 23, 4), status (B,)
    of PROOF_*) -- rows in the order of CHALLENGES / EVALS, Montgomery -- and with with_points the (B, 15, g) uint8 encodings too."""
    cv = get_curve(curve)
    B = len(proofs)
    g = lib().zk_g1_compressed_size(cv.curve_id)
    off, pos, vals = _flatten_public_inputs(public_inputs, B)
    bufs = [bytes(p) for p in proofs]
    ptrs = (ctypes.c_char_p * max(B, 1))(*bufs)
    lens = (ctypes.c_size_t * max(B, 1))(*[len(b) for b in bufs])
    ch = np.zeros((B, N_CHALLENGES, 4), dtype=np.uint64)
    ev = np.zeros((B, N_EVALS, 4), dtype=np.uint64)
    st = np.zeros(max(B, 1), dtype=np.uint8)
    pts = np.zeros((B, N_PROOF_BASES, g), dtype=np.uint8) if with_points else None
    check(lib().zk_proof_replay_batch(seeded._h, cv.curve_id, B, ptrs, lens, ptr_of(off), ptr_of(pos), ptr_of(vals), ptr_of(ch), ptr_of(ev),
                                      None if pts is None else ptr_of(pts), ptr_of(st)), "zk_proof_replay_batch")
    return (ch, ev, st[:B], pts) if with_points else (ch, ev, st[:B])


def _replay_dev(seeded, B, d_blob, n_bytes, d_poff, d_pioff, d_pos, d_vals, n_pi_total, cv, ctx):
    """zk_proof_replay_batch_dev over arrays already on the device -> (challenges, evals, points, status), queued"""
    torch = _torch()
    dev = d_blob.device
    g = lib().zk_g1_compressed_size(cv.curve_id)
    ch = torch.empty((B, N_CHALLENGES, 4), dtype=torch.int64, device=dev)
    ev = torch.empty((B, N_EVALS, 4), dtype=torch.int64, device=dev)
    pts = torch.empty((B, N_PROOF_BASES, g), dtype=torch.uint8, device=dev)
    st = torch.empty((B,), dtype=torch.uint8, device=dev)
    ctx.use_torch_stream()
    check(lib().zk_proof_replay_batch_dev(ctx.handle, seeded._h, cv.curve_id, B, ptr_of(d_blob), n_bytes, ptr_of(d_poff), ptr_of(d_pioff),
                                          ptr_of(d_pos), ptr_of(d_vals), n_pi_total, ptr_of(ch), ptr_of(ev), ptr_of(pts), ptr_of(st)),
          "zk_proof_replay_batch_dev")
    return ch, ev, pts, st


def _upload_batch(proofs, public_inputs, extra, dev):
    """The inputs of a batch in ONE host buffer and one copy: the uint64 arrays first (proof offsets, public-input offsets, positions,
    values, then `extra`), the proofs' bytes joined behind them.  Returns the device views and (bytes of proofs, public inputs)."""
    torch = _torch()
    B = len(proofs)
    off, pos, vals = _flatten_public_inputs(public_inputs, B)
    blob = b"".join(bytes(p) for p in proofs)
    poff = np.zeros(B + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in proofs], out=poff[1:])
    words = [poff, off, pos.reshape(-1), vals.reshape(-1)] + [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in extra]
    starts, at = [], 0
    for w in words:                                    # every array starts on 16 bytes: the kernels read field elements as 128-bit words
        starts.append(at)
        at += w.size + (w.size & 1)
    host = np.zeros(8 * at + max(len(blob), 1), dtype=np.uint8)
    head = host[:8 * at].view(np.uint64)
    for w, o in zip(words, starts):
        head[o:o + w.size] = w
    host[8 * at:8 * at + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    d = torch.from_numpy(host).to(dev)
    d_words = d[:8 * at].view(torch.int64)
    return [d_words[o:o + w.size] for w, o in zip(words, starts)], d[8 * at:], len(blob), int(off[B])


def replay_batch_dev(seeded, proofs, public_inputs=None, curve="bls12_381", ctx: Context | None = None):
    """Stage 2 on the device.  Arguments as `replay_batch`; the byte strings go up joined, with an offsets array, beside the flattened
    public inputs.  Returns device tensors (challenges (B, 14, 4) int64, evaluations (B, 23, 4) int64, points (B, 15, g) uint8, status
    (B,) uint8) with exactly the content `replay_batch(..., with_points=True)` returns; queued, not waited for."""
    torch = _torch()
    cv = get_curve(curve)
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    B = len(proofs)
    if B == 0:
        g = lib().zk_g1_compressed_size(cv.curve_id)
        return (torch.empty((0, N_CHALLENGES, 4), dtype=torch.int64, device=dev), torch.empty((0, N_EVALS, 4), dtype=torch.int64, device=dev),
                torch.empty((0, N_PROOF_BASES, g), dtype=torch.uint8, device=dev), torch.empty((0,), dtype=torch.uint8, device=dev))
    (d_poff, d_pioff, d_pos, d_vals), d_blob, n_bytes, n_pi = _upload_batch(proofs, public_inputs, [], dev)
    return _replay_dev(seeded, B, d_blob, n_bytes, d_poff, d_pioff, d_pos, d_vals, n_pi, cv, ctx)


def proof_point_bytes(proofs, curve="bls12_381") -> np.ndarray:
    """The 15 compressed points of every proof, (B, 15, g) uint8, by their fixed offsets (proof.rs:41-103: 13 commitments, then two
    openings followed by an Option byte each) -- no parsing, so stage 1 can start before stage 2.  A proof too short to hold them gets
    infinity encodings: stage 2 reports it."""
    cv = get_curve(curve)
    g = lib().zk_g1_compressed_size(cv.curve_id)
    out = np.zeros((len(proofs), N_PROOF_BASES, g), dtype=np.uint8)
    for j, p in enumerate(proofs):
        if len(p) < 15 * g + 2:
            out[j, :, g - 1] = 0x40
            continue
        a = np.frombuffer(bytes(p[:15 * g + 2]), dtype=np.uint8)
        out[j, :14] = a[:14 * g].reshape(14, g)
        out[j, 14] = a[14 * g + 1:15 * g + 1]
    return out


def scalar_rows(log_n, challenges, evals, public_inputs, coeff_a, coeff_d, weights, parse_status=None, point_status=None,
                curve="bls12_381", ctx: Context | None = None):
    """Stage 3.  challenges / evals: stage 2's rows (host arrays or device tensors); weights: B pairs (u, u') of integers;
    parse_status (B,), point_status (B * 15,): uint8, host or device, or None.  Returns device tensors (key rows (B, 20, 4), proof rows
    (B, 15, 4), opening rows (B, 2, 4) -- canonical scalars, int64 -- and status (B,) uint8); queued, not waited for."""
    torch = _torch()
    cv = get_curve(curve)
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)

    def up(x, dtype=None):
        if x is None:
            return None
        if not torch.is_tensor(x):
            a = np.ascontiguousarray(x)
            x = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a)
        return x.to(dev).contiguous()

    d_ch, d_ev = up(challenges), up(evals)
    B = d_ch.numel() // (4 * N_CHALLENGES)
    if d_ev.numel() != B * 4 * N_EVALS or len(weights) != B:
        raise ValueError("challenge rows, evaluation rows and weights must describe the same number of proofs")
    off, pos, vals = _flatten_public_inputs(public_inputs, B)
    d_off, d_pos, d_vals = up(off), up(pos), up(vals)
    w = ints_to_limbs([int(x) % cv.r for pair in weights for x in pair], 4) if B else np.zeros((1, 4), dtype=np.uint64)
    d_w = up(w)
    d_ps, d_pts = up(parse_status), up(point_status)
    return _scalars_dev(log_n, B, d_ch, d_ev, d_off, d_pos, d_vals, coeff_a, coeff_d, d_w, d_ps, d_pts, cv, ctx)


def _scalars_dev(log_n, B, d_ch, d_ev, d_off, d_pos, d_vals, coeff_a, coeff_d, d_w, d_ps, d_pts, cv, ctx):
    """zk_verify_scalars_dev over arrays already on the device (coeff_a, coeff_d: host, 4 limbs) -> (key, proof, opening rows, status)"""
    torch = _torch()
    dev = d_ch.device
    key = torch.empty((B, N_KEY_BASES, 4), dtype=torch.int64, device=dev)
    prf = torch.empty((B, N_PROOF_BASES, 4), dtype=torch.int64, device=dev)
    opn = torch.empty((B, 2, 4), dtype=torch.int64, device=dev)
    st = torch.empty((B,), dtype=torch.uint8, device=dev)
    ca = np.ascontiguousarray(coeff_a, dtype=np.uint64).reshape(4)
    cd = np.ascontiguousarray(coeff_d, dtype=np.uint64).reshape(4)
    ctx.use_torch_stream()
    check(lib().zk_verify_scalars_dev(ctx.handle, cv.curve_id, int(log_n), B, ptr_of(d_ch), ptr_of(d_ev), ptr_of(d_off), ptr_of(d_pos), ptr_of(d_vals),
                                      ptr_of(ca), ptr_of(cd), ptr_of(d_w), None if d_ps is None else ptr_of(d_ps),
                                      None if d_pts is None else ptr_of(d_pts), ptr_of(key), ptr_of(prf), ptr_of(opn), ptr_of(st)),
          "zk_verify_scalars_dev")
    return key, prf, opn, st


def column_sum(rows, curve="bls12_381", ctx: Context | None = None):
    """Stage 4's kernel: (n_rows, n_cols, 4) device scalars -> (n_cols, 4), the sum of every column mod r."""
    torch = _torch()
    cv = get_curve(curve)
    ctx = ctx or default_context(rows.device.index)
    n_rows, n_cols = rows.shape[0], rows.shape[1]
    out = torch.empty((n_cols, 4), dtype=torch.int64, device=rows.device)
    ctx.use_torch_stream()
    check(lib().zk_fr_column_sum_dev(ctx.handle, cv.curve_id, ptr_of(rows.contiguous()), n_rows, n_cols, ptr_of(out)), "zk_fr_column_sum_dev")
    return out


class _Resident:
    """what one batch leaves on the device: the decoded points as MSM bases and the scalar rows"""

    def __init__(self, n, key_rows, proof_rows, open_rows, proof_ck, open_ck, status, pts=None, inf=None):
        self.n, self.key_rows, self.proof_rows, self.open_rows = n, key_rows, proof_rows, open_rows
        self.proof_ck, self.open_ck, self.status = proof_ck, open_ck, status
        self.pts, self.inf = pts, inf             # the decoded points and their flags as plain tensors: the bases of `verdicts`

    def close(self):
        for ck in (self.proof_ck, self.open_ck):
            if ck is not None:
                ck.close()
        self.proof_ck = self.open_ck = None


class BatchVerifier:
    """B proofs of ONE circuit -> the two pairing inputs (L, R) and a status per proof; with a pairing key, valid or not.

    vk: the dict `ProverKey.verifier_key` returns (name -> G1Affine); n: the circuit's domain size; seeded_transcript: the
    `transcript.Transcript` after `seed_transcript(vk, n)`; coeff_a, coeff_d: the embedded curve's coefficients (4 Montgomery limbs).
    replay: where stage 2 runs -- "host", "device", or "auto" (the device from REPLAY_ON_DEVICE_FROM proofs); no result depends on it.
    pairing_key: the `pairing.PairingKey` of the verifier key's G2 points -- the check e(L, [tau]H) = e(R, H) behind `verify`,
    `verdicts` and `locate_invalid`; without one the verifier stops at (L, R) and `locate_invalid` takes the caller's check."""

    def __init__(self, vk: dict, n: int, seeded_transcript, coeff_a, coeff_d, curve="bls12_381", ctx: Context | None = None,
                 replay: str = "auto", pairing_key=None):
        torch = _torch()
        if replay not in ("host", "device", "auto"):
            raise ValueError('replay is "host", "device" or "auto"')
        self.replay = replay
        self.curve = get_curve(curve)
        if pairing_key is not None and pairing_key.curve != self.curve:
            raise ValueError("the pairing key is of another curve")
        self.pairing_key = pairing_key
        self.ctx = ctx or default_context(0)
        if n <= 0 or n & (n - 1):
            raise ValueError("the domain size is a power of two")
        self.n, self.log_n = n, n.bit_length() - 1
        self.seeded = seeded_transcript
        self.coeff_a = np.ascontiguousarray(coeff_a, dtype=np.uint64).reshape(4).copy()
        self.coeff_d = np.ascontiguousarray(coeff_d, dtype=np.uint64).reshape(4).copy()
        cv = self.curve
        pts = [vk[k] for k in KEY_BASES]
        g = fq_to_mont(cv, [cv.gx, cv.gy]).reshape(-1)
        xy = np.stack([np.asarray(p.xy(), dtype=np.uint64) for p in pts] + [g])
        inf = np.array([1 if p.infinity else 0 for p in pts] + [0], dtype=np.uint8)
        dev = torch.device("cuda", self.ctx.device)
        self._key_xy, self._key_inf = torch.from_numpy(xy.view(np.int64)).to(dev), torch.from_numpy(inf).to(dev)
        self._key_ck = CommitterKey(self._key_xy, cv, self.ctx, infinity=self._key_inf)
        self._res = None

    def close(self):
        if self._res is not None:
            self._res.close()
            self._res = None
        if self._key_ck is not None:
            self._key_ck.close()
            self._key_ck = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def random_weights(n_proofs: int) -> list:
        """128-bit non-zero weights from the operating system's randomness: what the soundness of the fold rests on"""
        return [(secrets.randbits(128) or 1, secrets.randbits(128) or 1) for _ in range(n_proofs)]

    def prepare(self, proofs, public_inputs=None, weights=None):
        """Stages 1-3 for a batch; the rows and the decoded points stay resident for `fold_range`.  Returns the statuses (B,) uint8."""
        torch = _torch()
        cv, ctx = self.curve, self.ctx
        B = len(proofs)
        if weights is None:
            weights = self.random_weights(B)
        if self._res is not None:
            self._res.close()
            self._res = None
        if B == 0:
            self._res = _Resident(0, None, None, None, None, None, np.zeros(0, dtype=np.uint8))
            return self._res.status
        if self.replay_on_device(B):
            pts, inf, key, prf, opn, st = self._stages_on_device(proofs, public_inputs, weights)
        else:
            # stage 1 first: the decode runs on the stream while the host replays the transcripts
            pts, inf, pst = decompress_batch(proof_point_bytes(proofs, cv), cv, ctx)
            ch, ev, parse_st = replay_batch(self.seeded, proofs, public_inputs, cv)
            key, prf, opn, st = scalar_rows(self.log_n, ch, ev, public_inputs, self.coeff_a, self.coeff_d, weights, parse_st, pst, cv, ctx)
        L2 = 2 * cv.fq_limbs
        proof_ck = CommitterKey(pts, cv, ctx, infinity=inf)                       # proof-major: proof j owns bases [15 j, 15 j + 15)
        o_pts = pts.view(B, N_PROOF_BASES, L2)[:, 13:15].contiguous().view(2 * B, L2)
        o_inf = inf.view(B, N_PROOF_BASES)[:, 13:15].contiguous().view(2 * B)
        open_ck = CommitterKey(o_pts, cv, ctx, infinity=o_inf)                    # the openings again, stride 2: the bases of L
        self._res = _Resident(B, key, prf, opn, proof_ck, open_ck, st.cpu().numpy(), pts, inf)
        return self._res.status

    def replay_on_device(self, n_proofs: int) -> bool:
        """where stage 2 of a batch of n_proofs runs under this verifier's `replay` setting"""
        if self.replay == "auto":
            return REPLAY_ON_DEVICE_FROM is not None and n_proofs >= REPLAY_ON_DEVICE_FROM
        return self.replay == "device"

    def _stages_on_device(self, proofs, public_inputs, weights):
        """Stages 2, 1, 3 behind ONE upload (proof bytes, offsets, public inputs, weights): the replay kernel's point encodings feed the
        decode, its rows and statuses the scalars; nothing is waited for."""
        torch = _torch()
        cv, ctx = self.curve, self.ctx
        B = len(proofs)
        if len(weights) != B:
            raise ValueError("one pair of weights per proof")
        w = ints_to_limbs([int(x) % cv.r for pair in weights for x in pair], 4)
        dev = torch.device("cuda", ctx.device)
        (d_poff, d_pioff, d_pos, d_vals, d_w), d_blob, n_bytes, n_pi = _upload_batch(proofs, public_inputs, [w], dev)
        ch, ev, enc, parse_st = _replay_dev(self.seeded, B, d_blob, n_bytes, d_poff, d_pioff, d_pos, d_vals, n_pi, cv, ctx)
        pts, inf, pst = decompress_batch(enc, cv, ctx)
        key, prf, opn, st = _scalars_dev(self.log_n, B, ch, ev, d_pioff, d_pos, d_vals, self.coeff_a, self.coeff_d, d_w, parse_st, pst, cv, ctx)
        return pts, inf, key, prf, opn, st

    def rows(self):
        """The prepared batch's resident scalar rows: device tensors (key (B, 20, 4), proof (B, 15, 4), openings (B, 2, 4)), canonical."""
        if self._res is None:
            raise RuntimeError("prepare a batch first")
        return self._res.key_rows, self._res.proof_rows, self._res.open_rows

    def fold_range(self, lo: int = 0, hi: int | None = None):
        """Stage 4 over the proofs [lo, hi) of the prepared batch: (L, R) as G1Affine.  Proofs with a non-zero status contribute
        nothing (their rows are zero)."""
        res = self._res
        if res is None:
            raise RuntimeError("prepare a batch first")
        hi = res.n if hi is None else hi
        if not 0 <= lo <= hi <= res.n:
            raise ValueError("range outside the batch")
        cv = self.curve
        if lo == hi:
            zero = np.zeros(cv.fq_limbs, dtype=np.uint64)
            one = fq_to_mont(cv, [1]).reshape(-1)
            return G1Affine(zero, one, True, cv.name), G1Affine(zero.copy(), one.copy(), True, cv.name)
        key_sum = column_sum(res.key_rows[lo:hi], cv, self.ctx)
        parts = [self._key_ck.msm_partial(key_sum),
                 res.proof_ck.msm_partial(res.proof_rows[lo:hi].reshape(-1, 4), N_PROOF_BASES * lo)]
        l_part = res.open_ck.msm_partial(res.open_rows[lo:hi].reshape(-1, 4), 2 * lo)
        return sum_partials(l_part.reshape(1, -1), cv), sum_partials(np.stack(parts), cv)

    def fold(self, proofs, public_inputs=None, weights=None, lo: int = 0, hi: int | None = None):
        """(L, R, statuses) of the proofs [lo, hi) of the batch.  weights: B pairs (u, u') of integers; None draws 128-bit non-zero
        values from the operating system -- never fix them: a prover who knows the weights can make invalid proofs cancel."""
        st = self.prepare(proofs, public_inputs, weights)
        L, R = self.fold_range(lo, hi)
        return L, R, st

    def _need_key(self):
        if self.pairing_key is None:
            raise ValueError("this verifier has no pairing key: pass pairing_key=PairingKey(h, tau_h, curve)")
        return self.pairing_key

    def verify(self, proofs, public_inputs=None, weights=None) -> bool:
        """True iff every proof of the batch is valid, except with probability about 2^-128 over the weights: no status is non-zero
        and the fold of the whole batch passes ONE pairing check, on the host.  weights: as `fold`."""
        key = self._need_key()
        st = self.prepare(proofs, public_inputs, weights)
        if np.any(st):
            return False
        return key.check(*self.fold_range())

    def pairing_inputs(self):
        """(L_j, R_j) of every proof of the prepared batch, each under its own weights: device tensors (xy_L (B, 2L), inf_L (B,),
        xy_R, inf_R), queued.  ONE `msm.segments_msm` call over [20 key points | 15 B proof points] with the resident rows as scalars,
        two segments per proof: 2 terms (the openings) for L_j, 35 for R_j.  Rows of a proof with a non-zero status are zero: both of
        its points are infinity."""
        torch = _torch()
        res = self._res
        if res is None:
            raise RuntimeError("prepare a batch first")
        B, dev = res.n, self._key_xy.device
        L2 = 2 * self.curve.fq_limbs
        if B == 0:
            e = torch.empty((0, L2), dtype=torch.int64, device=dev), torch.empty((0,), dtype=torch.uint8, device=dev)
            return e[0], e[1], e[0].clone(), e[1].clone()
        bases = torch.cat([self._key_xy, res.pts.view(-1, L2)])
        binf = torch.cat([self._key_inf, res.inf.view(-1)])
        own = N_KEY_BASES + N_PROOF_BASES * torch.arange(B, device=dev)[:, None]                  # proof j's first base
        idx_l = own + torch.arange(13, 15, device=dev)[None, :]
        idx_r = torch.cat([torch.arange(N_KEY_BASES, device=dev)[None, :].expand(B, N_KEY_BASES),
                           own + torch.arange(N_PROOF_BASES, device=dev)[None, :]], dim=1)
        index = torch.cat([idx_l, idx_r], dim=1).to(torch.int32).contiguous().view(-1)
        sc = torch.cat([res.open_rows, res.key_rows, res.proof_rows], dim=1).contiguous().view(-1, 4)
        per = 2 + N_KEY_BASES + N_PROOF_BASES
        off = (torch.arange(B, dtype=torch.int64, device=dev)[:, None] * per + torch.tensor([0, 2], dtype=torch.int64, device=dev)[None, :])
        off = torch.cat([off.view(-1), torch.tensor([B * per], dtype=torch.int64, device=dev)])
        xy, inf, st = segments_msm(bases, binf, off, index, sc, self.curve, self.ctx)
        self._seg_status = st
        xy, inf = xy.view(B, 2, L2), inf.view(B, 2)
        return xy[:, 0].contiguous(), inf[:, 0].contiguous(), xy[:, 1].contiguous(), inf[:, 1].contiguous()

    def verdicts(self, proofs, public_inputs=None, weights=None) -> np.ndarray:
        """Valid or not for every proof of the batch, with no bisection: (B,) bool.  After `prepare`, one segmented MSM gives every
        (L_j, R_j) and one launch runs the B pairing checks, one per lane.  A proof with a non-zero status is False without a pairing."""
        key = self._need_key()
        st = self.prepare(proofs, public_inputs, weights)
        if len(proofs) == 0:
            return np.zeros(0, dtype=bool)
        xy_l, inf_l, xy_r, inf_r = self.pairing_inputs()
        ok = key.check_batch(xy_l, inf_l, xy_r, inf_r, self.ctx).cpu().numpy()
        if int(self._seg_status.max()) != 0:
            raise RuntimeError("segments_msm: a segment of the batch's own layout was refused")
        return (ok != 0) & (st == 0)

    def locate_invalid(self, proofs, public_inputs, accepts=None, weights=None) -> list:
        """Indices of the proofs that do not verify: those with a non-zero status, and those a bisection over ranges finds with
        `accepts(L, R) -> bool` -- the verifier's own pairing key when `accepts` is None, else the caller's check.  The rows stay
        resident, so a range costs one fold; `accepts` is called at most 1 + 2 k ceil(log2 B) times for k failing proofs."""
        if accepts is None:
            accepts = self._need_key().check
        st = self.prepare(proofs, public_inputs, weights)
        bad = {int(j) for j in np.nonzero(st)[0]}
        B = len(proofs)

        def ok(lo, hi):
            return bool(accepts(*self.fold_range(lo, hi)))

        def search(lo, hi):                      # [lo, hi) is known to fail
            if hi - lo == 1:
                bad.add(lo)
                return
            mid = (lo + hi) // 2
            if ok(lo, mid):                      # then the failure is on the right: no check needed there
                search(mid, hi)
                return
            search(lo, mid)
            if not ok(mid, hi):
                search(mid, hi)

        if B and not ok(0, B):
            search(0, B)
        return sorted(bad)


class IpaBatchVerifier:
    """B proofs of ONE circuit under the inner-product-argument commitment -> valid or not.  IPA needs no
    pairing: where `BatchVerifier` ends in `pairing.PairingKey`, this verifier ends in `IpaCommitterKey.batch_check`.

    The stages in front of the openings are `BatchVerifier`'s, on a KZG-shaped byte string per proof (13 commitments, the two
    final_comm_keys where the KZG witnesses stand, the evaluations): proof.rs never appends an opening to the transcript
    (csrc/replay_walk.cuh), so the challenges are the proof's own, and the final keys get the opening points' curve and subgroup checks.
    The IPA check hashes each opening's combined commitment C = sum_k chi^k C_k, so unlike the KZG fold every proof needs its own two
    small MSMs as points: zk_verify_scalars_dev under the weights (1, 0) and (0, 1) gives their scalars (key columns 0..18, proof
    columns 0..12; the G column is -v), and ONE `msm.segments_msm` call over [20 key points | 15 B proof points] gives all 2 B of them.
    The 2 B openings ([C], [v], z or z w, the parsed ipa_pc::Proof) then go to `IpaCommitterKey.batch_check` / `locate_invalid`.

    vk, n, seeded_transcript, coeff_a, coeff_d, replay: as `BatchVerifier`; ipa_key: the `IpaCommitterKey` the proofs were made
    under; digest: the hash of ipa_pc's transcript."""

    def __init__(self, vk: dict, n: int, seeded_transcript, coeff_a, coeff_d, ipa_key, curve="bls12_381", ctx: Context | None = None,
                 digest: str = "blake2b", replay: str = "auto"):
        torch = _torch()
        from .domain import Radix2EvaluationDomain
        if replay not in ("host", "device", "auto"):
            raise ValueError('replay is "host", "device" or "auto"')
        self.replay, self.digest, self.ipa_key = replay, digest, ipa_key
        self.curve = cv = get_curve(curve)
        self.ctx = ctx or ipa_key.ctx
        if n <= 0 or n & (n - 1):
            raise ValueError("the domain size is a power of two")
        self.n, self.log_n = n, n.bit_length() - 1
        self.seeded = seeded_transcript
        self.coeff_a = np.ascontiguousarray(coeff_a, dtype=np.uint64).reshape(4).copy()
        self.coeff_d = np.ascontiguousarray(coeff_d, dtype=np.uint64).reshape(4).copy()
        self.omega = fr_from_mont(cv, np.asarray(Radix2EvaluationDomain.new(n, cv, self.ctx).group_gen()).reshape(1, 4))[0]
        pts = [vk[k] for k in KEY_BASES]
        g = fq_to_mont(cv, [cv.gx, cv.gy]).reshape(-1)
        xy = np.stack([np.asarray(p.xy(), dtype=np.uint64) for p in pts] + [g])
        inf = np.array([1 if p.infinity else 0 for p in pts] + [0], dtype=np.uint8)
        dev = torch.device("cuda", self.ctx.device)
        self._key_xy, self._key_inf = torch.from_numpy(xy.view(np.int64)).to(dev), torch.from_numpy(inf).to(dev)
        self.last = None             # what the last batch left: per-proof C_aw, C_saw, v_aw, v_saw, statuses (tests, tools)

    replay_on_device = BatchVerifier.replay_on_device

    def split(self, proofs):
        """Stage 1's host half: every proof -> (its KZG-shaped bytes, [aw fields, saw fields] of `ipa_proof_parse`), and the indices of
        the proofs whose IPA parts do not parse (their KZG-shaped bytes are empty: stage 2 reports them too)."""
        cv, log_d = self.curve, self.ipa_key.log_d
        g = 8 * cv.fq_limbs
        shaped, parts, bad = [], [], []
        for j, p in enumerate(proofs):
            p = bytes(p)
            st1, f1, e1 = ipa_proof_parse(p, cv, log_d, 13 * g) if len(p) >= 13 * g else (IPA_PROOF_TRUNCATED, None, None)
            st2, f2, e2 = ipa_proof_parse(p, cv, log_d, e1) if st1 == IPA_PROOF_OK else (st1, None, None)
            if st2 != IPA_PROOF_OK:
                bad.append(j)
                shaped.append(b"")
                parts.append(None)
                continue
            shaped.append(p[:13 * g] + f1[2] + b"\x00" + f2[2] + b"\x00" + p[e2:])
            parts.append((f1, f2))
        return shaped, parts, bad

    def _stages(self, shaped, public_inputs):
        """Stages 1 (head) to 2 and the scalars under (1, 0) and (0, 1) -> points, flags, (key, proof rows) x 2, challenges, status"""
        torch = _torch()
        cv, ctx = self.curve, self.ctx
        B = len(shaped)
        w_aw, w_saw = [(1, 0)] * B, [(0, 1)] * B
        if self.replay_on_device(B):
            dev = torch.device("cuda", ctx.device)
            wa, ws = ints_to_limbs([x for pr in w_aw for x in pr], 4), ints_to_limbs([x for pr in w_saw for x in pr], 4)
            (d_poff, d_pioff, d_pos, d_vals, d_wa, d_ws), d_blob, n_bytes, n_pi = _upload_batch(shaped, public_inputs, [wa, ws], dev)
            ch, ev, enc, parse_st = _replay_dev(self.seeded, B, d_blob, n_bytes, d_poff, d_pioff, d_pos, d_vals, n_pi, cv, ctx)
            pts, inf, pst = decompress_batch(enc, cv, ctx)
            rows = [_scalars_dev(self.log_n, B, ch, ev, d_pioff, d_pos, d_vals, self.coeff_a, self.coeff_d, d_w, parse_st, pst, cv, ctx)
                    for d_w in (d_wa, d_ws)]
        else:
            pts, inf, pst = decompress_batch(proof_point_bytes(shaped, cv), cv, ctx)
            ch, ev, parse_st = replay_batch(self.seeded, shaped, public_inputs, cv)
            rows = [scalar_rows(self.log_n, ch, ev, public_inputs, self.coeff_a, self.coeff_d, w, parse_st, pst, cv, ctx) for w in (w_aw, w_saw)]
        return pts, inf, rows, ch

    def combined_commitments(self, pts, inf, rows):
        """Stage 3: C_aw and C_saw of every proof, 2 B segments of 32 terms over [20 key points | 15 B proof points] in one launch
        (an opening uses fewer of the 32 columns: the others carry zero scalars and cost nothing).  Term arrays by torch indexing."""
        torch = _torch()
        B = rows[0][0].shape[0]
        dev = pts.device
        bases = torch.cat([self._key_xy, pts])
        binf = torch.cat([self._key_inf, inf])
        cols = torch.cat([torch.arange(19, device=dev), N_KEY_BASES + torch.arange(13, device=dev)])
        shift = torch.cat([torch.zeros(19, dtype=torch.int64, device=dev), torch.full((13,), N_PROOF_BASES, dtype=torch.int64, device=dev)])
        index = cols[None, None, :] + shift[None, None, :] * torch.arange(B, device=dev)[:, None, None]
        index = index.expand(B, 2, 32).to(torch.int32).contiguous().view(-1)
        sc = torch.stack([torch.cat([key[:, :19], prf[:, :13]], dim=1) for key, prf, _, _ in rows], dim=1).contiguous().view(-1, 4)
        off = torch.arange(2 * B + 1, dtype=torch.int64, device=dev) * 32
        return segments_msm(bases, binf, off, index, sc, self.curve, self.ctx)

    def openings(self, proofs, public_inputs=None):
        """Stages 1-4 up to the openings: (the 2 B' `IpaOpening`s of the B' proofs that got this far, their indices, the sorted indices
        of the proofs already known invalid: malformed bytes, a point that does not decode, a status of the scalars stage)."""
        torch = _torch()
        cv, ctx, ik = self.curve, self.ctx, self.ipa_key
        B, L, log_d = len(proofs), cv.fq_limbs, ik.log_d
        if public_inputs is not None and len(public_inputs) != B:
            raise ValueError("one public-input map per proof")
        if B == 0:
            self.last = {"C": [], "v": [], "status": np.zeros(0, dtype=np.uint8)}
            return [], [], []
        shaped, parts, bad = self.split(proofs)
        bad = set(bad)
        # the 4 log_d L / R encodings of every proof (infinity encodings for a proof that did not parse), decoded in one more call
        g = 8 * L
        inf_enc = bytes(g - 1) + b"\x40"
        lr = b"".join(inf_enc * (4 * log_d) if pp is None else b"".join(pp[0][0] + pp[0][1] + pp[1][0] + pp[1][1]) for pp in parts)
        pts, inf, rows, ch = self._stages(shaped, public_inputs)
        c_xy, c_inf, c_st = self.combined_commitments(pts, inf, rows)
        if log_d:
            lr_xy, lr_inf, lr_st = decompress_batch(lr, cv, ctx)
            lr_bad = lr_st.view(B, 4 * log_d).max(dim=1).values.cpu().numpy()
        else:
            lr_bad = np.zeros(B, dtype=np.uint8)
        status = np.maximum(rows[0][3].cpu().numpy(), rows[1][3].cpu().numpy())
        if int(c_st.max()) != 0:
            raise RuntimeError("segments_msm: a segment of the batch's own layout was refused")
        bad |= {int(j) for j in np.nonzero(status)[0]} | {int(j) for j in np.nonzero(lr_bad)[0]}

        def points(xy, flags):
            ints = fq_from_mont(cv, xy.cpu().numpy().view(np.uint64).reshape(-1, L))
            return [None if f else (ints[2 * k], ints[2 * k + 1]) for k, f in enumerate(flags.cpu().numpy().tolist())]

        C = points(c_xy, c_inf)                                                    # 2 B: C_aw, C_saw per proof
        neg_v = [limbs_to_ints(rows[k][0][:, N_KEY_BASES - 1].contiguous().cpu().numpy().view(np.uint64)) for k in (0, 1)]
        v = [[-x % cv.r for x in col] for col in neg_v]
        z_rows = ch[:, CHALLENGES.index("z")]
        z = fr_from_mont(cv, z_rows.contiguous().cpu().numpy().view(np.uint64) if torch.is_tensor(z_rows) else z_rows)
        heads = points(pts.view(B, N_PROOF_BASES, 2 * L)[:, 13:15].contiguous(), inf.view(B, N_PROOF_BASES)[:, 13:15].contiguous().view(-1))
        lrp = points(lr_xy, lr_inf) if log_d else []
        self.last = {"C": C, "v": [(v[0][j], v[1][j]) for j in range(B)], "status": status}
        good = [j for j in range(B) if j not in bad]
        out = []
        for j in good:
            for k in (0, 1):
                at = (4 * j + 2 * k) * log_d
                pr = IpaProof(lrp[at:at + log_d], lrp[at + log_d:at + 2 * log_d], heads[2 * j + k], parts[j][k][3])
                out.append(IpaOpening([C[2 * j + k]], z[j] * (self.omega if k else 1) % cv.r, [v[k][j]], pr, 1))
        return out, good, sorted(bad)

    def verify(self, proofs, public_inputs=None, weights=None) -> bool:
        """True iff every proof of the batch is valid (up to the soundness error of `IpaCommitterKey.batch_check`).  weights: one pair
        per OPENING (two openings per proof that reaches the openings stage) -- for tests; None draws them from the operating system."""
        ops, good, bad = self.openings(list(proofs), public_inputs)
        if bad:
            return False
        return self.ipa_key.batch_check(ops, weights, self.digest)

    def locate_invalid(self, proofs, public_inputs=None) -> list:
        """Indices of the proofs that do not verify, malformed ones included: opening j belongs to proof j // 2 of those that reached
        the openings stage."""
        ops, good, bad = self.openings(list(proofs), public_inputs)
        return sorted(set(bad) | {good[j // 2] for j in self.ipa_key.locate_invalid(ops, self.digest)})
