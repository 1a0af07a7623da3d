"""CPU suite of the batch verifier's host stage (csrc/wire.hip zk_proof_replay_batch) and of the new entry points' argument checks.

The proofs are real: `oracle/prover_oracle.py::prove` at 32 rows on both curves, with a committer that returns poly(tau) G by the big-int
group law (no device), accepted by the restated verifier (`oracle/verifier_oracle.py`).  The library's parse and replay must give that
verifier's challenges and evaluations; malformed bytes must each be told apart by status, never crash."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ark_plonk_amd as zk  # noqa: E402
from ark_plonk_amd import _lib, transcript, verifier  # noqa: E402
from ark_plonk_amd.curves import fq_to_mont, fr_from_mont, fr_to_mont  # noqa: E402
from oracle import bigint_oracle as bo  # noqa: E402
from oracle import prover_oracle as po  # noqa: E402
from oracle import verifier_oracle as vo  # noqa: E402
from oracle import wire_oracle as wo  # noqa: E402
from tests.conftest import TAU  # noqa: E402
from tests.test_prover_gpu import KEY, build_circuit  # noqa: E402

LOG_N = 5
LABEL = b"batch verifier"
LIB_NAME = dict(KEY, sigma0="left_sigma", sigma1="right_sigma", sigma2="out_sigma", sigma3="fourth_sigma")
CH_NAMES = ("zeta", "beta", "gamma", "delta", "epsilon", "alpha", "range", "logic", "fixed", "var", "lookup", "z", "aw", "saw")
CUSTOM = ("a_next_eval", "b_next_eval", "d_next_eval", "q_arith_eval", "q_c_eval", "q_l_eval", "q_r_eval")


def affine(cid, P):
    cv = zk.get_curve(cid)
    if P is None:
        return zk.G1Affine(np.zeros(cv.fq_limbs, dtype=np.uint64), fq_to_mont(cid, [1])[0], True, cv.name)
    return zk.G1Affine(fq_to_mont(cid, [P[0]])[0], fq_to_mont(cid, [P[1]])[0], False, cv.name)


class Case:
    """one valid proof, the two seeded transcripts, what the oracle reads out of it"""

    def __init__(self, cid):
        self.cid, self.cv = cid, bo.CURVES[cid]
        cv, n = self.cv, 1 << LOG_N
        self.ca, self.cd = bo.seeded_scalars(cv, 0x51, 2)
        sel, sigma, table, wires, pub = build_circuit(cv, LOG_N, 7 + LOG_N + cid, False, (self.ca, self.cd))
        G = (cv.gx, cv.gy)
        commit = lambda coeffs: bo.ec_mul(cv, bo.horner(coeffs, TAU, cv.r), G)   # noqa: E731  poly(tau) G
        osel = {k: sel[v] for k, v in KEY.items()}
        ifft = lambda ev: bo.ntt(cv, 1, LOG_N, ev)                               # noqa: E731
        self.vk_pts = {k: commit(ifft(v)) for k, v in osel.items()}
        self.vk_pts.update({f"sigma{k}": commit(ifft(sigma[k])) for k in range(4)})
        self.pub = pub
        self.data, self.prover_ch, polys = po.prove(cv, LOG_N, osel, sigma, table, wires, pub, self.oracle_seeded(), commit, self.ca, self.cd)
        dlog = {k: bo.horner(v, TAU, cv.r) for k, v in polys.items()}
        ok, _, det = vo.verify_with_trapdoor(cv, LOG_N, self.data, self.oracle_seeded(), pub, dlog, TAU, self.ca, self.cd)
        assert ok, det
        t = transcript.Transcript(LABEL, cid)
        self.seeded = transcript.seed_transcript(t, {LIB_NAME[k]: affine(cid, P) for k, P in self.vk_pts.items() if k in LIB_NAME}, n)

    def oracle_seeded(self):
        return vo.seed_transcript(self.cv, wo.PlonkTranscript(LABEL, self.cv), self.vk_pts, 1 << LOG_N)

    def oracle_replay(self, data, pub):
        proof = vo.parse_proof(self.cv, data)
        return proof, vo.replay_transcript(self.cv, self.oracle_seeded(), proof, pub)

    def lib_replay(self, data, pub, with_points=False):
        pi = {i: fr_to_mont(self.cid, [v])[0] for i, v in pub.items()}
        return verifier.replay_batch(self.seeded, [data], [pi], self.cid, with_points=with_points)


@pytest.fixture(scope="module")
def cases():
    return {cid: Case(cid) for cid in (0, 1)}


def assert_rows_match(case, data, pub):
    proof, ch = case.oracle_replay(data, pub)
    got_ch, got_ev, st = case.lib_replay(data, pub)
    assert st.tolist() == [verifier.PROOF_OK]
    assert fr_from_mont(case.cid, got_ch[0]) == [ch[k] for k in CH_NAMES]
    assert fr_from_mont(case.cid, got_ev[0]) == [proof["evals"][k] for k in vo.EVALS + CUSTOM]
    assert verifier.CHALLENGES == CH_NAMES and verifier.EVALS == vo.EVALS + CUSTOM


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("n_pi", [0, 1, 3])
def test_replay_matches_the_oracle(cases, cid, n_pi):
    case = cases[cid]
    n = 1 << LOG_N
    pub = {pos: v for pos, v in zip((0, 7, n - 1), bo.seeded_scalars(case.cv, 0x77 + n_pi, 3))}
    pub = dict(list(pub.items())[:n_pi])
    assert_rows_match(case, case.data, pub)
    # the proof's own public inputs give the challenges its prover drew; the seeded transcript was not consumed by the calls above
    _, ch = case.oracle_replay(case.data, case.pub)
    got_ch, _, _ = case.lib_replay(case.data, case.pub)
    assert fr_from_mont(cid, got_ch[0]) == [ch[k] for k in CH_NAMES]
    assert all(ch[k] == case.prover_ch[k] for k in CH_NAMES)


@pytest.mark.parametrize("cid", [0, 1])
def test_a_zero_public_input_is_not_part_of_the_message(cases, cid):
    case = cases[cid]
    pub = dict(case.pub)
    pub[9] = 0
    assert_rows_match(case, case.data, pub)


def layout(cv):
    g, f = wo.fq_flag_bytes(cv), wo.fr_bytes(cv)
    evals0 = 15 * g + 2
    return g, f, evals0, evals0 + 16 * f          # point size, scalar size, offset of the evaluations, offset of the custom count


def drop_label(cv, data, label):
    g, f, _, cnt = layout(cv)
    k = int.from_bytes(data[cnt:cnt + 8], "little")
    pos, out = cnt + 8, b""
    for _ in range(k):
        ln = int.from_bytes(data[pos:pos + 8], "little")
        entry = data[pos:pos + 8 + ln + f]
        if data[pos + 8:pos + 8 + ln] != label:
            out += entry
        pos += len(entry)
    return data[:cnt] + (k - 1).to_bytes(8, "little") + out


@pytest.mark.parametrize("cid", [0, 1])
def test_malformed_bytes_each_give_their_own_status(cases, cid):
    case = cases[cid]
    cv, d = case.cv, case.data
    g, f, ev0, cnt = layout(cv)
    k = int.from_bytes(d[cnt:cnt + 8], "little")
    bad = {
        "truncated": (d[:-1], verifier.PROOF_TRUNCATED),
        "trailing": (d + b"\x00", verifier.PROOF_TRAILING),
        "option": (d[:14 * g] + b"\x01" + d[14 * g + 1:], verifier.PROOF_BAD_OPTION),
        "eval = r": (d[:ev0 + 3 * f] + cv.r.to_bytes(f, "little") + d[ev0 + 4 * f:], verifier.PROOF_FR_NOT_REDUCED),
        "label removed": (drop_label(cv, d, b"q_c_eval"), verifier.PROOF_MISSING_LABEL),
        "count inflated": (d[:cnt] + (k + 1).to_bytes(8, "little") + d[cnt + 8:], verifier.PROOF_BAD_COUNT),
    }
    assert len({st for _, st in bad.values()}) == len(bad)
    for name, (data, want) in bad.items():
        ch, ev, st = case.lib_replay(data, case.pub)
        assert st.tolist() == [want], name
        assert not ch.any() and not ev.any(), name                     # a rejected proof leaves zero rows
    # ... each in a batch next to the good proof, which is not disturbed; and degenerate inputs
    datas = [d] + [x for x, _ in bad.values()] + [b"", d[:5], d[:cnt + 3], d[:cnt] + (1 << 63).to_bytes(8, "little") + d[cnt + 8:]]
    pi = {i: fr_to_mont(cid, [v])[0] for i, v in case.pub.items()}
    ch, ev, st = verifier.replay_batch(case.seeded, datas, [pi] * len(datas), cid)
    _, want_ch = case.oracle_replay(d, case.pub)
    assert fr_from_mont(cid, ch[0]) == [want_ch[k] for k in CH_NAMES]
    assert st.tolist() == [0] + [s for _, s in bad.values()] + [verifier.PROOF_TRUNCATED] * 3 + [verifier.PROOF_BAD_COUNT]
    # the second option byte, and a custom evaluation that is not reduced
    ch, ev, st = case.lib_replay(d[:15 * g + 1] + b"\x01" + d[15 * g + 2:], case.pub)
    assert st.tolist() == [verifier.PROOF_BAD_OPTION]
    ch, ev, st = case.lib_replay(d[:-f] + cv.r.to_bytes(f, "little"), case.pub)
    assert st.tolist() == [verifier.PROOF_FR_NOT_REDUCED]
    # public inputs out of order are the caller's mistake, told apart from the proof's
    off = np.array([0, 2], dtype=np.uint64)
    pos = np.array([5, 3], dtype=np.uint64)
    vals = fr_to_mont(cid, [1, 2])
    buf = (ctypes.c_char_p * 1)(d)
    lens = (ctypes.c_size_t * 1)(len(d))
    ch1, ev1, st1 = np.zeros((14, 4), np.uint64), np.zeros((23, 4), np.uint64), np.zeros(1, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)          # noqa: E731
    assert _lib.lib().zk_proof_replay_batch(case.seeded._h, cid, 1, buf, lens, p(off), p(pos), p(vals), p(ch1), p(ev1), None, p(st1)) == 0
    assert st1.tolist() == [verifier.PROOF_BAD_PUBLIC_INPUTS]


@pytest.mark.parametrize("cid", [0, 1])
def test_infinity_with_stray_x_bits_replays_in_canonical_form(cases, cid):
    """ark re-serialises the decoded point into the transcript: an infinity-flagged commitment is appended with x = 0 whatever its
    bytes held."""
    case = cases[cid]
    g = wo.fq_flag_bytes(case.cv)
    enc = bytearray((5).to_bytes(g, "little"))
    enc[-1] |= 0x40
    assert wo.de_g1(case.cv, bytes(enc)) is None
    for idx in (0, 5, 12):                                             # a wire commitment, f, t_4
        data = case.data[:idx * g] + bytes(enc) + case.data[(idx + 1) * g:]
        assert_rows_match(case, data, case.pub)
        _, ch = case.oracle_replay(data, case.pub)
        assert ch["zeta" if idx == 0 else "z"] != case.prover_ch["zeta" if idx == 0 else "z"]


@pytest.mark.parametrize("cid", [0, 1])
def test_point_bytes_by_offset_equal_the_parsed_ones(cases, cid):
    case = cases[cid]
    g = wo.fq_flag_bytes(case.cv)
    _, _, st, pts = case.lib_replay(case.data, case.pub, with_points=True)
    assert np.array_equal(pts, verifier.proof_point_bytes([case.data], cid))
    proof = vo.parse_proof(case.cv, case.data)
    want = [proof["commitments"][k] for k in vo.COMMITMENTS] + [proof["aw_opening"], proof["saw_opening"]]
    assert [wo.de_g1(case.cv, pts[0, k].tobytes()) for k in range(15)] == want
    # a proof that stage 2 rejects hands stage 1 infinity encodings, by either route
    _, _, st, pts = case.lib_replay(case.data[:-1], case.pub, with_points=True)
    short = verifier.proof_point_bytes([case.data[:15 * g]], cid)
    assert st[0] != 0 and (pts[0, :, -1] == 0x40).all() and not pts[0, :, :-1].any() and np.array_equal(short, pts)


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_parse_and_replay_under_asan_ubsan(tmp_path):
    """tests/sanitize/fuzz_replay.cpp, a program of its own linked with csrc/wire.hip (host code only): truncations at every length,
    length fields around and far beyond the buffer, random flips -- each in a heap block of exactly its size."""
    import subprocess
    exe = str(tmp_path / "fuzz_replay")
    csrc = os.path.join(ROOT, "ark_plonk_amd", "csrc")
    cmd = [HIPCC, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(csrc, "wire.hip"), "-x", "c++",
           os.path.join(ROOT, "tests", "sanitize", "fuzz_replay.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "fuzz_replay ok" in run.stdout and "runtime error" not in run.stderr


def test_null_arguments_are_refused(cases):
    L = _lib.lib()
    bad = _lib.ZK_ERR_BAD_ARG
    assert L.zk_g1_decompress_batch_dev(None, 0, None, 0, None, None, None) == bad
    assert L.zk_g1_decompress_batch_dev(None, 0, None, 4, None, None, None) == bad
    assert L.zk_verify_scalars_dev(None, 0, 5, 0, *([None] * 14)) == bad
    assert L.zk_fr_column_sum_dev(None, 0, None, 0, 20, None) == bad
    assert L.zk_proof_replay_batch(None, 0, 0, None, None, *([None] * 7)) == bad
    seeded = cases[0].seeded._h
    assert L.zk_proof_replay_batch(seeded, 7, 0, None, None, *([None] * 7)) == bad          # unknown curve
    assert L.zk_proof_replay_batch(seeded, 0, 1, None, None, *([None] * 7)) == bad          # a proof announced, none given
    assert L.zk_proof_replay_batch(seeded, 0, 0, None, None, *([None] * 7)) == _lib.ZK_OK   # an empty batch is no error
    buf = (ctypes.c_char_p * 1)(cases[0].data)
    lens = (ctypes.c_size_t * 1)(len(cases[0].data))
    off = np.zeros(2, dtype=np.uint64)
    assert L.zk_proof_replay_batch(seeded, 0, 1, buf, lens, off.ctypes.data_as(ctypes.c_void_p), *([None] * 6)) == bad   # no outputs
    for name in ("zk_g1_decompress_batch_dev", "zk_proof_replay_batch", "zk_verify_scalars_dev", "zk_fr_column_sum_dev"):
        assert name in _lib.SYMBOLS
    assert zk.BatchVerifier is verifier.BatchVerifier
