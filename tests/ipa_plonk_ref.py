"""TEST INFRASTRUCTURE -- the reference verifier of a PLONK proof under the inner-product-argument commitment, on integers: the
checker of tests/test_ipa_plonk_gpu.py.

`Proof::verify` (proof.rs:110-425) with PC = ipa_pc: oracle.verifier_oracle's parse / replay / r_0 / linearisation terms over the
KZG-shaped head of the proof (13 commitments, the two final_comm_keys where the KZG witnesses stand, the evaluations), then, in place
of the two pairing checks, tests/ipa_oracle.py's `check` over a known-logarithm key: the caller knows the logarithm of every commitment
(the tau-powers of tests/conftest.py are a valid comm_key, h a known multiple of G), so each opening's combined commitment is Fr
arithmetic and a point only where the transcript needs one.  The byte layout of the two ipa_pc::Proofs is walked here on its own (not
through ark_plonk_amd.ipa.ipa_proof_parse); the hash is ark_plonk_amd.ipa.transcript_hash, the one holder of those encodings."""
from __future__ import annotations

import ipa_oracle as io
from ark_plonk_amd.ipa import IpaProof
from oracle import verifier_oracle as vo
from oracle import wire_oracle as wo


def split_proof(cv, data: bytes, log_d: int):
    """-> (KZG-shaped bytes, [aw, saw] as (l encodings, r encodings, key encoding, c)); ValueError on malformed bytes"""
    g = wo.fq_flag_bytes(cv)
    pos = 13 * g
    parts = []
    for _ in range(2):
        vecs = []
        for _ in range(2):
            if pos + 8 > len(data) or int.from_bytes(data[pos:pos + 8], "little") != log_d:
                raise ValueError("l_vec / r_vec count")
            pos += 8
            vecs.append([data[pos + k * g:pos + (k + 1) * g] for k in range(log_d)])
            pos += log_d * g
        if pos + g + 34 > len(data):
            raise ValueError("truncated")
        key, c = data[pos:pos + g], int.from_bytes(data[pos + g:pos + g + 32], "little")
        pos += g + 32
        if data[pos:pos + 2] != b"\x00\x00" or c >= cv.r:
            raise ValueError("option byte or c")
        pos += 2
        parts.append((vecs[0], vecs[1], key, c))
    return data[:13 * g] + parts[0][2] + b"\x00" + parts[1][2] + b"\x00" + data[pos:], parts


def verify(cv, log_n, data, vk_pts, pub, dlog, key_logs, k_h, coeff_a, coeff_d, digest="blake2b", label=b"end to end"):
    """dlog: name -> logarithm of the 13 proof commitments and the verifier key's (test_prover_gpu.dlogs; a caller who replaces a
    commitment passes that point's logarithm); key_logs, k_h: the logarithms of comm_key and h.  Returns (ok, details)."""
    p = cv.r
    log_d = len(key_logs).bit_length() - 1
    try:
        shaped, parts = split_proof(cv, bytes(data), log_d)
        proof = vo.parse_proof(cv, shaped)
        ipa = [IpaProof([wo.de_g1(cv, e) for e in l], [wo.de_g1(cv, e) for e in r], wo.de_g1(cv, key), c) for l, r, key, c in parts]
    except (ValueError, AssertionError, IndexError) as err:
        return False, {"malformed": str(err)}
    ev = proof["evals"]
    t = vo.seed_transcript(cv, wo.PlonkTranscript(label, cv), vk_pts, 1 << log_n)
    ch = vo.replay_transcript(cv, t, proof, pub)
    ch.update(coeff_a=coeff_a, coeff_d=coeff_d)
    r0 = vo.compute_r0(cv, log_n, ev, ch, pub)
    lin = sum(s * dlog[name] for name, s in vo.linearisation_terms(cv, log_n, ev, ch)) % p
    ze = ch["zeta"]
    table = (dlog["table_1"] + ze * dlog["table_2"] + ze * ze % p * dlog["table_3"] + ze * ze * ze % p * dlog["table_4"]) % p
    aw = [(lin, -r0 % p), (dlog["sigma0"], ev["left_sigma_eval"]), (dlog["sigma1"], ev["right_sigma_eval"]), (dlog["sigma2"], ev["out_sigma_eval"]),
          (dlog["f_comm"], ev["f_eval"]), (dlog["h_2_comm"], ev["h2_eval"]), (table, ev["table_eval"]), (dlog["a_comm"], ev["a_eval"]),
          (dlog["b_comm"], ev["b_eval"]), (dlog["c_comm"], ev["c_eval"]), (dlog["d_comm"], ev["d_eval"])]
    saw = [(dlog["z_comm"], ev["permutation_eval"]), (dlog["a_comm"], ev["a_next_eval"]), (dlog["b_comm"], ev["b_next_eval"]),
           (dlog["d_comm"], ev["d_next_eval"]), (dlog["h_1_comm"], ev["h1_next_eval"]), (dlog["z_2_comm"], ev["z2_next_eval"]),
           (table, ev["table_next_eval"])]
    z = ch["z"]
    KL = io.KnownLog(cv)
    oks, Cs, vs = [], [], []
    for pairs, chi, point, pr in ((aw, ch["aw"], z, ipa[0]), (saw, ch["saw"], z * cv.root_of_unity(log_n) % p, ipa[1])):
        C = sum(pow(chi, k, p) * c_log for k, (c_log, _) in enumerate(pairs)) % p
        v = sum(pow(chi, k, p) * val for k, (_, val) in enumerate(pairs)) % p
        Cs.append(KL.point(C) if C else None)
        vs.append(v)
        oks.append(io.check(KL, key_logs, k_h, [C], point, [v], pr, 1, digest))
        if not oks[-1]:                                     # Proof::verify stops at the first opening that fails
            break
    return all(oks), {"openings": oks, "C": Cs, "v": vs, "challenges": ch}
