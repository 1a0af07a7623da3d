"""The byte layout of an ipa_pc::Proof inside a PLONK proof (ark_plonk_amd.ipa.ipa_proof_bytes / ipa_proof_parse), on hand-built
bytes: the layout round-trips, and every malformed form is a status, never an exception.  No GPU."""
import pytest

from ark_plonk_amd import ipa
from ark_plonk_amd.curves import get_curve
from oracle import bigint_oracle as bo
from oracle import wire_oracle as wo


def hand_built(cid, log_d, c):
    """the bytes written out field by field, and the proof they encode"""
    cv = bo.CURVES[cid]
    G = (cv.gx, cv.gy)
    pts = [bo.ec_mul(cv, k + 2, G) for k in range(2 * log_d + 1)]
    if log_d:
        pts[1] = None                                                  # an infinity among the L
        pts[log_d] = bo.ec_neg(cv, pts[log_d])                         # the other root among the R
    l, r, key = pts[:log_d], pts[log_d:2 * log_d], pts[2 * log_d]
    data = log_d.to_bytes(8, "little") + b"".join(wo.ser_g1(cv, p) for p in l)
    data += log_d.to_bytes(8, "little") + b"".join(wo.ser_g1(cv, p) for p in r)
    data += wo.ser_g1(cv, key) + c.to_bytes(32, "little") + b"\x00" + b"\x00"
    return data, ipa.IpaProof(l, r, key, c)


@pytest.mark.parametrize("log_d", [0, 1, 5])
@pytest.mark.parametrize("cid", [0, 1])
def test_layout_round_trips(cid, log_d):
    cv = bo.CURVES[cid]
    g = wo.fq_flag_bytes(cv)
    data, proof = hand_built(cid, log_d, cv.r - 1)
    assert len(data) == 16 + (2 * log_d + 1) * g + 34
    assert ipa.ipa_proof_bytes(proof, cid) == data                     # the library's encoder writes the hand-built bytes
    for pre, post in ((b"", b""), (b"\x07" * 13, b"tail")):            # at an offset, with bytes behind it
        st, fields, end = ipa.ipa_proof_parse(pre + data + post, cid, log_d, len(pre))
        assert st == ipa.IPA_PROOF_OK and end == len(pre) + len(data)
        l, r, key, c = fields
        assert [wo.de_g1(cv, e) for e in l] == proof.l_vec and [wo.de_g1(cv, e) for e in r] == proof.r_vec
        assert wo.de_g1(cv, key) == proof.final_comm_key and c == proof.c
    for p in proof.l_vec + proof.r_vec + [proof.final_comm_key]:       # the point encoding is the independent serialiser's
        assert ipa.g1_compress(cid, p) == wo.ser_g1(cv, p)
    assert get_curve(cid).fq_limbs * 8 == g


@pytest.mark.parametrize("cid", [0, 1])
def test_malformed_bytes_are_statuses(cid):
    cv = bo.CURVES[cid]
    g = wo.fq_flag_bytes(cv)
    log_d = 3
    data, _ = hand_built(cid, log_d, 5)
    parse = lambda b, k=log_d: ipa.ipa_proof_parse(b, cid, k)          # noqa: E731
    assert parse(data)[0] == ipa.IPA_PROOF_OK
    # a count other than log d1: in l_vec, in r_vec, a proof of another key, a count far beyond the bytes
    at_r = 8 + log_d * g
    assert parse((2).to_bytes(8, "little") + data[8:]) == (ipa.IPA_PROOF_BAD_COUNT, None, None)
    assert parse(data[:at_r] + (4).to_bytes(8, "little") + data[at_r + 8:]) == (ipa.IPA_PROOF_BAD_COUNT, None, None)
    assert parse(data, 4)[0] == ipa.IPA_PROOF_BAD_COUNT and parse(data, 2)[0] == ipa.IPA_PROOF_BAD_COUNT
    assert parse((1 << 63).to_bytes(8, "little") + data[8:])[0] == ipa.IPA_PROOF_BAD_COUNT
    # truncation at every length
    for n in range(len(data)):
        assert parse(data[:n]) == (ipa.IPA_PROOF_TRUNCATED, None, None), n
    assert ipa.ipa_proof_parse(data, cid, log_d, 1)[0] != ipa.IPA_PROOF_OK          # read from the wrong offset
    # an option byte other than None: hiding_comm, rand
    for k in (2, 1):
        bad = bytearray(data)
        bad[-k] = 1
        assert parse(bytes(bad)) == (ipa.IPA_PROOF_BAD_OPTION, None, None)
    # c >= r
    at_c = len(data) - 34
    for c in (cv.r, cv.r + 1, (1 << 256) - 1):
        assert parse(data[:at_c] + c.to_bytes(32, "little") + data[at_c + 32:]) == (ipa.IPA_PROOF_C_NOT_REDUCED, None, None)
    assert parse(data[:at_c] + (cv.r - 1).to_bytes(32, "little") + data[at_c + 32:])[0] == ipa.IPA_PROOF_OK
