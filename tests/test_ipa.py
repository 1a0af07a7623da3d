"""CPU side of the inner-product-argument commitment (ark_plonk_amd/ipa.py, ark_plonk_amd/csrc/ipa.hip): the test oracle's two groups
agree byte for byte, its check accepts honest proofs and rejects every single tamper, the transcript's encoding of the point at
infinity, and the key-fold kernel's register budget (gfx950 device code compiled here, no GPU)."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import ipa_oracle as io
from ark_plonk_amd.ipa import IpaProof, transcript_hash
from oracle import bigint_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CURVES = {0: bo.BLS12_381, 1: bo.BN254}


def make_instance(cv, d1, n_polys, seed, deg=None):
    rng = np.random.default_rng(seed)

    def fr():
        return int.from_bytes(rng.bytes(40), "little") % cv.r

    logs = [fr() for _ in range(d1)]
    k_h = fr()
    deg = d1 if deg is None else deg
    polys = [[fr() for _ in range(deg)] for _ in range(n_polys)]
    return logs, k_h, polys, fr(), fr()


def both_groups(cv, logs, k_h, polys, z, chi, digest):
    G = (cv.gx, cv.gy)
    KL = io.KnownLog(cv)
    comms_l = [io.commit(KL, logs, p) for p in polys]
    p_known = io.open_(KL, logs, k_h, polys, comms_l, z, chi, digest)
    GE = io.Generic(cv)
    key = [bo.ec_mul(cv, k, G) for k in logs]
    h = bo.ec_mul(cv, k_h, G)
    comms_g = [io.commit(GE, key, p) for p in polys]
    p_gen = io.open_(GE, key, h, polys, comms_g, z, chi, digest)
    return p_known, p_gen, (KL, comms_l)


@pytest.mark.parametrize("digest", ["blake2b", "blake2s"])
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("d1", [1, 2, 4, 64, 256])
def test_generic_and_known_log_proofs_are_identical(d1, cid, digest):
    cv = CURVES[cid]
    logs, k_h, polys, z, chi = make_instance(cv, d1, 3, 1000 * d1 + 10 * cid + (digest == "blake2s"))
    p_known, p_gen, _ = both_groups(cv, logs, k_h, polys, z, chi, digest)
    assert p_known == p_gen
    assert len(p_gen.l_vec) == d1.bit_length() - 1


@pytest.mark.parametrize("cid", [0, 1])
def test_check_accepts_and_rejects_every_single_tamper(cid):
    cv = CURVES[cid]
    d1, digest = 64, "blake2b"
    logs, k_h, polys, z, chi = make_instance(cv, d1, 3, 77 + cid)
    KL = io.KnownLog(cv)
    comms = [io.commit(KL, logs, p) for p in polys]
    proof = io.open_(KL, logs, k_h, polys, comms, z, chi, digest)
    values = [bo.horner(p, z, cv.r) for p in polys]
    assert io.check(KL, logs, k_h, comms, z, values, proof, chi, digest)
    G = (cv.gx, cv.gy)

    def bumped(p):
        return bo.ec_add(cv, p, G)

    def copy(pr):
        return IpaProof(list(pr.l_vec), list(pr.r_vec), pr.final_comm_key, pr.c)

    for j in range(len(proof.l_vec)):
        t = copy(proof)
        t.l_vec[j] = bumped(t.l_vec[j])
        assert not io.check(KL, logs, k_h, comms, z, values, t, chi, digest), ("L", j)
        t = copy(proof)
        t.r_vec[j] = bumped(t.r_vec[j])
        assert not io.check(KL, logs, k_h, comms, z, values, t, chi, digest), ("R", j)
    t = copy(proof)
    t.c = (t.c + 1) % cv.r
    assert not io.check(KL, logs, k_h, comms, z, values, t, chi, digest)
    t = copy(proof)
    t.final_comm_key = bumped(t.final_comm_key)
    assert not io.check(KL, logs, k_h, comms, z, values, t, chi, digest)
    bad_values = [(values[0] + 1) % cv.r] + values[1:]
    assert not io.check(KL, logs, k_h, comms, z, bad_values, proof, chi, digest)
    bad_comms = [(comms[0] + 1) % cv.r] + comms[1:]
    assert not io.check(KL, logs, k_h, bad_comms, z, values, proof, chi, digest)


@pytest.mark.parametrize("cid", [0, 1])
def test_zero_high_half_gives_an_infinity_l0_encoded_as_specified(cid):
    cv = CURVES[cid]
    d1 = 16
    logs, k_h, polys, z, chi = make_instance(cv, d1, 2, 5 + cid, deg=d1 // 2)
    p_known, p_gen, _ = both_groups(cv, logs, k_h, polys, z, chi, "blake2s")
    assert p_gen.l_vec[0] is None and p_known == p_gen
    # the zero point is (x = 0, y = 1, flag = 1), each coordinate in the base field's byte length
    fl = 48 if cid == 0 else 32
    enc = (0).to_bytes(32, "little") + (0).to_bytes(fl, "little") + (1).to_bytes(fl, "little") + b"\x01"
    exp, i = None, 0
    while exp is None:
        x = int.from_bytes(hashlib.blake2s(enc + i.to_bytes(8, "little")).digest()[:32], "little") & ((1 << cv.r.bit_length()) - 1)
        exp = x if x < cv.r else None
        i += 1
    assert transcript_hash(cv.name, "blake2s", [("fr", 0), ("g1", None)]) == exp


def test_transcript_hash_maps_into_the_field_by_rejection():
    for cv in CURVES.values():
        for d in ("blake2b", "blake2s"):
            vals = {transcript_hash(cv.name, d, [("fr", k)]) for k in range(64)}
            assert len(vals) == 64 and all(0 <= v < cv.r for v in vals)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_fold_kernel_has_no_spills_and_no_scratch():
    src = os.path.join(ROOT, "ark_plonk_amd", "csrc", "ipa.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-pragma-unroll-threshold=1000000", "--cuda-device-only",
           "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=1500).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    folds = {k: v for k, v in kernels.items() if "ipa_fold_key" in k}
    assert len(folds) == 2, sorted(kernels)        # one per curve
    for name, k in kernels.items():
        assert k["VGPRs Spill"] == 0 and k["ScratchSize"] == 0, (name, k)
