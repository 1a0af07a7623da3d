"""CPU side of the IPA key derivation (ark_plonk_amd/ipa.py: generator_preimage, from_random_bytes, sample_generators_host,
IpaUniversalParams; csrc/h2c.cuh on the host): the host statement of `ipa_pc::setup`'s rule against the checker
(tests/ipa_setup_ref.py), the figures a CPU model of the rule gave when the rule was written down, setup's and trim's index arithmetic
with the checker's points standing in for the device, the two Blake2 compressions of the kernel header against hashlib (a stand-alone
program under ASan + UBSan: nothing is loaded into Python under a sanitizer), and the committed fixture.  No GPU."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import ipa_setup_ref as ref
from ark_plonk_amd import ipa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ipa_generators.json")


@pytest.mark.parametrize("curve, digest", ref.COMBOS)
def test_host_rule_equals_the_checker(curve, digest):
    want = ref.generators(curve, digest, 0, 32)
    got = ipa.sample_generators_host(curve, 32, 0, digest)
    assert [(st, p, a) for st, p, a, _ in want] == got
    # ... and digest by digest, rejected ones included
    for i in range(32):
        for j in (None, 0, 1, 2):
            data = ref.HASHES[digest](ipa.generator_preimage(i, j)).digest()
            st, p, _ = ref.from_random_bytes(curve, data)
            assert ipa.from_random_bytes(curve, data) == (st, p)
    # a range that does not start at 0, and a cap: exactly the indices that need more attempts run out
    assert ipa.sample_generators_host(curve, 3, 7, digest) == got[7:10]
    capped = ipa.sample_generators_host(curve, 16, 0, digest, max_tries=3)
    for (st, p, a), (wst, wp, wa, _) in zip(capped, want):
        assert (st, p, a) == ((ref.OK, wp, wa) if wa <= 3 else (ref.EXHAUSTED, None, 3))


def test_preimage_layout():
    assert ipa.generator_preimage(0) == b"PC-DL-2020" + bytes(8)
    assert ipa.generator_preimage(0x0102030405060708, 0x1112131415161718) == b"PC-DL-2020" + bytes(range(8, 0, -1)) + bytes(range(0x18, 0x10, -1))
    assert len(ipa.generator_preimage(5, 0)) == 26 and ipa.generator_preimage(5, 0) != ipa.generator_preimage(5)


def test_from_random_bytes_corner_cases():
    for curve in ("bls12_381", "bn254"):
        cv = ipa.get_curve(curve)
        g = 8 * cv.fq_limbs
        enc = lambda x, flags=0: bytes(a | b for a, b in zip(x.to_bytes(g, "little"), bytes(g - 1) + bytes([flags << 6])))
        cases = [b"", b"\x01", bytes(g - 1), enc(0), enc(0) + b"\xff", bytes(range(64)), enc(0, 1), enc(1, 1), enc(0, 3), enc(5, 3),
                 enc(cv.q - 1), enc(cv.q), enc(cv.q + 1), enc(cv.q, 3), enc(2), enc(2, 2), enc(3), enc(3, 2)]
        if curve == "bls12_381":
            cases += [bytes(a | b for a, b in zip(enc(3), bytes(g - 1) + b"\x20")), bytes(a | b for a, b in zip(enc(2, 2), bytes(g - 1) + b"\x20"))]
        seen = set()
        for data in cases:
            st, p, _ = ref.from_random_bytes(curve, data)
            assert ipa.from_random_bytes(curve, data) == (st, p), data.hex()
            seen.add(st)
        assert seen == {ref.OK, ref.BAD_FLAGS, ref.X_NOT_REDUCED, ref.NOT_ON_CURVE, ref.INF_FLAG_X_NONZERO}
        assert ipa.from_random_bytes(curve, enc(0, 1)) == (ref.OK, None)
        assert ipa.from_random_bytes(curve, enc(cv.q, 3))[0] == ref.X_NOT_REDUCED          # the field element is read before the flags
    # bit 381 of a BLS12-381 buffer is cleared, not rejected
    x = next(x for x in range(2, 50) if ref.from_random_bytes("bls12_381", x.to_bytes(48, "little"))[0] == ref.OK)
    plain = ipa.from_random_bytes("bls12_381", x.to_bytes(48, "little"))
    assert plain[0] == ref.OK and ipa.from_random_bytes("bls12_381", (x | 1 << 381).to_bytes(48, "little")) == plain
    # both signs
    lo, hi = plain[1], ipa.from_random_bytes("bls12_381", (x | 1 << 383).to_bytes(48, "little"))[1]
    q = ipa.get_curve("bls12_381").q
    assert lo[0] == hi[0] == x and lo[1] + hi[1] == q and lo[1] < hi[1]


# What a CPU model of the rule gave when it was written down (hashlib + oracle.bigint_oracle): a cross-check that this implementation
# reads the rule as it was meant, not reference output -- the crate itself is unpinned.
MODEL_ATTEMPTS = {
    ("bls12_381", "blake2s"): [1, 7, 1, 1, 4, 1, 2, 2, 5, 1, 3, 1, 3, 2, 2, 4],
    ("bls12_381", "blake2b"): [12, 1, 7, 1, 8, 10, 2, 2, 13, 14, 1, 3, 7, 1, 3, 7],
    ("bn254", "blake2s"): [1, 4, 2, 6, 4, 1, 2, 2, 3, 1, 2, 4, 7, 16, 3, 1],
    ("bn254", "blake2b"): [8, 8, 3, 10, 18, 7, 12, 7, 4, 13, 2, 1, 2, 5, 3, 3],
}
MODEL_MAX_200 = {("bls12_381", "blake2s"): 10, ("bls12_381", "blake2b"): 24, ("bn254", "blake2s"): 27, ("bn254", "blake2b"): 39}


@pytest.mark.parametrize("curve, digest", ref.COMBOS)
def test_cross_check_values_of_the_model(curve, digest):
    assert [a for _, _, a in ipa.sample_generators_host(curve, 16, 0, digest)] == MODEL_ATTEMPTS[(curve, digest)]
    assert sum(MODEL_ATTEMPTS[(curve, digest)]) == {"bls12_381blake2s": 40, "bls12_381blake2b": 92, "bn254blake2s": 59, "bn254blake2b": 106}[curve + digest]
    counts = [ref.attempts_only(curve, digest, i) for i in range(200)]
    assert max(a for a, _ in counts) == MODEL_MAX_200[(curve, digest)]
    assert 2.0 <= round(sum(a for a, _ in counts) / 200, 1) <= 5.7          # the model's figures, to the digit it gave them
    assert 1.965 <= sum(r for _, r in counts) / 200 <= 2.015
    if (curve, digest) == ("bn254", "blake2b"):
        assert counts[59][0] == 39


def test_generator_zero_of_the_model():
    g = ipa.sample_generators_host("bls12_381", 1, 0, "blake2s")[0][1]
    assert g[0] == 0x42c14781e984336f37bd354e00046b65036ee2b8bdde85be742532946f75f58547224195f2f8b3be914aae06b95ce33
    assert ipa.sample_generators_host("bn254", 1, 0, "blake2s")[0][1] == (
        0x2f9148d2289dc60a28411faf7e6c9d6ea7eaf813934cd3f54219513a797d6e30, 0x26d938cd6309eaabc4f9c1ba6950aa8ce0b119cad38b2ba31a2d111ca40efffd)
    # the cofactor did its work: the BLS12-381 generator is in the r-torsion, and is not the hashed point itself
    bls = ref.bo.CURVES["bls12_381"]
    assert ref.bo.ec_mul(bls, bls.r, g) is ref.bo.INF
    st, p = ipa.from_random_bytes("bls12_381", hashlib.blake2s(ipa.generator_preimage(0)).digest())
    assert st == ref.OK and p != g and ref.bo.ec_mul(bls, bls.r, p) is not ref.bo.INF


@pytest.mark.parametrize("max_degree", [0, 1, 2, 6, 7, 8])
def test_setup_and_trim_index_arithmetic(max_degree):
    curve, digest = "bn254", "blake2s"
    d, n_gens, h_at, s_at = ref.setup_layout(max_degree)
    assert (d + 1) & d == 0 and d >= max_degree and (d + 1) // 2 <= max(max_degree, 1)
    pts = [p for _, p, _, _ in ref.generators(curve, digest, 0, n_gens)]
    pp = ipa.IpaUniversalParams(curve, max_degree, pts, digest=digest)
    assert pp.max_degree == d and pp.h == pts[h_at] == pts[-1] and pp.s == pts[s_at] == pts[-2]
    assert pp.comm_key == pts[:d + 1] and len(pp.comm_key) == d + 1
    for supported in range(0, 20):
        want = ref.trim_points(d, supported)
        if want is None:
            with pytest.raises(ValueError):
                pp.trim_size(supported)
            with pytest.raises(ValueError):
                pp.trim(supported)
        else:
            assert pp.trim_size(supported) == want and want & (want - 1) == 0 and supported < want <= d + 1
    with pytest.raises(ValueError):
        ipa.IpaUniversalParams(curve, max_degree, pts[:-1], digest=digest)


def test_blake2_of_the_kernel_header_on_the_host(tmp_path):
    """csrc/h2c.cuh's two compressions, compiled for the host with ASan + UBSan, against hashlib -- on the message lengths a preimage
    can have and around them, on the all-ones message, and through the entry the kernel calls"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "blake2_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "ark_plonk_amd", "csrc"),
           "-x", "c++", os.path.join(ROOT, "tests", "native", "blake2_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "blake2_check ok" in run.stdout and "runtime error" not in run.stderr, (run.stdout + run.stderr)[-3000:]
    plain, gens = [], []
    for line in run.stdout.splitlines()[:-1]:
        f = line.split(" ")
        if f[1] == "generator":
            i, attempt = int(f[2]), int(f[3])
            want = ref.HASHES[f[0]](ipa.generator_preimage(i, None if attempt == 0 else attempt - 1)).digest()
            assert bytes.fromhex(f[4]) == want + bytes(64 - len(want)), line
            gens.append((f[0], i, attempt))
        else:
            msg = bytes.fromhex(f[1])
            assert f[2] == ref.HASHES[f[0]](msg).hexdigest(), line
            plain.append((f[0], msg))
    counting = bytes(range(26))
    assert plain == [(h, m) for m in [counting[:k] for k in (0, 1, 10, 18, 26)] + [b"\xff" * 26] for h in ("blake2s", "blake2b")]
    assert gens == [(h, i, a) for i, a in ((0, 0), (1, 3), (2 ** 32 + 5, 40)) for h in ("blake2s", "blake2b")]
    shutil.rmtree(tmp_path, ignore_errors=True)


def test_fixture_of_the_first_generators():
    """tests/golden/ipa_generators.json (written by tests/golden/gen_golden_ipa_setup.py from the checker): the first 8 generators and
    attempt counts per curve and digest, compressed -- what the host functions give today must be what they gave when it was written"""
    gold = json.load(open(GOLDEN))
    assert sorted(gold) == sorted(f"{c}/{d}" for c, d in ref.COMBOS)
    for curve, digest in ref.COMBOS:
        rec = gold[f"{curve}/{digest}"]
        got = ipa.sample_generators_host(curve, 8, 0, digest)
        assert rec["attempts"] == [a for _, _, a in got]
        assert rec["generators"] == [ipa.g1_compress(curve, p).hex() for _, p, _ in got]
        assert rec["generators"] == [ref.compress(curve, p) for _, p, _, _ in ref.generators(curve, digest, 0, 8)]
