"""Build the gfx950 shared library (hipcc, in-tree).  `python -m ark_plonk_amd.build [--force]`.

The heavy kernels are compiled as separate objects -- one per (curve, NTT radix exponent) and four MSM
units per curve (sort / accumulate / reduce / host plan: csrc/msm_common.cuh) -- so a full build
parallelises over the host cores and an edit rebuilds only what it touches.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "obj")
LIB = os.path.join(HERE, "libark_plonk_amd.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -pragma-unroll-threshold: the NTT passes keep 8 field elements per lane in registers and every loop over
# them must fully unroll (a rolled loop indexes the array at run time and sends it to scratch memory)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
         "-mllvm", "-pragma-unroll-threshold=1000000", "-Wpass-failed"]

FIELD_HDRS = ["field_common.cuh", "field.cuh", "fieldu.cuh", "fields.cuh", "curve_params.h", "zk_common.h"]
HOST_HDRS = FIELD_HDRS + ["ecu.cuh", "ctx.h", "g1_host.h", "../../include/ark_plonk_amd.h"]
API_HDRS = HOST_HDRS + ["api_internal.h"]
# helpers with one definition each: Fr / 32-byte element access; bounded lazy arithmetic on the 29-bit Fr type; the MSM's point storage
FR_IO, ZBOUND, POINT_IO = ["fr_io.cuh"], ["fr_io.cuh", "zbound.cuh"], ["point_io.cuh"]
DOMAIN, DEV_SCAN = ["fr_io.cuh", "domain.cuh"], ["dev_scan.cuh"]       # domain and permutation constants; the integer exclusive scan
GADGET = ["gadget_common.cuh"]            # what the two units of the device composer (layout, witness) share
BLOCK_INV = ["block_inverse.cuh"]         # one field inversion per workgroup: the key fold, the gadget witnesses, the verifier's scalars
G1_LIFT = ["g1_lift.cuh"]              # an x to a point of the curve (root, sign rule): the point decoder and the IPA key derivation
PAIRING = ["pairing.cuh", "pairing_params.h"]      # the Fq12 tower, the Miller loop over a line table, the final exponentiation: host and device
REPLAY = ["strobe.cuh", "replay_walk.cuh"]      # merlin's sponge and the verifier's parse + replay of one proof: host (wire) and device (replay)
# the C ABI, one unit per subsystem (api_internal.h is what they share)
API_UNITS = ("api_ctx", "residency", "srs", "commit", "round", "api_host", "api_poly")
MSM_UNITS = ("msm_accumulate", "msm_reduce", "msm_sort", "msm_plan")      # heaviest first


def jobs():
    """(object name, source, extra defines, header deps)"""
    out = [(f"{u}.o", f"{u}.hip", [], API_HDRS + (DOMAIN if u == "api_poly" else [])) for u in API_UNITS] + [
        ("hostio.o", "hostio.hip", [], HOST_HDRS),
        ("wire.o", "wire.hip", [], HOST_HDRS + REPLAY),
        ("kzg.o", "kzg.hip", [], HOST_HDRS + ZBOUND),
        ("lookup.o", "lookup.hip", [], HOST_HDRS + ZBOUND + DEV_SCAN),
        ("grand_product.o", "grand_product.hip", [], HOST_HDRS + DOMAIN),
        ("quotient.o", "quotient.hip", [], HOST_HDRS + ZBOUND + DOMAIN),
        ("quadtest.o", "quadtest.hip", [], HOST_HDRS + ["ecq.cuh"]),
        ("ntt.o", "ntt.hip", [], HOST_HDRS + DOMAIN + ["ntt_pass.cuh"]),
        ("ntt_pass_table.o", "ntt_pass_table.hip", [], []),
        ("msm_dispatch.o", "msm_dispatch.hip", [], HOST_HDRS),
        # the inner-product-argument commitment; circuit compilation (the wire permutation from the variable map, the witness gather);
        # the circuit check (per-row masks of violated gate, copy and lookup constraints)
        ("ipa.o", "ipa.hip", [], API_HDRS + FR_IO + POINT_IO + BLOCK_INV),
        ("compile.o", "compile.hip", [], API_HDRS + DOMAIN + DEV_SCAN),
        ("check.o", "check.hip", [], API_HDRS + ZBOUND + DOMAIN),
        # the device composer: gadget segments (rows, ids, selectors, insertions) and lookup tables, built once per circuit ...
        ("gadget_layout.o", "gadget_layout.hip", [], API_HDRS + FR_IO + GADGET),
        # ... and the values of the variables the segments create, replayed once per proof
        ("gadget_witness.o", "gadget_witness.hip", [], API_HDRS + FR_IO + GADGET + BLOCK_INV),
        # the output of a lookup: the (a, b, d) -> first-row map of a lookup table and its queries (compares 32-byte words: both curves)
        ("lookup_map.o", "lookup_map.hip", [], API_HDRS + FR_IO),
        # the verifier's device side: batch decoding of compressed G1 points, per-proof scalars, the column sum of a fold (its host
        # side, parse and replay, is in wire.hip)
        ("verify.o", "verify.hip", [], API_HDRS + DOMAIN + BLOCK_INV + G1_LIFT),
        # ... and the same parse and replay on the device, one proof per lane
        ("replay.o", "replay.hip", [], API_HDRS + REPLAY),
        # many small MSMs over one set of bases, each as a point: one wavefront per segment
        ("g1_segments.o", "g1_segments.hip", [], API_HDRS + BLOCK_INV),
        # ipa_pc::setup: the committer key's generators hashed to the curve (wave-local candidate search, cofactor clearing)
        ("ipa_setup.o", "ipa_setup.hip", [], API_HDRS + BLOCK_INV + G1_LIFT + ["h2c.cuh"]),
        # the KZG pairing check: prepared G2 keys (host), one check on the host, one check per lane on the device
        ("pairing.o", "pairing.hip", [], API_HDRS + PAIRING),
    ]
    for c in (0, 1):
        # ARK_PLONK_AMD_MSM_FLAGS: extra compiler flags for the MSM objects only (scheduler experiments: tools/ab_bench.sh)
        for unit in MSM_UNITS:
            out.append((f"{unit}_c{c}.o", f"{unit}.hip", [f"-DZK_CURVE_SEL={c}"] + os.environ.get("ARK_PLONK_AMD_MSM_FLAGS", "").split(),
                        HOST_HDRS + POINT_IO + ["msm_common.cuh"] + (["ecq.cuh"] if unit == "msm_reduce" else [])))
        for s in range(3, 10):
            out.append((f"ntt_pass_c{c}_s{s}.o", "ntt_pass_inst.hip", [f"-DZK_CURVE_SEL={c}", f"-DZK_NTT_S={s}"],
                        FIELD_HDRS + ["ntt_pass.cuh"]))
    return out


# What a committed counter file (profiles/pmc_*.json) describes: (source, defines) of the units that hold its kernels, in hash order
PMC_UNITS = {
    "pmc_msm_accumulate.json": [("msm_accumulate.hip", ["-DZK_CURVE_SEL=0"])],
    "pmc_ntt.json": [("ntt.hip", [])] + [("ntt_pass_inst.hip", ["-DZK_CURVE_SEL=0", f"-DZK_NTT_S={s}"]) for s in range(3, 10)],
}


def device_asm(src: str, defs=(), timeout: float = 900) -> str:
    """gfx950 assembly of one unit's device code as the library build compiles it.  `__hip_cuid_<hex>` hashes the command line and
    the path, so it is replaced by a fixed token; nothing else in the text depends on where or when it was compiled."""
    import re
    cmd = [HIPCC] + FLAGS + list(defs) + ["--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", r.stdout)


def device_code_sha256(units, workers: int = 8) -> str:
    """sha256 over the device assembly of `units` ((source, defines) pairs), concatenated in the order given"""
    import hashlib
    with ThreadPoolExecutor(max_workers=workers) as ex:
        texts = list(ex.map(lambda u: device_asm(*u), units))
    return hashlib.sha256("".join(texts).encode()).hexdigest()


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False, workers: int | None = None) -> str:
    os.makedirs(OBJ, exist_ok=True)
    todo = []
    objs = []
    for obj, src, defs, hdrs in jobs():
        o = os.path.join(OBJ, obj)
        objs.append(o)
        deps = [os.path.join(CSRC, src)] + [os.path.join(CSRC, h) for h in hdrs]
        if force or _stale(o, deps):
            todo.append([HIPCC] + FLAGS + defs + ["-c", os.path.join(CSRC, src), "-o", o])
    # heaviest first (large S, MSM) so the tail of the build is short
    todo.sort(key=lambda c: (0 if "/msm_" in " ".join(c[-3:]) else 1, -int(next((d.split("=")[1] for d in c if d.startswith("-DZK_NTT_S=")), 0))))

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
        return r.stderr

    if todo:
        n = workers or min(len(todo), max(1, (os.cpu_count() or 4)))
        with ThreadPoolExecutor(max_workers=n) as ex:
            for err in ex.map(run, todo):
                if verbose and err.strip():
                    print(err, file=sys.stderr)
    if force or todo or _stale(LIB, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd[:6]), "...", flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
