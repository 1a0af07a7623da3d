"""The C++ host layer (host/ark_plonk_amd.hpp) driven by a compiled caller: host/example.cpp is built with g++
against libark_plonk_amd.so, run on the GPU, and its outputs are compared with the Python mirror's."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _inputs(n):
    out = np.zeros(4 * n, dtype=np.uint64)
    s = 0x5EED0000
    m = (1 << 64) - 1
    for i in range(4 * n):
        s = (s + 0x9E3779B97F4A7C15) & m
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        out[i] = (z >> 2) if i % 4 == 3 else z
    return out.reshape(n, 4)


def test_cpp_example_matches_python_mirror(tmp_path, ctx):
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib
    exe = str(tmp_path / "example")
    libdir = os.path.join(ROOT, "ark_plonk_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "host"), os.path.join(ROOT, "host", "example.cpp"), "-o", exe,
                        "-L", libdir, "-l:libark_plonk_amd.so", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    log_n = 13
    # a pairing key over (H, [TAU]H) and the opening R = TAU * 3 G of the example's first SRS point L = 3 G, as Montgomery limbs
    from ark_plonk_amd.curves import fq_to_mont, g1_mul, g2_mul, get_curve
    from ark_plonk_amd.pairing import PairingKey
    from tests.conftest import TAU
    cv = get_curve(0)
    tau_h = g2_mul(cv, TAU)
    pairing_limbs = fq_to_mont(cv, [*cv.g2x, *cv.g2y, *tau_h[0], *tau_h[1], *g1_mul(cv, 3 * TAU)]).reshape(-1)
    assert pairing_limbs.size == 60
    run = subprocess.run([exe, str(log_n)] + [f"{int(v):016x}" for v in pairing_limbs], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = dict(ln.split(" ", 1) for ln in run.stdout.strip().splitlines())
    assert lines["roundtrip"] == "ok" and lines["commit_round"] == "ok" and lines["host_batch"] == "ok" and lines["deferred_round"] == "ok"
    assert lines["device_winsums"] == "ok"
    assert lines["residency_cache"] == "ok"
    # zk::PairingKey: a valid and two invalid check_pair, four lanes of check_batch, an unreduced coordinate thrown as ZK_ERR_BAD_ARG;
    # the GT words it printed are PairingKey.gt's in Python
    assert lines["pairing"] == "ok"
    three_g = fq_to_mont(cv, list(g1_mul(cv, 3)))
    key = PairingKey.from_trapdoor(TAU, 0)
    want_gt = key.gt(zk.G1Affine(three_g[0], three_g[1], False, cv.name), 1)
    key.close()
    assert lines["pairing_gt"].split() == [f"{int(v):016x}" for v in want_gt.reshape(-1)]
    n = 1 << log_n
    ev = _inputs(n)
    dom = zk.Radix2EvaluationDomain.new(n, 0, ctx)
    coeffs = dom.ifft(torch.from_numpy(ev.view(np.int64)).cuda())
    c0 = coeffs[0].cpu().numpy().view(np.uint64)
    assert lines["coeff0"].split() == [f"{int(v):016x}" for v in c0]
    ks = np.zeros((n, 4), dtype=np.uint64)
    ks[:, 0] = 3 + 2 * np.arange(n, dtype=np.uint64)
    bases = torch.empty((n, 12), dtype=torch.int64, device="cuda")
    ctx.use_torch_stream()
    _lib.check(_lib.lib().zk_g1_fixed_base_batch_dev(ctx.handle, 0, torch.from_numpy(ks.view(np.int64)).cuda().data_ptr(), n, bases.data_ptr()))
    ck = zk.CommitterKey(bases, 0, ctx)
    cm = ck.commit(coeffs)
    cm_ev = ck.commit(torch.from_numpy(ev.view(np.int64)).cuda())
    ck.close()
    assert lines["commit_x"].split() == [f"{int(v):016x}" for v in cm.x]
    # the C++ Transcript / serialize mirror against the Python one (both over the C ABI) on the same commitments
    from ark_plonk_amd import transcript as tr
    pre = tr.Transcript(b"example", 0)
    pre.circuit_domain_sep(n)
    t = pre.clone()
    for lb, pt in (("w_l", cm), ("w_r", cm_ev), ("w_o", cm), ("w_4", cm_ev)):
        t.append(lb, pt)
    zeta = t.challenge_scalar("zeta")
    assert lines["zeta"].split() == [f"{int(v):016x}" for v in zeta]
    assert bytes(int(b, 16) for b in lines["commit_ser"].split()) == tr.g1_serialize(cm, 0)
