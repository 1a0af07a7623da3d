"""rust-shim/ cannot be compiled in this pipeline (no cargo / rustc).  What can be checked on the CPU: the `extern "C"` block of
plonk-gpu-sys says what include/ark_plonk_amd.h says (name, arity, pointer / integer widths of every parameter and of the
return value), it is the generator's current output, every library symbol is exported, and every `sys::zk_*` call of the
hand-written crate exists with the right number of arguments.  Reference interface mirrored: plonk-core/src/commitment.rs:8-49,
proof_system/prover.rs:32-37, circuit.rs:264-287."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ark_plonk_amd.h")
SYS_RS = os.path.join(ROOT, "rust-shim", "plonk-gpu-sys", "src", "lib.rs")
SHIM_SRC = os.path.join(ROOT, "rust-shim", "plonk-gpu", "src")


def _c_class(ctype: str) -> str:
    """width class of a C parameter type, derived independently of tools/gen_rust_ffi.py"""
    t = ctype.replace("const", " ").replace("[4]", "*").replace("[]", "*")
    depth = t.count("*")
    base = t.replace("*", " ").split()[0]
    widths = {"int": "i32", "int64_t": "i64", "uint8_t": "u8", "uint32_t": "u32", "uint64_t": "u64", "size_t": "usize", "double": "f64", "char": "i8",
              "void": "void"}
    b = widths.get(base, "struct:" + base)
    return "ptr" * 0 + ("p" * depth + ":" + b if depth else b)


def _rust_class(rtype: str) -> str:
    depth = len(re.findall(r"\*(?:const|mut)", rtype))
    base = re.sub(r"\*(?:const|mut)\s*", "", rtype).strip()
    names = {"c_char": "i8", "c_void": "void", "ZkCtx": "struct:zk_ctx", "ZkSrs": "struct:zk_srs", "ZkTranscript": "struct:zk_transcript",
             "ZkDomainInfo": "struct:zk_domain_info", "ZkQuotientArgs": "struct:zk_quotient_args", "ZkProof": "struct:zk_proof"}
    b = names.get(base, base)
    return "p" * depth + ":" + b if depth else b


def _split_top(s: str):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "([{<":
            depth += 1
        elif ch in ")]}>":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    return [x.strip() for x in out]


def c_prototypes():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for m in re.finditer(r"\n((?:const\s+)?(?:int|void|size_t|char|zk_transcript)\s*\*?\s*)(zk_\w+)\s*\(([^;{]*)\)\s*;", text):
        ret = " ".join(m.group(1).split())
        params = []
        for a in _split_top(" ".join(m.group(3).split())):
            if not a or a == "void":
                continue
            mm = re.match(r"(.*?)(\w+)\s*(\[\d*\])?$", a)
            params.append(_c_class(mm.group(1) + (mm.group(3) or "")))
        protos[m.group(2)] = (None if ret == "void" else _c_class(ret), params)
    return protos


def rust_externs():
    text = open(SYS_RS).read()
    block = text[text.index('extern "C" {'):]
    fns = {}
    for m in re.finditer(r"pub fn (zk_\w+)\((.*?)\)(?:\s*->\s*([^;]+))?;", block):
        params = [_rust_class(p.split(":", 1)[1]) for p in _split_top(m.group(2)) if p]
        fns[m.group(1)] = (None if m.group(3) is None else _rust_class(m.group(3)), params)
    return fns


def test_generated_ffi_is_current():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--stdout"], capture_output=True, text=True, check=True)
    assert out.stdout == open(SYS_RS).read(), "rust-shim/plonk-gpu-sys/src/lib.rs is stale: run python tools/gen_rust_ffi.py"


def test_every_extern_matches_its_c_prototype():
    c, r = c_prototypes(), rust_externs()
    assert len(c) >= 90
    assert set(c) == set(r), (sorted(set(c) - set(r)), sorted(set(r) - set(c)))
    for name in sorted(c):
        assert c[name][0] == r[name][0], (name, "return", c[name][0], r[name][0])
        assert len(c[name][1]) == len(r[name][1]), (name, "arity")
        for k, (a, b) in enumerate(zip(c[name][1], r[name][1])):
            assert a == b, (name, k, a, b)


def test_the_binding_table_of_the_python_mirror_agrees_too():
    """ark_plonk_amd/_lib.py binds the same header by hand (ctypes): same names, same arity."""
    from ark_plonk_amd import _lib
    c = c_prototypes()
    assert set(_lib.SYMBOLS) == set(c), (sorted(set(c) - set(_lib.SYMBOLS)), sorted(set(_lib.SYMBOLS) - set(c)))
    for name, (_, args) in _lib.SYMBOLS.items():
        assert len(args) == len(c[name][1]), name


def test_hand_written_crate_calls_declared_functions_with_the_right_arity():
    fns = rust_externs()
    used = set()
    for fn in sorted(os.listdir(SHIM_SRC)):
        src = open(os.path.join(SHIM_SRC, fn)).read()
        src = re.sub(r"//[^\n]*", "", src)
        assert "..." not in src and "todo!" not in src and "unimplemented!" not in src, fn
        for m in re.finditer(r"sys::(zk_\w+)\s*\(", src):
            name = m.group(1)
            assert name in fns, (fn, name)
            depth, i = 1, m.end()
            while depth:
                depth += {"(": 1, ")": -1}.get(src[i], 0)
                i += 1
            args = _split_top(src[m.end():i - 1])
            assert len(args) == len(fns[name][1]), (fn, name, len(args), len(fns[name][1]))
            used.add(name)
    # the calls the reference's interface needs: trim -> register + table, commit, open, the verifier-side MSM, the four transforms
    assert {"zk_ctx_create", "zk_srs_register", "zk_srs_precompute", "zk_srs_free", "zk_kzg_commit_batch", "zk_kzg_open", "zk_msm_g1",
            "zk_ntt", "zk_strerror"} <= used
    # ... and the device-resident form behind the headline (device.rs): vectors, transforms, blocking and deferred PC calls
    assert {"zk_dev_alloc", "zk_dev_upload", "zk_dev_download", "zk_dev_free", "zk_ntt_dev", "zk_ntt_batch_dev", "zk_kzg_commit_batch_dev",
            "zk_kzg_open_dev", "zk_kzg_round_begin_dev", "zk_kzg_open_begin_dev", "zk_kzg_round_reduce", "zk_kzg_round_end",
            "zk_kzg_round_abort"} <= used
    # ... and the SURVEY.md 8f N1 / N2 entry points with the round-2 / round-5 builders around them
    assert {"zk_perm_product_dev", "zk_lookup_product_dev", "zk_quotient_evals_dev", "zk_poly_evaluate_dev", "zk_poly_lincomb_dev",
            "zk_lookup_query_dev", "zk_lookup_combine_split_dev", "zk_dev_copy"} <= used


PATCH = os.path.join(ROOT, "rust-shim", "patches", "plonk-core-device-prover.patch")
# what the tests need of the reference tree the patch is written against (heliaxdev/ark-plonk): the digest of every hunk's pre-image
# there, and the transcript of its prove_with_preprocessed -- tests/golden/gen_golden_reference.py writes it from a checkout of that tree
REF_GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_prover.json")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def _reference():
    return json.load(open(REF_GOLDEN))


def _added_lines(path_suffix):
    """the '+' lines the patch adds to one file"""
    out, on = [], False
    for ln in open(PATCH).read().splitlines():
        if ln.startswith("+++ "):
            on = ln.split()[1].endswith(path_suffix)
            continue
        if ln.startswith("--- ") or ln.startswith("diff "):
            continue
        if on and ln.startswith("+"):
            out.append(ln[1:])
    return "\n".join(out)


def test_the_prover_patch_applies_to_the_reference():
    """patches/plonk-core-device-prover.patch (commitment.rs: the DeviceBackend hook; error.rs: its error; linearisation_poly.rs:
    compute_on_device; prover.rs: prove_on_device) applies cleanly to the reference tree this repository was built against: every
    hunk's context and removed lines are, at the hunk's own position, the lines the reference has there (their digests, taken from
    that tree, are in tests/golden/reference_prover.json)."""
    import hashlib
    from gen_golden_reference import patch_hunks
    hunks = patch_hunks(open(PATCH).read())
    pre = _reference()["patch_preimage"]
    assert len(hunks) == len(pre) and hunks
    for (path, start, length, old, _), want in zip(hunks, pre):
        assert (path, start, length) == (want["file"], want["old_start"], want["old_len"]), (path, start, length)
        assert len(old) == length, (path, start)
        assert hashlib.sha256("\n".join(old).encode()).hexdigest() == want["sha256"], f"{path}:{start}: the hunk does not apply to the reference"


def _transcript_ops(src):
    """ordered (operation, label) pairs of a prover body: what the transcript hashes, in order"""
    src = re.sub(r"//[^\n]*", "", src)
    return [(m.group(1), m.group(2)) for m in re.finditer(r"(append|challenge_scalar)\s*\(\s*b\"([^\"]*)\"", src)]


def test_the_patched_prover_hashes_what_the_reference_hashes():
    """prove_on_device must leave the transcript byte-identical: the same appends and challenge draws, same labels, same order as
    prove_with_preprocessed (proof_system/prover.rs:163-638).  The patch is parsed; the reference's sequence is known by the digests
    tests/golden/reference_prover.json holds, taken from that source parsed the same way."""
    from gen_golden_reference import op_digest, text_digest
    ref = _reference()
    want = ref["transcript_ops"]
    added = _added_lines("proof_system/prover.rs")
    got = _transcript_ops(added[added.index("fn prove_on_device"):])
    assert len(want) == 53 and [op_digest(op, label) for op, label in got] == want
    # values too: every appended expression names the same quantity (commitments by their role, evaluations by their field)
    def appended(src):
        src = re.sub(r"//[^\n]*", "", src)
        return [re.sub(r"\s+", "", m.group(1)) for m in re.finditer(r"append\(\s*b\"[^\"]*\",\s*([^;]*?)\)\s*;", src, flags=re.S)]
    ref_digests, new_vals = ref["appended"], appended(added[added.index("fn prove_on_device"):])
    assert len(ref_digests) == len(new_vals)
    role = {"w_commits[0].commitment()": "&a_comm", "w_commits[1].commitment()": "&b_comm", "w_commits[2].commitment()": "&c_comm",
            "w_commits[3].commitment()": "&d_comm", "f_poly_commit[0].commitment()": "&f_comm", "h_1_poly_commit[0].commitment()": "&h_1_comm",
            "h_2_poly_commit[0].commitment()": "&h_2_comm", "z_poly_commit[0].commitment()": "&z_comm_round3",
            "t_commits[0].commitment()": "&t_1_comm", "t_commits[1].commitment()": "&t_2_comm", "t_commits[2].commitment()": "&t_3_comm",
            "t_commits[3].commitment()": "&t_4_comm"}
    by_role = {v: k for k, v in role.items()}
    for d, b in zip(ref_digests, new_vals):
        assert text_digest(by_role.get(b, b)) == d, b


def test_device_backend_trait_and_its_gpu_implementation_agree():
    """the trait the patch adds to plonk-core/src/commitment.rs and `impl DeviceBackend<Fr, GpuKZG10> for GpuBackend` (device.rs):
    same methods, same number of parameters; the prover calls nothing else on it."""
    trait_src = _added_lines("commitment.rs")
    trait_src = trait_src[trait_src.index("pub trait DeviceBackend"):]
    impl_src = open(os.path.join(SHIM_SRC, "device.rs")).read()
    impl_src = impl_src[impl_src.index("impl DeviceBackend<Fr, GpuKZG10> for GpuBackend"):]

    def methods(src):
        out = {}
        for m in re.finditer(r"fn (\w+)\s*\(", src):
            depth, i = 1, m.end()
            while depth:
                depth += {"(": 1, ")": -1}.get(src[i], 0)
                i += 1
            out[m.group(1)] = len(_split_top(src[m.end():i - 1]))
        return out
    t, g = methods(trait_src), methods(impl_src)
    assert set(t) == {"upload", "transform_batch", "commit_begin", "open_begin", "round_reduce", "round_end",
                      # round 5: the O(n) steps between the transforms and the commitments (SURVEY.md 8f N1 / N2 and the rounds around them)
                      "resident", "slice", "lincomb", "evaluate", "lookup_query", "combine_split", "permutation_product", "lookup_product", "quotient"}
    assert {k: g.get(k) for k in t} == t
    prover = _added_lines("proof_system/prover.rs")
    lin = _added_lines("proof_system/linearisation_poly.rs")
    called = (set(re.findall(r"\bdev\.(\w+)\(", prover)) | set(re.findall(r"\bdev\.(\w+)\(", lin))) - {"as_ref"}
    assert called <= set(t)
    # ... and every one of the new steps IS called: prove_on_device keeps z, z_2, the quotient, the evaluations and the linearisation
    # polynomial on the device (permutation/mod.rs:652-801, quotient_poly.rs:34-178, linearisation_poly.rs:164-349)
    assert {"resident", "slice", "lincomb", "evaluate", "lookup_query", "combine_split", "permutation_product", "lookup_product", "quotient"} <= called
    # nothing of size n comes back: the patched prover never asks a device vector for a host copy, and never calls the host-side
    # builders whose inputs and outputs are host polynomials
    body = prover[prover.index("fn prove_on_device"):]
    for host_call in ("to_host(", "host_poly(", "compute_permutation_poly(", "compute_lookup_permutation_poly(", "quotient_poly::compute",
                      "linearisation_poly::compute::<", "combine_split(&", "MultiSet::compress("):
        assert host_call not in body, host_call
    # the scheme's side of the hook
    kzg = open(os.path.join(SHIM_SRC, "kzg.rs")).read()
    assert "fn device_backend(ck: &Self::CommitterKey)" in kzg and "GpuBackend::new" in kzg


def test_gpu_kzg10_implements_every_required_method():
    """PolynomialCommitment 0.3's required items + plonk-core's HomomorphicCommitment (commitment.rs:8-19), written out."""
    src = open(os.path.join(SHIM_SRC, "kzg.rs")).read()
    assert "impl PolynomialCommitment<Fr, Poly> for GpuKZG10" in src and "impl HomomorphicCommitment<Fr> for GpuKZG10" in src
    for item in ("type UniversalParams", "type CommitterKey", "type VerifierKey", "type PreparedVerifierKey", "type Commitment",
                 "type PreparedCommitment", "type Randomness", "type Proof", "type BatchProof", "type Error",
                 "fn setup", "fn trim", "fn commit", "fn open<", "fn open_individual_opening_challenges", "fn check<",
                 "fn check_individual_opening_challenges", "fn multi_scalar_mul"):
        assert item in src, item


def test_device_linearisation_batches_what_the_python_prover_batches():
    """`linearisation_poly::compute_on_device` (the patch) and ark_plonk_amd/linearisation.py -- the form the `-m gpu` suite proves
    against the restated verifier -- issue the same 23 evaluations in the same order and the same 19 lincomb terms: the Rust side
    cannot be compiled here, its structure can be read."""
    from ark_plonk_amd import linearisation as lin
    src = _added_lines("proof_system/linearisation_poly.rs")
    src = src[src.index("pub fn compute_on_device"):]
    ev = src[src.index("dev.evaluate(&["):]
    ev = ev[:ev.index("])?;")]
    pairs = re.findall(r"(?:on|at)\(&(?:polys\.)?([\w\[\]\.]+), (zw?)\)", ev)
    rust_name = {"wires[0]": "w_l", "wires[1]": "w_r", "wires[2]": "w_o", "wires[3]": "w_4"}
    names = [(rust_name.get(nm, nm), pt) for nm, pt in pairs]
    assert [nm for nm, pt in names if pt == "z"] == list(lin.EVAL_AT_Z)
    assert [nm for nm, pt in names if pt == "zw"] == list(lin.EVAL_AT_ZW)
    assert len(names) == 23 and [pt for _, pt in names] == ["z"] * 16 + ["zw"] * 7
    lc = src[src.index("dev.lincomb("):]
    lc = lc[:lc.index("\n        ],\n")]
    terms = re.findall(r"(?:on|at)\(&(?:polys\.)?([\w\[\]\.]+),", lc)
    want = ["q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_range", "q_logic", "q_fixed", "q_variable", "z", "fourth_sigma", "q_lookup", "z2", "h1",
            "quotient[0]", "quotient[1]", "quotient[2]", "quotient[3]"]
    assert terms == want


def _strip_rust(src):
    """comments, string / char literals and lifetimes out of Rust source: what is left must have balanced delimiters"""
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r'b?"(?:\\.|[^"\\])*"', '""', src, flags=re.S)
    src = re.sub(r"b?'(?:\\.|[^'\\])'", "''", src)          # char / byte literals ('a', '\n'); lifetimes ('a without a closing quote) stay
    return src


def _balanced(src, what):
    stack = []
    pairs = {")": "(", "]": "[", "}": "{"}
    line = 1
    for ch in src:
        if ch == "\n":
            line += 1
        if ch in "([{":
            stack.append((ch, line))
        elif ch in ")]}":
            assert stack and stack[-1][0] == pairs[ch], f"{what}: unbalanced {ch!r} near line {line} (open: {stack[-1] if stack else None})"
            stack.pop()
    assert not stack, f"{what}: unclosed {stack[-1]}"


def _residue(src, what):
    """(closing, opening) brackets of stripped source that no pair inside it matches; two that mismatch fail the test"""
    pairs = {")": "(", "]": "[", "}": "{"}
    closes, opens = [], []
    for ch in src:
        if ch in "([{":
            opens.append(ch)
        elif ch in ")]}":
            if opens:
                assert opens[-1] == pairs[ch], f"{what}: {ch!r} closes {opens[-1]!r}"
                opens.pop()
            else:
                closes.append(ch)
    return "".join(closes), "".join(opens)


def test_rust_sources_and_patch_have_balanced_delimiters():
    """No compiler here: at least every Rust file of the shim, and every file of plonk-core as the patch leaves it, closes what it
    opens (a dropped brace or parenthesis in 1 000 lines of unbuildable source would otherwise go unnoticed).  The reference's files
    compile, and every hunk's context and removed lines are theirs (test_the_prover_patch_applies_to_the_reference), so a patched
    file is balanced when every hunk's new lines leave unmatched what its old lines leave unmatched -- where the new lines may close
    some of the brackets around the hunk if they reopen the same ones at once (`} impl ... {`)."""
    for root, _, files in os.walk(os.path.join(ROOT, "rust-shim")):
        for fn in files:
            if fn.endswith(".rs"):
                path = os.path.join(root, fn)
                _balanced(_strip_rust(open(path).read()), os.path.relpath(path, ROOT))
    from gen_golden_reference import patch_hunks
    hunks = patch_hunks(open(PATCH).read())
    assert sorted({h[0] for h in hunks}) == sorted(["plonk-core/src/commitment.rs", "plonk-core/src/error.rs", "plonk-core/src/proof_system/prover.rs",
                                                    "plonk-core/src/proof_system/linearisation_poly.rs"])
    reopen = {")": "(", "]": "[", "}": "{"}
    for path, start, _, old, new in hunks:
        what = f"{path} (patched, hunk at line {start})"
        c_old, o_old = _residue(_strip_rust("\n".join(old)), what)
        c_new, o_new = _residue(_strip_rust("\n".join(new)), what)
        assert c_new.startswith(c_old), what
        extra = c_new[len(c_old):]
        assert o_new == "".join(reopen[ch] for ch in reversed(extra)) + o_old, what


def test_patched_prover_declares_what_it_uses():
    """Every `d_*` / `k_*` binding the new prove_on_device reads is introduced by a `let` before its first use, and none is introduced
    twice in one scope level by mistake (a renamed variable is the typical slip of source that never met a compiler)."""
    body = _added_lines("proof_system/prover.rs")
    body = _strip_rust(body[body.index("fn prove_on_device"):])
    declared = {}
    for m in re.finditer(r"\blet\s+(?:mut\s+)?(?:\(([^)]*)\)|(\w+))", body):
        names = [n.strip().lstrip("mut ").strip() for n in (m.group(1).split(",") if m.group(1) else [m.group(2)])]
        for n in names:
            declared.setdefault(n, m.start())
    used = {}
    for m in re.finditer(r"(?<![\.\w])([dk]_[a-z0-9_]+)\b(?!\s*:)", body):       # not a field access, not a struct field name
        used.setdefault(m.group(1), m.start())
    for name, pos in used.items():
        assert name in declared and declared[name] <= pos, f"{name} used at offset {pos} before any `let`"


def test_shim_context_per_thread_option_is_complete():
    """`ARK_PLONK_AMD_CTX_PER_THREAD=1` (T unchanged callers on one card): the per-thread context is created by the
    same function as the process-wide one (so the opt-in caches apply to both), lives in a thread_local whose Drop destroys it, is tried
    once per thread, and the default path still hands out the one process-wide context."""
    src = open(os.path.join(SHIM_SRC, "lib.rs")).read()
    body = src[src.index("fn new_ctx()"):src.index("pub fn layout_checks")]
    assert "zk_ctx_create" in body and "zk_ctx_set_commit_cache" in body and "zk_ctx_set_residency_cache" in body
    assert re.search(r"impl Drop for ThreadCtx \{[^}]*fn drop\(&mut self\) \{[^}]*zk_ctx_destroy", body, re.S)
    assert "thread_local!" in body and "ARK_PLONK_AMD_CTX_PER_THREAD" in body
    ctx_fn = body[body.index("pub fn ctx()"):]
    assert ctx_fn.count("new_ctx()") == 2                       # the process-wide one under the Once, the thread's under its own flag
    assert "t.1.set(true)" in ctx_fn and "unsafe { CTX.0 }" in ctx_fn
    assert src.count("fn new_ctx") == 1 and src.count("zk_ctx_create") == 1
