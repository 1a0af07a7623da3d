"""Generates tests/golden/reference_prover.json -- what tests/test_rust_shim.py needs to know about the reference tree
(heliaxdev/ark-plonk) that rust-shim/patches/plonk-core-device-prover.patch is written against, so that the tests run
without that tree:

    python tests/golden/gen_golden_reference.py PATH_TO_ARK_PLONK_CHECKOUT

Content:
  * patch_preimage: for every hunk of the patch, the file, the hunk's old range (start, length) and the sha256 of the
    reference's lines in that range -- a hunk applies cleanly exactly when its context and removed lines hash to it;
  * transcript_ops: the sha256 of every (operation, label) pair of `prove_with_preprocessed` (proof_system/prover.rs:163-638),
    in order;
  * appended: the sha256 of the expression each `append` of that body hashes, whitespace removed, in order.
Only digests are stored, nothing of the reference's source.
"""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATCH = os.path.join(ROOT, "rust-shim", "patches", "plonk-core-device-prover.patch")
OUT = os.path.join(ROOT, "tests", "golden", "reference_prover.json")
HUNK = re.compile(r"^@@ -(\d+)(?:,(\d+))? \+\d+(?:,\d+)? @@")


def patch_hunks(patch_text):
    """(file relative to the tree root, old start, old length, old-side lines, new-side lines) of every hunk of a `patch -p1` diff"""
    out, path, cur = [], None, None
    for ln in patch_text.splitlines():
        if ln.startswith("+++ "):
            path = ln.split()[1].split("/", 1)[1]
            continue
        if ln.startswith("--- ") or ln.startswith("diff "):
            continue
        m = HUNK.match(ln)
        if m:
            cur = [path, int(m.group(1)), int(m.group(2) if m.group(2) is not None else 1), [], []]
            out.append(cur)
        elif cur is not None and ln[:1] in (" ", "-", "+"):
            if ln[0] != "+":
                cur[3].append(ln[1:])
            if ln[0] != "-":
                cur[4].append(ln[1:])
    return out


def lines_digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def text_digest(text):
    return hashlib.sha256(text.encode()).hexdigest()


def op_digest(op, label):
    return text_digest(f"{op}:{label}")


def transcript_ops(src):
    src = re.sub(r"//[^\n]*", "", src)
    return [[m.group(1), m.group(2)] for m in re.finditer(r"(append|challenge_scalar)\s*\(\s*b\"([^\"]*)\"", src)]


def appended(src):
    src = re.sub(r"//[^\n]*", "", src)
    return [re.sub(r"\s+", "", m.group(1)) for m in re.finditer(r"append\(\s*b\"[^\"]*\",\s*([^;]*?)\)\s*;", src, flags=re.S)]


def main(ref):
    pre = []
    hunks = patch_hunks(open(PATCH).read())
    for path, start, length, old, _ in hunks:
        ref_lines = open(os.path.join(ref, path)).read().splitlines()
        got = ref_lines[start - 1:start - 1 + length]
        if got != old or len(old) != length:
            sys.exit(f"{path}:{start}: the patch's hunk does not apply to {ref} at its stated position")
        pre.append({"file": path, "old_start": start, "old_len": length, "sha256": lines_digest(got)})
    text = open(os.path.join(ref, "plonk-core", "src", "proof_system", "prover.rs")).read()
    body = text[text.index("pub fn prove_with_preprocessed"):text.index("/// Proves a circuit is satisfied, then clears the witness variables")]
    out = {"reference": "heliaxdev/ark-plonk", "patch": "rust-shim/patches/plonk-core-device-prover.patch", "patch_preimage": pre,
           "transcript_ops": [op_digest(op, label) for op, label in transcript_ops(body)],
           "appended": [text_digest(v) for v in appended(body)]}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(pre)} hunks, {len(out['transcript_ops'])} transcript operations")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
