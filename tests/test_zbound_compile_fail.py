"""The rules of csrc/zbound.cuh are static_asserts: a formula that breaks one must not compile.  Each case here is one translation
unit over the host build of the header (as tests/native/fu_check.cpp includes it), one line past a rule, and the host compiler has to
refuse it with that rule's own message; the same line inside the rule compiles, so the refusal is the rule's and not the harness's.
What this guards: the KZG and lookup kernels (kzg.hip, lookup.hip) hold their bounds in these types only.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ark_plonk_amd", "csrc")

PRELUDE = """
#include <cstdint>
#include <cstring>
#include "curve_params.h"
#include "field.cuh"
#include "fieldu.cuh"
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
#include "fr_io.cuh"
#include "zbound.cuh"
typedef Fu<FrBls12_381UParams> F;
static uint4 buf[3];
"""

# name: (the rule's message, a body that keeps the rule, the same body one step past it)
CASES = {
    "sum_of_33_terms": ("sum too large for the 261-bit container",
                        "typedef ZRun<F, 0, 20, 32> S; S::T a(F::zero()); a = S::step(a, Z<F, 20>(F::one()));",
                        "typedef ZRun<F, 0, 20, 33> S; S::T a(F::zero()); a = S::step(a, Z<F, 20>(F::one()));"),
    "product_past_6400": ("Montgomery product operands too large",
                          "Z<F, 640> a(F::zero()); Z<F, 10> b(F::one()); Z<F, 20> c = a * b; (void)c;",
                          "Z<F, 641> a(F::zero()); Z<F, 10> b(F::one()); Z<F, 20> c = a * b; (void)c;"),
    "wider_store_into_narrower_buffer": ("bound would shrink",
                                         "typedef Z<F, 30> Buf; st_z<Buf>(buf, 0, Z<F, 30>(F::zero()));",
                                         "typedef Z<F, 30> Buf; st_z<Buf>(buf, 0, Z<F, 50>(F::zero()));"),
    "subtrahend_above_16r": ("subtrahend above 16r",
                             "Z<F, 10> a(F::one()); Z<F, 160> b(F::zero()); auto c = a - b; (void)c;",
                             "Z<F, 10> a(F::one()); Z<F, 161> b(F::zero()); auto c = a - b; (void)c;"),
}


def compile_unit(tmp_path, name, body):
    src = tmp_path / f"{name}.cpp"
    src.write_text(PRELUDE + "void unit() { " + body + " }\n")
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True, text=True, timeout=300)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
@pytest.mark.parametrize("name", sorted(CASES))
def test_formula_past_a_rule_does_not_compile(name, tmp_path):
    message, inside, past = CASES[name]
    ok = compile_unit(tmp_path, name + "_inside", inside)
    assert ok.returncode == 0, ok.stderr[-2000:]
    bad = compile_unit(tmp_path, name + "_past", past)
    assert bad.returncode != 0 and "static assertion failed" in bad.stderr and message in bad.stderr, bad.stderr[-2000:]
