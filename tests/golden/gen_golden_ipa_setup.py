"""Writes tests/golden/ipa_generators.json from the checker (tests/ipa_setup_ref.py): the first 8 generators of `ipa_pc::setup`'s
rule as this repository states it, compressed (ark-serialize), with the attempts each took, for the two curves and the two digests.
The rule is unpinned against the crate: the file records what the checker gave, so that a later change of either statement shows.

    python tests/golden/gen_golden_ipa_setup.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ipa_setup_ref as ref  # noqa: E402


def main():
    out = {}
    for curve, digest in ref.COMBOS:
        gens = ref.generators(curve, digest, 0, 8)
        out[f"{curve}/{digest}"] = {"attempts": [a for _, _, a, _ in gens], "generators": [ref.compress(curve, p) for _, p, _, _ in gens]}
    with open(os.path.join(HERE, "ipa_generators.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
