"""ark_plonk_amd -- MI355X-native NTT + MSM hot path of the ark-plonk prover (HIP, gfx950).

Host-side mirror of the reference interfaces for this path:
  Radix2EvaluationDomain / GeneralEvaluationDomain  <- ark_poly::EvaluationDomain
  VariableBaseMSM, CommitterKey (commit / open)     <- ark_ec::msm::VariableBaseMSM, KZG10 PC::commit/open
  permutation / quotient / lookup / linearisation    <- the O(n) bodies of prover rounds 2-5 (permutation/mod.rs, quotient_poly.rs,
                                                       lookup/multiset.rs, linearisation_poly.rs) on device-resident vectors
  transcript, prover                                 <- merlin + TranscriptProtocol, Proof bytes; Prover::prove_with_preprocessed end to end
All compute runs in libark_plonk_amd.so (C ABI: include/ark_plonk_amd.h); there is no CPU fallback.
"""
from .context import Context, default_context  # noqa: F401
from .curves import BLS12_381, BN254, get_curve  # noqa: F401
from .domain import GeneralEvaluationDomain, Radix2EvaluationDomain  # noqa: F401
from . import linearisation, lookup, permutation, prover, quotient, transcript  # noqa: F401
from . import _lib, msm  # noqa: F401
from . import compile  # noqa: F401  (circuit description -> ProverKey / VerifierKey / seeded transcript)
from .compile import CircuitDescription, VerifierKey, assign  # noqa: F401
from . import circuit_check  # noqa: F401  (which rows of a circuit a witness violates, before the proof)
from .circuit_check import BIT_NAMES, CheckReport, CircuitNotSatisfied, check_circuit  # noqa: F401
from . import composer  # noqa: F401  (gadget circuits and their witnesses, built on the device)
from .composer import Composer  # noqa: F401
from . import verifier  # noqa: F401  (batch verification up to the two pairing inputs)
from .verifier import BatchVerifier, IpaBatchVerifier  # noqa: F401
from . import pairing  # noqa: F401  (the KZG pairing check: a prepared G2 key, one check on the host, B checks on the device)
from .pairing import G2Affine, PairingKey  # noqa: F401
from .msm import (CommitterKey, G1Affine, VariableBaseMSM, kzg_witness, srs_cache_config, segments_msm, srs_cache_stats,  # noqa: F401
                  sum_partials, sum_partials_batch)

__all__ = [
    "Context", "default_context", "BLS12_381", "BN254", "get_curve", "GeneralEvaluationDomain",
    "Radix2EvaluationDomain", "CommitterKey", "G1Affine", "VariableBaseMSM", "kzg_witness", "sum_partials", "sum_partials_batch", "srs_cache_stats", "srs_cache_config", "permutation", "quotient", "lookup", "linearisation", "prover", "transcript",
    "verifier", "BatchVerifier", "IpaBatchVerifier", "segments_msm", "composer", "Composer", "circuit_check", "check_circuit", "CheckReport", "CircuitNotSatisfied", "BIT_NAMES",
    "pairing", "PairingKey", "G2Affine",
]
