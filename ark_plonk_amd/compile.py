"""`Circuit::compile` (circuit.rs:226-259 -> proof_system/preprocess.rs:126-423, lookup/preprocess.rs:42-69) on the device: from what a
circuit builder produces -- per gate four VARIABLE INDICES and twelve selector values, the variable map's insertion list, the lookup
table, the public-input rows -- to the `ProverKey` `prover.prove` takes, the `VerifierKey` and the seeded transcript; and the witness
step `to_scalars` (prover.rs:188-192) as `assign`.

    padding (preprocess.rs:61-88, lookup/multiset.rs:70-79)        torch copies
    sigma evaluations (permutation/mod.rs:101-169)                 zk_perm_sigma_dev   (csrc/compile.hip)
    16 + 4 iffts, 16 coset ffts over 4n (preprocess.rs:138-349)    ProverKey (zk_ntt_dev)
    16 + 4 commitments (preprocess.rs:351-374, lookup :63-64)      two deferred rounds on the ctx (a round holds at most 16 jobs)
    VerifierKey::seed_transcript (widget/mod.rs:252-278)           transcript.seed_transcript

Variable 0 is the composer's `zero_var` (composer.rs:308): padding rows point at it.  The circuit builder itself (who produces the
ids and the selector values) is not part of the library."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import ZkError, check, lib
from .context import check_dev_tensor, ptr_of
from .curves import get_curve
from .domain import Radix2EvaluationDomain
from .msm import G1Affine
from .prover import SELECTORS, ProverKey
from .transcript import Transcript, g1_deserialize, g1_serialize, seed_transcript

# field order of the derived CanonicalSerialize of `VerifierKey` (widget/mod.rs:148-176, arithmetic.rs:94-118, lookup.rs:215-229)
VK_FIELDS = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith", "q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add",
             "left_sigma", "right_sigma", "out_sigma", "fourth_sigma", "q_lookup", "table_1", "table_2", "table_3", "table_4")
SIGMA_NAMES = ("left_sigma", "right_sigma", "out_sigma", "fourth_sigma")


def _ids(x, device):
    """u32 ids / positions as a contiguous int32 device tensor (the kernels read the bits as unsigned)"""
    import torch
    if not type(x).__module__.startswith("torch"):
        x = torch.from_numpy(np.ascontiguousarray(x).astype(np.int64))
    return x.to(device=device, dtype=torch.int32).contiguous()


def padded_size(n_gates: int, table_rows: int = 0) -> int:
    """`circuit_bound` (composer.rs:131-138): the next power of two >= max(gates, table rows)"""
    return 1 << max(max(int(n_gates), int(table_rows), 1) - 1, 0).bit_length()


@dataclass
class CircuitDescription:
    n_gates: int
    selectors: dict                 # prover.SELECTORS name -> (n_gates, 4) Montgomery rows, device
    wires: list                     # w_l, w_r, w_o, w_4: variable ids, n_gates each (int32 device tensors)
    num_vars: int
    ins_var: object                 # the calls of add_variable_to_map in call order: variable ...
    ins_pos: object                 # ... and position = wire * n + row with n = size() (the PADDED size)
    table_cols: list = field(default_factory=list)      # up to four (rows, 4) Montgomery columns
    public_inputs: dict = field(default_factory=dict)   # row -> 4 Montgomery limbs
    curve: object = "bls12_381"

    def size(self) -> int:
        rows = max([int(t.shape[0]) for t in self.table_cols], default=0)
        return padded_size(self.n_gates, rows)

    @classmethod
    def from_gates(cls, selectors: dict, w_l, w_r, w_o, w_4, num_vars: int, table_cols=(), public_inputs=None, curve="bls12_381",
                   device="cuda"):
        """The insertion list in the canonical order -- row by row; Left, Right, Output, Fourth -- for circuits without gates that
        map a cell of another row (logic.rs:212-218) or leave one unmapped."""
        import torch
        wires = [_ids(w, device) for w in (w_l, w_r, w_o, w_4)]
        g = int(wires[0].numel())
        rows = max([int(t.shape[0]) for t in table_cols], default=0)
        n = padded_size(g, rows)
        row = torch.arange(g, device=wires[0].device, dtype=torch.int64)
        ins_pos = torch.stack([row + w * n for w in range(4)], dim=1).reshape(-1).to(torch.int32).contiguous()
        ins_var = torch.stack(wires, dim=1).reshape(-1).contiguous()
        return cls(g, dict(selectors), wires, int(num_vars), ins_var, ins_pos, list(table_cols), dict(public_inputs or {}), curve)


def sigma_evals(domain: Radix2EvaluationDomain, ins_var, ins_pos, num_vars: int, ctx=None, positions: bool = False):
    """zk_perm_sigma_dev: the four sigma evaluation vectors over `domain` (and, with positions=True, sigma as u32[4n]) from the
    variable map's insertion list."""
    import torch
    n = domain.size()
    dev = ins_var.device if type(ins_var).__module__.startswith("torch") else "cuda"
    ins_var, ins_pos = _ids(ins_var, dev), _ids(ins_pos, dev)
    ctx = ctx or domain._ctx_for(ins_var)
    if ins_var.numel() != ins_pos.numel():
        raise ValueError("one position per inserted variable expected")
    out = [torch.empty((n, 4), dtype=torch.int64, device=ins_var.device) for _ in range(4)]
    pos = torch.empty(4 * n, dtype=torch.int32, device=ins_var.device) if positions else None
    ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in out])
    ctx.use_torch_stream()
    check(lib().zk_perm_sigma_dev(ctx.handle, domain.curve.curve_id, domain.log_size_of_group(), ptr_of(ins_var), ptr_of(ins_pos),
                                  ins_var.numel(), int(num_vars), None if pos is None else ptr_of(pos), ptrs), "zk_perm_sigma_dev")
    return (out, pos) if positions else out


def gather(values, index, curve="bls12_381", ctx=None):
    """zk_fr_gather_dev: out[i] = values[index[i]] ((num_values, 4) Montgomery rows, u32 indices; all on the device)"""
    import torch
    from .context import default_context
    cv = get_curve(curve)
    ctx = ctx or default_context(values.device.index)
    nv = check_dev_tensor(values, 4, ctx.device)
    index = _ids(index, values.device)
    out = torch.empty((index.numel(), 4), dtype=torch.int64, device=values.device)
    ctx.use_torch_stream()
    check(lib().zk_fr_gather_dev(ctx.handle, cv.curve_id, ptr_of(values), nv, ptr_of(index), index.numel(), ptr_of(out)), "zk_fr_gather_dev")
    return out


class VerifierKey(dict):
    """`VerifierKey` (widget/mod.rs:148-176): the padded size n and the 20 commitments, name -> G1Affine -- the dict
    `ProverKey.verifier_key` returns, so `transcript.seed_transcript` takes it unchanged."""

    def __init__(self, n: int, points: dict, curve="bls12_381"):
        if set(points) != set(VK_FIELDS):
            raise ValueError("the 20 commitments of a verifier key expected")
        super().__init__(points)
        self.n = int(n)
        self.curve = get_curve(curve)

    def seed(self, t: Transcript) -> Transcript:
        return seed_transcript(t, self, self.n)

    def to_bytes(self) -> bytes:
        return self.n.to_bytes(8, "little") + b"".join(g1_serialize(self[k], self.curve) for k in VK_FIELDS)

    @classmethod
    def from_bytes(cls, data: bytes, curve="bls12_381") -> "VerifierKey":
        cv = get_curve(curve)
        sz = lib().zk_g1_compressed_size(cv.curve_id)
        if len(data) != 8 + len(VK_FIELDS) * sz:
            raise ValueError("wrong length")
        pts = {k: g1_deserialize(data[8 + i * sz:8 + (i + 1) * sz], cv) for i, k in enumerate(VK_FIELDS)}
        return cls(int.from_bytes(data[:8], "little"), pts, cv)


def _pad_rows(t, n: int, fill_first: bool):
    import torch
    rows = int(t.shape[0])
    if rows == n:
        return t.contiguous()
    out = torch.zeros((n, 4), dtype=torch.int64, device=t.device)
    out[:rows] = t
    if fill_first and rows:
        out[rows:] = t[0]
    return out


def padded_wire_ids(desc: CircuitDescription):
    """the four id columns padded to size() with variable 0 (preprocess.rs:82-85)"""
    import torch
    n = desc.size()
    out = []
    for w in desc.wires:
        p = torch.zeros(n, dtype=torch.int32, device=w.device)
        p[: w.numel()] = w
        out.append(p)
    return out


def compile(desc: CircuitDescription, ck, transcript_label=b"plonk", curve=None, ctx=None):  # noqa: A001  (the reference's name)
    """-> (ProverKey, VerifierKey, Transcript seeded with the key and the padded size)."""
    cv = get_curve(curve if curve is not None else desc.curve)
    ctx = ctx or ck.ctx
    if ck.round_pending():
        raise RuntimeError("a deferred round is open on this ctx: close it (round_end) before compile")
    if set(desc.selectors) != set(SELECTORS) or len(desc.wires) != 4 or len(desc.table_cols) > 4:
        raise ValueError("12 selector columns, 4 wire id columns and at most 4 table columns expected")
    n = desc.size()
    domain = Radix2EvaluationDomain.new(n, cv, ctx)
    domain_4n = Radix2EvaluationDomain.new(4 * n, cv, ctx)
    if domain is None or domain_4n is None:
        raise ZkError(_lib.ZK_ERR_DOMAIN_TOO_LARGE, "compile")
    dev = desc.wires[0].device
    sel = {}
    for name in SELECTORS:
        if check_dev_tensor(desc.selectors[name], 4, ctx.device) != desc.n_gates:
            raise ValueError(f"selector {name}: n_gates rows expected")
        sel[name] = _pad_rows(desc.selectors[name], n, False)
    import torch
    table = [_pad_rows(desc.table_cols[k], n, True) if k < len(desc.table_cols) else torch.zeros((n, 4), dtype=torch.int64, device=dev)
             for k in range(4)]
    sig = sigma_evals(domain, desc.ins_var, desc.ins_pos, desc.num_vars, ctx)
    pk = ProverKey(domain, domain_4n, sel, sig, table)
    # the reference's two PC::commit calls (preprocess.rs:351-374: 16 polynomials; lookup/preprocess.rs:63-64: 4), each one deferred round
    try:
        ck.commit_begin([pk.polys[k] for k in SELECTORS] + list(pk.sigma_polys))
        first = ck.round_end(16)
        ck.commit_begin(domain.batch(1, pk.table_cols))
        tables = ck.round_end(4)
    except BaseException:
        try:
            if ck.round_pending():
                ck.round_abort()
        except Exception:
            pass
        raise
    pts = dict(zip(list(SELECTORS) + list(SIGMA_NAMES), first))
    pts.update({f"table_{k + 1}": tables[k] for k in range(4)})
    vk = VerifierKey(n, pts, cv)
    return pk, vk, vk.seed(Transcript(transcript_label, cv))


def assign(desc: CircuitDescription, values, ctx=None):
    """`to_scalars` (prover.rs:188-192): the four wire columns `prover.prove` takes, values[(padded) id columns].  values: (num_vars, 4)
    Montgomery rows on the device; values[0] must be zero (variable 0 is the zero variable every padding row points at)."""
    if int(values.shape[0]) != desc.num_vars:
        raise ValueError("one value per variable expected")
    if values[0].cpu().numpy().any():
        raise ValueError("variable 0 is the zero variable: its value must be zero")
    return [gather(values, w, desc.curve, ctx) for w in padded_wire_ids(desc)]
