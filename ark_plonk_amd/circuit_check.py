"""Which rows of a circuit does a witness violate?  `check_circuit` runs zk_circuit_check_dev (csrc/check.hip) over a `ProverKey`
and the four wire columns BEFORE a proof is computed: every row gets a 32-bit mask of the constraints it breaks -- the summands of the
gate identities the quotient enforces, one by one, the copy constraints behind sigma, membership of the lookup rows in the table --
and the report names the rows.  The reference's counterpart, `StandardComposer::check_circuit_satisfied` (composer.rs:661-814, feature
`trace`), is serial, stops at the first failing gate and knows arithmetic, logic and range gates only.

`prover.prove(..., check=True)` calls it first and raises `CircuitNotSatisfied` instead of returning proof bytes no verifier accepts."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import check, lib
from .context import check_dev_tensor
from .domain import KIND_FFT

# THE bit assignment (include/ark_plonk_amd.h and DESIGN.md section 6d tabulate the same): BIT_NAMES[b] is bit b of a row's mask
BIT_NAMES = ("arith",
             "range0", "range1", "range2", "range3",
             "logic0", "logic1", "logic2", "logic3", "logic4",
             "fixed0", "fixed1", "fixed2", "fixed3",
             "curve0", "curve1", "curve2",
             "lookup",
             "copy_l", "copy_r", "copy_o", "copy_4")
# the selector columns of zk_circuit_check_args, in the order of prover.SELECTORS
_SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith", "q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add", "q_lookup")


def bit_names(mask: int) -> list:
    return [name for b, name in enumerate(BIT_NAMES) if (int(mask) >> b) & 1]


class CheckReport:
    """ok; mask (device int32 tensor, one word per row); failing_rows; first_row (n when ok); counts (name -> rows with that bit)."""

    def __init__(self, n: int, mask, summary: _lib.CircuitCheckSummary):
        self.n = int(n)
        self.mask = mask
        self.failing_rows = int(summary.failing_rows)
        self.first_row = int(summary.first_row)
        self.first_mask = int(summary.first_mask)
        self.counts = {name: int(summary.bit_count[b]) for b, name in enumerate(BIT_NAMES)}
        self.ok = self.failing_rows == 0

    def rows(self, limit: int | None = 16) -> list:
        """[(row, [names of its set bits])] in ascending row order, at most `limit` of them (None: all)"""
        import torch
        if self.ok:
            return []
        idx = torch.nonzero(self.mask).flatten()
        if limit is not None:
            idx = idx[:limit]
        words = self.mask[idx].cpu().numpy().view(np.uint32)
        return [(int(r), bit_names(w)) for r, w in zip(idx.cpu().tolist(), words.tolist())]

    def __str__(self) -> str:
        if self.ok:
            return f"circuit satisfied ({self.n} rows)"
        shown = self.rows(8)
        lines = [f"circuit NOT satisfied: {self.failing_rows} of {self.n} rows fail"]
        lines += [f"  row {r}: {', '.join(names)}" for r, names in shown]
        if self.failing_rows > len(shown):
            lines.append(f"  ... and {self.failing_rows - len(shown)} more")
        lines.append("  rows per constraint: " + ", ".join(f"{k} {v}" for k, v in self.counts.items() if v))
        return "\n".join(lines)

    __repr__ = __str__


class CircuitNotSatisfied(ValueError):
    def __init__(self, report: CheckReport):
        super().__init__(str(report))
        self.report = report


def check_columns(curve, log_n: int, wires, selector_evals: dict, sigma_evals, table_cols, table_rows: int, pi_evals, coeff_a_mont, coeff_d_mont,
                  ctx, want_mask: bool = True):
    """zk_circuit_check_dev on evaluation columns ((n, 4) Montgomery device tensors): (mask or None, CircuitCheckSummary).
    table_rows <= n rows of the table columns are read; pi_evals may be None."""
    import torch
    n = 1 << log_n
    a = _lib.CircuitCheckArgs()
    cols = {"w_l": wires[0], "w_r": wires[1], "w_o": wires[2], "w_4": wires[3]}
    cols.update({k: selector_evals[k] for k in _SELECTORS})
    if pi_evals is not None:
        cols["pi"] = pi_evals
    for name, t in cols.items():
        if check_dev_tensor(t, 4, ctx.device) != n:
            raise ValueError(f"{name}: {n} rows expected")
        setattr(a, name, t.data_ptr())
    for k in range(4):
        if check_dev_tensor(sigma_evals[k], 4, ctx.device) != n:
            raise ValueError(f"sigma {k}: {n} rows expected")
        a.sigma[k] = sigma_evals[k].data_ptr()
        if table_rows:
            if check_dev_tensor(table_cols[k], 4, ctx.device) < table_rows:
                raise ValueError(f"table column {k}: {table_rows} rows expected")
            a.table[k] = table_cols[k].data_ptr()
    a.table_rows = int(table_rows)
    for dst, src in ((a.coeff_a, coeff_a_mont), (a.coeff_d, coeff_d_mont)):
        for j, v in enumerate(np.asarray(src, dtype=np.uint64).reshape(4)):
            dst[j] = int(v)
    mask = torch.empty(n, dtype=torch.int32, device=wires[0].device) if want_mask else None
    out = _lib.CircuitCheckSummary()
    ctx.use_torch_stream()
    check(lib().zk_circuit_check_dev(ctx.handle, curve.curve_id, log_n, ctypes.addressof(a), None if mask is None else mask.data_ptr(),
                                     ctypes.addressof(out)), "zk_circuit_check_dev")
    return mask, out


def selector_evaluations(pk) -> dict:
    """the twelve selector columns over the domain: q_lookup's as the key holds them, the other eleven as the (exact) NTT of their
    polynomials -- the key does not keep them, and they are dropped after the check"""
    names = [k for k in _SELECTORS if k != "q_lookup"]
    out = dict(zip(names, pk.domain.batch(KIND_FFT, [pk.polys[k] for k in names])))
    out["q_lookup"] = pk.q_lookup_evals
    return out


def check_circuit(pk, wires, public_inputs: dict, coeff_a_mont, coeff_d_mont, selector_evals: dict | None = None, ctx=None) -> CheckReport:
    """pk: a `prover.ProverKey`; wires, public_inputs, coeff_a / coeff_d: as `prover.prove` takes them.  selector_evals: the twelve
    selector columns over the domain when the caller still has them (else the eleven the key lacks are transformed back)."""
    import torch
    d = pk.domain
    n = d.size()
    ctx = ctx or d._ctx_for(wires[0])
    sel = dict(selector_evals) if selector_evals is not None else selector_evaluations(pk)
    pi = None
    if public_inputs:
        pi = torch.zeros((n, 4), dtype=torch.int64, device=wires[0].device)
        for pos, v in public_inputs.items():
            pi[pos] = torch.from_numpy(np.asarray(v, dtype=np.uint64).reshape(4).view(np.int64)).to(pi.device)
    rows = min(int(pk.table_cols[0].shape[0]), n)
    mask, summary = check_columns(d.curve, d.log_size_of_group(), list(wires), sel, pk.sigma_evals, pk.table_cols, rows, pi, coeff_a_mont,
                                  coeff_d_mont, ctx)
    return CheckReport(n, mask, summary)
