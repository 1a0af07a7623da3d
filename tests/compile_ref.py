"""Helper of tests/test_compile*.py (no test): the wire permutation of plonk-core/src/permutation/mod.rs:101-169 restated from its
definition, twice -- a dict of lists in plain Python, and a numpy form for large n -- and the encoding K * omega^row as integers.

Definition: the variable map holds, per variable, its positions (wire * n + row; wire 0..3 = Left, Right, Output, Fourth) in the order
they were inserted; sigma sends each position to the next one of its variable's list, the last to the first; a position no variable
holds stays where it is."""
import numpy as np

K = (1, 7, 13, 17)          # permutation/constants.rs:12-22


def sigma_dict(n, ins_var, ins_pos):
    sigma = list(range(4 * n))
    lists = {}
    for v, p in zip(ins_var, ins_pos):
        lists.setdefault(int(v), []).append(int(p))
    for lst in lists.values():
        for i, p in enumerate(lst):
            sigma[p] = lst[(i + 1) % len(lst)]
    return sigma


def sigma_numpy(n, ins_var, ins_pos):
    var = np.asarray(ins_var, dtype=np.int64)
    pos = np.asarray(ins_pos, dtype=np.int64)
    sigma = np.arange(4 * n, dtype=np.int64)
    m = var.shape[0]
    if m == 0:
        return sigma
    order = np.argsort(var, kind="stable")              # equal variables keep their insertion order
    sv, sp = var[order], pos[order]
    head = np.ones(m, dtype=bool)
    head[1:] = sv[1:] != sv[:-1]
    start = np.maximum.accumulate(np.where(head, np.arange(m), 0))      # index of the segment head of every element
    last = np.ones(m, dtype=bool)
    last[:-1] = head[1:]
    nxt = np.arange(m) + 1
    nxt[last] = start[last]
    sigma[sp] = sp[nxt]
    return sigma


def canonical_insertions(n, w_l, w_r, w_o, w_4):
    """row by row; Left, Right, Output, Fourth (what add_variables_to_map does per gate)"""
    ins_var, ins_pos = [], []
    for row, ids in enumerate(zip(w_l, w_r, w_o, w_4)):
        for wire, v in enumerate(ids):
            ins_var.append(int(v))
            ins_pos.append(wire * n + row)
    return ins_var, ins_pos


def encode(r, omega, n, sigma):
    """[[K_w' * omega^row' mod r for the n rows of wire w] for w in 0..3]"""
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * omega % r
    return [[K[int(s) // n] * pw[int(s) % n] % r for s in sigma[w * n:(w + 1) * n]] for w in range(4)]


def cycle_count(sigma):
    """cycles of a permutation given as an integer array (pointer doubling: the least label reachable, log n rounds)"""
    s = np.asarray(sigma, dtype=np.int64)
    label = np.arange(s.shape[0], dtype=np.int64)
    jump = s.copy()
    for _ in range(max(1, int(s.shape[0]).bit_length())):
        label = np.minimum(label, label[jump])
        jump = jump[jump]
    return int(np.unique(label).shape[0])
