"""The device hash maps on keys that collide: lookup.hip's multiset table (ls_insert_table, ls_count_queries, wave_value_leader) and
check.hip's key maps (map_build, map_find).  Random 32-byte values never share a hash, so three paths never ran: lanes of one
wavefront with one hash and different values, a probe chain that wraps from the last slot to slot 0, and a long chain mixed with
duplicates.  The collisions are built on the Python restatement of the hash (tests/edge_values.py), which tests/test_fieldu.py holds
equal to the compiled functions; the expected results come from oracle/bigint_oracle.py and tests/circuit_check_ref.py."""
import random

import numpy as np
import pytest

from ark_plonk_amd import _lib, lookup
from ark_plonk_amd.curves import fr_from_mont, fr_to_mont
from oracle import bigint_oracle as bo
from test_circuit_check_gpu import Circ, identity_sigma
from tests import circuit_check_ref as ref
from tests import edge_values as ev

pytestmark = pytest.mark.gpu


def dev(cid, ints):
    import torch
    return torch.from_numpy(np.ascontiguousarray(fr_to_mont(cid, ints)).view(np.int64).reshape(-1, 4)).cuda()


def back(cid, t):
    return fr_from_mont(cid, t.cpu().numpy().view(np.uint64).reshape(-1, 4)) if t.shape[0] else []


def split_agrees(cid, t_words, f_words, ctx):
    """t and f as stored words: the device halves equal the restatement's"""
    cv = bo.CURVES[cid]
    t, f = [ev.field_value(cv, v) for v in t_words], [ev.field_value(cv, v) for v in f_words]
    assert [int(x) for x in fr_to_mont(cid, t[:1])[0]] == [(t_words[0] >> (64 * k)) & ev.M64 for k in range(4)]   # the word that was hashed
    want1, want2 = bo.combine_split(t, f)
    h1, h2 = lookup.combine_split(dev(cid, t), dev(cid, f), cid, ctx)
    assert back(cid, h1) == want1 and back(cid, h2) == want2


# ---------------------------------------------------------------------------------------------------------------- combine_split
@pytest.mark.parametrize("cid", [0, 1])
def test_colliding_pair_in_one_wavefront(cid, ctx):
    """t = A, B, A, B, ... (130 entries, el_mix(A) == el_mix(B)): every wavefront of the insert holds both values under one hash, so
    the leader election has to compare the values; f queries both, 36 times A and 13 times B, mixed in one wavefront."""
    rng = random.Random(0xC0 + cid)
    a, b = ev.colliding_pair(rng)
    assert ev.el_mix(0, a) == ev.el_mix(0, b)
    t = [a, b] * 65
    f = [a if i % 4 else b for i in range(49)]
    assert (f.count(a), f.count(b)) == (36, 13)
    split_agrees(cid, t, f, ctx)
    split_agrees(cid, [b, a, a] * 40 + [b], [b] * 70 + [a], ctx)                   # the second of the pair first, odd counts


@pytest.mark.parametrize("cid", [0, 1])
def test_many_colliding_pairs_among_duplicates(cid, ctx):
    """16 colliding pairs interleaved with 40 random values, every value several times: n_t = 300 over two workgroups."""
    rng = random.Random(0xC2 + cid)
    pool = [v for _ in range(16) for v in ev.colliding_pair(rng)] + [rng.getrandbits(252) for _ in range(40)]
    assert len(set(pool)) == 72 and len({ev.el_mix(0, v) for v in pool}) == 56
    order = list(range(72))
    rng.shuffle(order)
    t = [pool[order[i % 72]] if i < 144 else pool[rng.randrange(72)] for i in range(300)]
    f = [pool[rng.randrange(72)] for _ in range(211)]
    split_agrees(cid, t, f, ctx)


@pytest.mark.parametrize("cid", [0, 1])
def test_probe_chain_wraps_to_slot_zero(cid, ctx):
    """n_t <= 512, so the table has 1024 slots: eight distinct values whose hash lands on slot 1023 and eight on slot 1022 make one chain
    over slots 1022, 1023, 0, 1, ..., 13 -- with duplicates of its members and a colliding pair inside it.  f queries every member."""
    rng = random.Random(0xC4 + cid)
    last, before = ev.slot_cluster(1023, 1023, 8, ev.el_hash, seed=cid), ev.slot_cluster(1023, 1022, 8, ev.el_hash, seed=cid)
    twin = ev.colliding_partner(last[3], rng)                                    # same hash, so the same home slot
    assert all(ev.el_hash(v) & 1023 == 1023 for v in last + [twin]) and all(ev.el_hash(v) & 1023 == 1022 for v in before)
    chain = [v for pair in zip(last, before) for v in pair] + [twin]
    others = [rng.getrandbits(252) for _ in range(60)]
    t = chain + others[:30] + chain[::-1] + others[30:] + chain[::2]
    assert len(t) <= 512
    f = [v for k, v in enumerate(chain) for _ in range(1 + k % 3)] + others[::7]
    split_agrees(cid, t, f, ctx)
    absent = ev.slot_cluster(1023, 1023, 1, ev.el_hash, seed=7, exclude=chain)[0]   # one more value of the wrapped chain, which t lacks
    cv = bo.CURVES[cid]
    with pytest.raises(lookup.ElementNotIndexed):
        lookup.combine_split(dev(cid, [ev.field_value(cv, v) for v in t]), dev(cid, [ev.field_value(cv, v) for v in chain + [absent]]), cid, ctx)


@pytest.mark.parametrize("cid", [0, 1])
def test_query_that_collides_with_a_table_value_is_not_indexed(cid, ctx):
    cv = bo.CURVES[cid]
    rng = random.Random(0xC6 + cid)
    a, b = ev.colliding_pair(rng)
    t = [rng.getrandbits(252) for _ in range(20)] + [a] + [rng.getrandbits(252) for _ in range(20)]
    split_agrees(cid, t, [a, t[0], a], ctx)
    with pytest.raises(KeyError):
        bo.combine_split(t, [a, b])
    with pytest.raises(lookup.ElementNotIndexed):
        lookup.combine_split(dev(cid, [ev.field_value(cv, v) for v in t]), dev(cid, [ev.field_value(cv, v) for v in (a, b, a)]), cid, ctx)
    split_agrees(cid, t, [a, t[0], a], ctx)                                       # the ctx is as usable as before


# ---------------------------------------------------------------------------------------------------------------- circuit check
@pytest.mark.parametrize("cid", [0, 1])
def test_lookup_map_with_colliding_rows(cid, ctx):
    """W = 4: 256 distinct table rows (capacity 512) that share their first three columns.  Eight fourth columns have a colliding
    partner: four partners are table rows too (two keys, one hash), four are absent.  Eight more rows hash to the last slot, 511, and
    wrap.  A query equal to any table row passes; a query equal to an absent partner fails bit 17 and nothing else."""
    cv = bo.CURVES[cid]
    log_n, n, rows = 10, 1 << 10, 256
    rng = random.Random(0xC8 + cid)
    xyz = [rng.getrandbits(252) for _ in range(3)]
    row_hash = lambda v: ev.key_hash(xyz + [v])  # noqa: E731
    pairs = [ev.colliding_pair(rng) for _ in range(8)]
    assert all(row_hash(a) == row_hash(b) and a != b for a, b in pairs)
    present = [a for a, _ in pairs] + [b for _, b in pairs[:4]]
    absent = [b for _, b in pairs[4:]]
    cluster = ev.slot_cluster(511, 511, 8, row_hash, seed=cid)
    t3 = present + cluster
    while len(t3) < rows:
        v = rng.getrandbits(252)
        if v not in t3 and v not in absent:
            t3.append(v)
    rng.shuffle(t3)
    fv = lambda v: ev.field_value(cv, v)  # noqa: E731
    x, y, z = (fv(v) for v in xyz)
    query = [t3[rng.randrange(rows)] for _ in range(n)]
    hit_rows = {}
    for k, v in enumerate(present + cluster):                                  # every crafted row is queried, at known rows
        query[3 + 5 * k] = v
        hit_rows[3 + 5 * k] = v
    miss_rows = [200 + 64 * k + k for k in range(4)]
    for i, v in zip(miss_rows, absent):
        query[i] = v
    cols = Circ.blank(cid, log_n, rows).cols
    cols.update({("t", 0): [x] * rows, ("t", 1): [y] * rows, ("t", 2): [z] * rows, ("t", 3): [fv(v) for v in t3],
                 ("w", 0): [x] * n, ("w", 1): [y] * n, ("w", 2): [z] * n, ("w", 3): [fv(v) for v in query], ("q", "q_lookup"): [1] * n})
    want = Circ(cid, log_n, cols, rows).agree(ctx)                              # device == definition, all rows and the summary
    assert [i for i, m in enumerate(want) if m] == miss_rows and all(want[i] == 1 << 17 for i in miss_rows)
    assert all(want[i] == 0 for i in hit_rows)


@pytest.mark.parametrize("cid", [0, 1])
def test_copy_map_rejects_a_colliding_sigma_entry(cid, ctx):
    """W = 1: a sigma entry with the full hash of an identity encoding K_w omega^row (or only its slot: a walk down the chain) that
    equals no encoding is a bad sigma entry, like the 5 of test_three_cycle_and_a_bad_sigma_entry -- never a position."""
    cv = bo.CURVES[cid]
    log_n, n = 3, 8
    ident = identity_sigma(cid, log_n)
    keys = {ev.stored_word(cv, ident[k][i]) for k in range(4) for i in range(n)}
    cap_mask = 64 - 1                                                            # capacity = the power of two >= 2 * 4n
    rng = random.Random(0xCA + cid)
    base = Circ.blank(cid, log_n)
    assert base.agree(ctx) == [0] * n
    crafted = []
    for k, i in ((0, 0), (1, 4), (3, 7)):                                        # the full hash of a key
        key = ev.stored_word(cv, ident[k][i])
        partner = ev.colliding_partner(key, rng)
        while partner >= cv.r or partner in keys:
            partner = ev.colliding_partner(key, rng)
        assert ev.key_hash([partner]) == ev.key_hash([key])
        crafted.append((k, i, partner))
    key = ev.stored_word(cv, ident[2][5])                                        # the home slot of a key only
    near = ev.slot_cluster(cap_mask, ev.key_hash([key]) & cap_mask, 2, lambda v: ev.key_hash([v]), seed=cid, exclude=keys)
    crafted += [(2, 5, near[0]), (0, 3, near[1])]
    for k, i, word in crafted:
        bad = base.changed((("s", k), i, ev.field_value(cv, word)))
        with pytest.raises(ref.NotAnEncoding):
            bad.reference()
        with pytest.raises(_lib.ZkError) as e:
            bad.device(ctx)
        assert e.value.code == _lib.ZK_ERR_BAD_ARG, (k, i)
    assert base.agree(ctx) == [0] * n                                            # the ctx is as usable as before
