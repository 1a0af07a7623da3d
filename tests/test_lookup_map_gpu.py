"""GPU suite of the (a, b, d) -> first-row map of a lookup table (csrc/lookup_map.hip: lookup_map_build, lookup_map_query;
zk_lookup_map_slots / _build_dev / _query_dev) and of `LookupTable.lookup` on top of it, against the reference's definition --
`LookupTable::lookup` (lookup/lookup_table.rs:172-180), a scan for the FIRST row whose columns 0, 1 and 3 match (tests/lookup_out_ref.py:
first_match).  Tables and queries are built from STORED words (what the kernels hash and compare; tests/edge_values.py restates the
hash), so colliding keys and probe chains that wrap around the end of the map can be placed on purpose.  Every comparison is exact."""
import ctypes
import random

import numpy as np
import pytest

from ark_plonk_amd import _lib
from ark_plonk_amd.composer import LookupTable
from ark_plonk_amd.curves import fr_from_mont, fr_to_mont, get_curve
from ark_plonk_amd.lookup import ElementNotIndexed
from tests import edge_values as ev
from tests.lookup_out_ref import first_match

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
SENTINEL = (1 << 256) - 1                                   # what an output nobody writes still holds


def dev_words(words):
    """stored words -> (n, 4) int64 device tensor, as they are"""
    import torch
    arr = np.array([[(v >> (64 * k)) & ev.M64 for k in range(4)] for v in words], dtype=np.uint64).reshape(-1, 4)
    return torch.from_numpy(arr.view(np.int64)).cuda()


def host_words(t):
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in t.cpu().numpy().view(np.uint64)]


def dev_u32(vals):
    import torch
    return torch.tensor(list(vals), dtype=torch.int64).to(torch.int32).cuda()


class DevTable:
    """a table of rows (a, b, c, d) of stored words on the device, with its map"""

    def __init__(self, ctx, cid, rows):
        import torch
        self.ctx, self.cid, self.rows = ctx, cid, rows
        self.cols = [dev_words([r[w] for r in rows]) for w in range(4)]
        self.slots = _lib.lib().zk_lookup_map_slots(len(rows))
        self.map = torch.zeros(self.slots, dtype=torch.int32, device="cuda")      # zeros: the build must clear it itself
        ctx.use_torch_stream()
        rc = _lib.lib().zk_lookup_map_build_dev(ctx.handle, cid, self.cols[0].data_ptr(), self.cols[1].data_ptr(), self.cols[3].data_ptr(),
                                                len(rows), self.map.data_ptr(), self.slots)
        assert rc == 0, rc

    def query(self, keys, through_ids=False, seed=0):
        """-> (rc, c words or SENTINEL per query, positions, misses, first miss).  through_ids: the operands come from one value
        vector by index and the outputs go to a permuted, larger vector"""
        import torch
        n = len(keys)
        out_rows = n + 3 if through_ids else n
        out = dev_words([SENTINEL] * out_rows)
        pos = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        keep, op_ids, out_ids, operand_rows = [], None, None, n
        if through_ids:
            rng = random.Random(seed)
            pool = sorted({v for k in keys for v in k}) + [rng.getrandbits(250) for _ in range(5)]
            rng.shuffle(pool)
            values = dev_words(pool)
            idv = [dev_u32([pool.index(k[w]) for k in keys]) for w in range(3)]
            perm = rng.sample(range(out_rows), n)
            oid = dev_u32(perm)
            keep = [values, idv, oid]
            operands, op_ids, out_ids, operand_rows = [values.data_ptr()] * 3, (ctypes.c_void_p * 3)(*[t.data_ptr() for t in idv]), oid.data_ptr(), len(pool)
        else:
            vecs = [dev_words([k[w] for k in keys]) for w in range(3)]
            keep = [vecs]
            operands = [t.data_ptr() for t in vecs]
        misses, first = ctypes.c_uint64(99), ctypes.c_uint64(99)
        self.ctx.use_torch_stream()
        rc = _lib.lib().zk_lookup_map_query_dev(self.ctx.handle, self.cid, (ctypes.c_void_p * 4)(*[c.data_ptr() for c in self.cols]), len(self.rows),
                                                self.map.data_ptr(), self.slots, n, (ctypes.c_void_p * 3)(*operands), op_ids, operand_rows,
                                                out.data_ptr(), out_ids, out_rows, pos.data_ptr(), ctypes.byref(misses), ctypes.byref(first))
        got = host_words(out)
        if through_ids:
            assert all(got[j] == SENTINEL for j in set(range(out_rows)) - set(perm))       # nothing written beside the named places
            got = [got[j] for j in perm]
        del keep
        return rc, got, pos.cpu().numpy().view(np.uint32).tolist(), misses.value, first.value

    def expect(self, keys):
        idx = [first_match(self.rows, *k) for k in keys]
        return [SENTINEL if i is None else self.rows[i][2] for i in idx], [EMPTY if i is None else i for i in idx]

    def check(self, keys, **kw):
        rc, got, pos, misses, first = self.query(keys, **kw)
        want, want_pos = self.expect(keys)
        missing = [i for i, p in enumerate(want_pos) if p == EMPTY]
        assert got == want and pos == want_pos
        assert (rc, misses, first) == ((_lib.ZK_ERR_NOT_INDEXED, len(missing), missing[0]) if missing else (0, 0, len(keys)))


def edge_words(cid):
    cv = get_curve(cid)
    return [0, ev.stored_word(cv, cv.r - 1)]                # the field values 0 and r - 1


def random_table(cid, n_rows, rng):
    """rows over small pools, so that keys repeat (with other c); 0 and r - 1 in every key column"""
    e = edge_words(cid)
    pools = [e + [rng.getrandbits(250) for _ in range(6)] for _ in range(3)]
    return [(rng.choice(pools[0]), rng.choice(pools[1]), rng.getrandbits(250), rng.choice(pools[2])) for _ in range(n_rows)]


def absent_key(rows, rng):
    while True:
        k = (rng.getrandbits(250), rng.getrandbits(250), rng.getrandbits(250))
        if first_match(rows, *k) is None:
            return k


# ---- 1. every table size against the scan, directly and through index vectors
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("n_rows", [0, 1, 2, 63, 64, 65, 257, 300])
def test_map_equals_the_first_match_scan(cid, n_rows, ctx):
    rng = random.Random(1000 * cid + n_rows)
    rows = random_table(cid, n_rows, rng)
    if n_rows >= 63:                                        # the edges as whole keys, each twice with another c
        e = edge_words(cid)
        for j, k in enumerate([(e[0], e[0], e[0]), (e[1], e[1], e[1]), (e[0], e[1], e[0])]):
            rows[10 + j] = (k[0], k[1], rng.getrandbits(250), k[2])
            rows[40 + j] = (k[0], k[1], rng.getrandbits(250), k[2])
    t = DevTable(ctx, cid, rows)
    assert t.slots >= 2 * n_rows
    owners = sorted(set(t.map.cpu().numpy().view(np.uint32).tolist()) - {EMPTY})
    assert owners == sorted({first_match(rows, r[0], r[1], r[3]) for r in rows})          # one slot per distinct key: its first row
    for n in (1, 63, 64, 65, 130):
        keys = [(r[0], r[1], r[3]) for r in (rng.choice(rows) for _ in range(n))] if rows else [absent_key(rows, rng) for _ in range(n)]
        t.check(keys)
        t.check(keys, through_ids=True, seed=n)


# ---- 2. duplicates of a key: the first row wins, wherever its duplicates run
@pytest.mark.parametrize("cid", [0, 1])
def test_first_of_duplicate_keys_wins(cid, ctx):
    rng = random.Random(77 + cid)
    rows = [(rng.getrandbits(250), rng.getrandbits(250), rng.getrandbits(250), rng.getrandbits(250)) for _ in range(300)]
    k1, k2 = absent_key(rows, rng), absent_key(rows, rng)
    for i in (5, 40, 270):                                  # wavefront 0 twice, and the second workgroup
        rows[i] = (k1[0], k1[1], rng.getrandbits(250), k1[2])
    for i in (70, 100, 299):                                # wavefront 1 twice, and the second workgroup
        rows[i] = (k2[0], k2[1], rng.getrandbits(250), k2[2])
    assert len({rows[i][2] for i in (5, 40, 270, 70, 100, 299)}) == 6
    t = DevTable(ctx, cid, rows)
    rc, got, pos, misses, _ = t.query([k1, k2, k1])
    assert (rc, misses) == (0, 0) and pos == [5, 70, 5] and got == [rows[5][2], rows[70][2], rows[5][2]]
    slots = t.map.cpu().numpy().view(np.uint32).tolist()
    assert all(i not in slots for i in (40, 270, 100, 299)) and slots.count(5) == 1 and slots.count(70) == 1


# ---- 3. keys that collide under the hash
@pytest.mark.parametrize("cid", [0, 1])
def test_colliding_keys(cid, ctx):
    rng = random.Random(31 + cid)
    a, b = rng.getrandbits(250), rng.getrandbits(250)
    d1, d2 = ev.colliding_pair(rng)
    a1, a2 = ev.colliding_pair(rng)
    assert ev.key_hash([a, b, d1]) == ev.key_hash([a, b, d2]) and ev.key_hash([a1, b, d1]) == ev.key_hash([a2, b, d1]) and d1 != d2 and a1 != a2
    filler = [(rng.getrandbits(250), rng.getrandbits(250), rng.getrandbits(250), rng.getrandbits(250)) for _ in range(61)]
    both = filler[:30] + [(a, b, 111, d1), (a, b, 222, d2), (a1, b, 333, d1)] + filler[30:]
    t = DevTable(ctx, cid, both)
    t.check([(a, b, d2), (a, b, d1), (a1, b, d1), (a, b, d2)])
    rc, got, pos, misses, first = t.query([(a, b, d1), (a2, b, d1), (a1, b, d1)])          # the partner of a present key is absent
    assert (rc, misses, first) == (_lib.ZK_ERR_NOT_INDEXED, 1, 1) and pos == [30, EMPTY, 32] and got == [111, SENTINEL, 333]
    one = filler[:30] + [(a, b, 111, d1)] + filler[30:]
    t = DevTable(ctx, cid, one)
    t.check([(a, b, d1), (a, b, d2), (a, b, d1)], through_ids=True)
    rc, got, pos, misses, first = t.query([(a, b, d2)])
    assert (rc, misses, first, pos, got) == (_lib.ZK_ERR_NOT_INDEXED, 1, 0, [EMPTY], [SENTINEL])


# ---- 4. probe chains that wrap from the last slot to slot 0
@pytest.mark.parametrize("cid", [0, 1])
def test_chain_wraps_around_the_end_of_the_map(cid, ctx):
    rng = random.Random(55 + cid)
    a, b = rng.getrandbits(250), rng.getrandbits(250)
    h = lambda v: ev.key_hash([a, b, v])  # noqa: E731
    last, before = ev.slot_cluster(1023, 1023, 8, h, seed=cid), ev.slot_cluster(1023, 1022, 8, h, seed=cid)
    chain = last + before
    absent = ev.slot_cluster(1023, 1023, 1, h, seed=7, exclude=chain)[0]
    rows = [(rng.getrandbits(250), rng.getrandbits(250), rng.getrandbits(250), rng.getrandbits(250)) for _ in range(300)]
    for i, d in zip(rng.sample(range(290), 16), chain):
        rows[i] = (a, b, rng.getrandbits(250), d)
    rows[295] = (a, b, rng.getrandbits(250), last[2])       # a duplicate of a chain member behind its first row
    t = DevTable(ctx, cid, rows)
    assert t.slots == 1024
    slots = t.map.cpu().numpy().view(np.uint32).tolist()
    assert all(slots[s] != EMPTY for s in (1022, 1023, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13))      # 16 keys from slot 1022 on
    t.check([(a, b, d) for d in chain] + [(a, b, absent)] + [(a, b, d) for d in reversed(chain)])
    t.check([(a, b, d) for d in chain], through_ids=True)


# ---- 5. misses: alone, between hits, in several wavefronts
@pytest.mark.parametrize("cid", [0, 1])
def test_misses_are_counted_and_located(cid, ctx):
    rng = random.Random(91 + cid)
    rows = random_table(cid, 257, rng)
    t = DevTable(ctx, cid, rows)

    def hit():
        r = rng.choice(rows)
        return r[0], r[1], r[3]
    t.check([absent_key(rows, rng)])
    t.check([absent_key(rows, rng) for _ in range(130)], through_ids=True)
    for missing in ([129], [64], [3, 4, 63, 64, 65, 128], [77, 0]):
        keys = [hit() for _ in range(130)]
        for i in missing:
            keys[i] = absent_key(rows, rng)
        t.check(keys)
        t.check(keys, through_ids=True, seed=missing[0])
    # a key that shares a and b with a row but not d, and one that shares b and d but not a
    r = rows[100]
    t.check([(r[0], r[1], r[3] ^ 1), (r[0] ^ 1, r[1], r[3]), (r[0], r[1], r[3])])
    t.check([hit() for _ in range(65)])                     # the ctx and the map are as good as before


# ---- 6. refusals: codes, not crashes
@pytest.mark.parametrize("cid", [0, 1])
def test_refusals(cid, ctx):
    import torch
    L = _lib.lib()
    rng = random.Random(3 + cid)
    rows = random_table(cid, 65, rng)
    t = DevTable(ctx, cid, rows)
    cols = (ctypes.c_void_p * 4)(*[c.data_ptr() for c in t.cols])
    keys = [(r[0], r[1], r[3]) for r in rows[:10]]
    vecs = [dev_words([k[w] for k in keys]) for w in range(3)]
    ops = (ctypes.c_void_p * 3)(*[v.data_ptr() for v in vecs])
    out = dev_words([SENTINEL] * 10)
    BAD, ptr = _lib.ZK_ERR_BAD_ARG, out.data_ptr()

    def q(h=ctx.handle, curve=cid, table=cols, n_rows=65, smap=t.map.data_ptr(), slots=t.slots, n=10, operands=ops, ids=None, op_rows=10, o=ptr,
          oids=None, o_rows=10):
        return L.zk_lookup_map_query_dev(h, curve, table, n_rows, smap, slots, n, operands, ids, op_rows, o, oids, o_rows, None, None, None)
    assert q() == 0 and host_words(out) == [r[2] for r in rows[:10]]          # positions and the out-parameters are optional
    assert [q(h=None), q(curve=7), q(table=None), q(smap=None), q(operands=None), q(o=None)] == [BAD] * 6
    assert q(table=(ctypes.c_void_p * 4)(cols[0], cols[1], None, cols[3])) == BAD
    assert q(operands=(ctypes.c_void_p * 3)(ops[0], None, ops[2])) == BAD
    assert [q(slots=t.slots * 2), q(slots=t.slots - 1), q(op_rows=9), q(o_rows=9)] == [BAD] * 4
    assert q(n=1 << 32, op_rows=1 << 32, o_rows=1 << 32) == _lib.ZK_ERR_UNSUPPORTED
    assert q(n=0) == 0
    # an index outside its vector: refused by the flag word, and the query that holds it writes nothing
    out2 = dev_words([SENTINEL] * 10)
    ids_ok, ids_bad = dev_u32(range(10)), dev_u32([0, 1, 2, 10, 4, 5, 6, 7, 8, 9])
    id_ptrs = (ctypes.c_void_p * 3)(ids_ok.data_ptr(), ids_bad.data_ptr(), None)
    assert q(ids=id_ptrs, o=out2.data_ptr()) == BAD and host_words(out2)[3] == SENTINEL
    assert q(oids=dev_u32([0, 1, 2, 3, 4, 5, 6, 7, 8, 10]).data_ptr(), o=out2.data_ptr()) == BAD
    assert q(ids=(ctypes.c_void_p * 3)(ids_ok.data_ptr(), ids_ok.data_ptr(), ids_ok.data_ptr())) == 0
    # the build
    smap = torch.zeros(t.slots, dtype=torch.int32, device="cuda")
    a, b, d = t.cols[0].data_ptr(), t.cols[1].data_ptr(), t.cols[3].data_ptr()
    B = L.zk_lookup_map_build_dev
    assert [B(None, cid, a, b, d, 65, smap.data_ptr(), t.slots), B(ctx.handle, 7, a, b, d, 65, smap.data_ptr(), t.slots),
            B(ctx.handle, cid, a, None, d, 65, smap.data_ptr(), t.slots), B(ctx.handle, cid, a, b, d, 65, None, t.slots),
            B(ctx.handle, cid, a, b, d, 65, smap.data_ptr(), 64), B(ctx.handle, cid, a, b, d, 65, smap.data_ptr(), 512)] == [BAD] * 6
    assert B(ctx.handle, cid, a, b, d, (1 << 30) + 1, smap.data_ptr(), 1 << 31) == _lib.ZK_ERR_UNSUPPORTED
    assert B(ctx.handle, cid, None, None, None, 0, smap.data_ptr(), 64) == 0        # an empty table: an empty map
    torch.cuda.synchronize()
    assert smap[:64].cpu().numpy().view(np.uint32).tolist() == [EMPTY] * 64 and smap[64:].abs().sum().item() == 0
    assert q() == 0


# ---- 7. LookupTable.lookup
def fr_dev(cid, ints):
    import torch
    return torch.from_numpy(fr_to_mont(cid, ints).view(np.int64)).cuda()


def lookup_ints(table, cid, ctx, a, b, d):
    out = table.lookup(fr_dev(cid, a), fr_dev(cid, b), fr_dev(cid, d), cid, ctx)
    return [int(v) for v in fr_from_mont(cid, out.cpu().numpy().view(np.uint64))]


@pytest.mark.parametrize("cid", [0, 1])
def test_lookup_table_lookup(cid, ctx):
    r = get_curve(cid).r
    rng = random.Random(12 + cid)
    xor = LookupTable.xor_table(0, 4)
    a, b = [rng.randrange(16) for _ in range(130)], [rng.randrange(16) for _ in range(130)]
    assert lookup_ints(xor, cid, ctx, a, b, [r - 1] * 130) == [x ^ y for x, y in zip(a, b)]
    with pytest.raises(ElementNotIndexed, match="query 2 "):
        lookup_ints(xor, cid, ctx, [1, 2, 16, 3, 17], [1, 2, 3, 4, 5], [r - 1] * 5)
    with pytest.raises(ElementNotIndexed, match="query 0 "):
        lookup_ints(xor, cid, ctx, [1], [1], [0])           # the tag of another operation
    # the reference's own cases (lookup_table.rs:286-300)
    assert lookup_ints(LookupTable.add_table(0, 3), cid, ctx, [2], [3], [0]) == [5]
    with pytest.raises(ElementNotIndexed):
        lookup_ints(LookupTable.xor_table(0, 5), cid, ctx, [17], [367], [0])
    # rows and blocks mixed, with a key that two rows hold: the first is the answer
    t = LookupTable()
    t.insert_row(3, 5, 1000, 1)                             # before the mul block's (3, 5, 15 mod 8, 1)
    t.insert_multi_mul(2, 3)
    t.insert_and_row(12, 10, 5)                             # (12 & 10) % 5 = 3, tag 2
    t.insert_multi_and(6, 3)
    t.insert_add_row(7, 7, 10)
    t.insert_xor_row(9, 5, 7)                               # (9 ^ 5) % 7 = 5, tag -1
    t.insert_mul_row(6, 7, 100)                             # behind the block's (6, 7, 42 mod 8, 1)
    t.insert_row(r - 1, 0, 77, r - 1)
    assert t.size() == 1 + 36 + 1 + 4 + 4
    got = lookup_ints(t, cid, ctx, [3, 12, 7, 7, 9, 6, r - 1, 2], [5, 10, 7, 6, 5, 7, 0, 7], [1, 2, 0, 2, r - 1, 1, r - 1, 1])
    assert got == [1000, 3, 4, 6, 5, 2, 77, 6]
    # the columns and the map are kept until the table changes
    kept = t._dev
    lookup_ints(t, cid, ctx, [3], [5], [1])
    assert t._dev is kept
    with pytest.raises(ElementNotIndexed):
        lookup_ints(t, cid, ctx, [100], [200], [3])
    t.insert_row(100, 200, 300, 3)
    assert t._dev is None and lookup_ints(t, cid, ctx, [100, 3], [200, 5], [3, 1]) == [300, 1000]
    t.insert_multi_xor(0, 1)
    assert t._dev is None and lookup_ints(t, cid, ctx, [1], [0], [r - 1]) == [1]
