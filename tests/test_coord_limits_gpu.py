"""GPU: the integer kernels every sparse layer reads its tables from, against the dictionary model of coord_ref.py (tuples of
Python ints, no packing), at the limits of the key, under a full hash table, and through the device-count forms that the
prefetch path queues behind a compaction.  Every result is an integer or is compared bit for bit; there is no tolerance.

Entry point -> the tests that reach it:
  eprecon_hash_build_async            test_hash_grid_at_the_limit, test_kernel_maps_at_the_limit, test_maps_at_the_block_edge,
                                      test_full_table_*, test_three_keys_*, test_build_refuses_a_table_without_an_empty_slot
  eprecon_hash_query_async            the same, test_unique_at_the_limit, test_unique_dn_*, test_hash_build_dn_*
  eprecon_hash_status                 test_hash_grid_at_the_limit, test_clean_set_has_status_zero
  eprecon_hash_build_dn_async         test_hash_build_dn_inserts_the_live_rows_only
  eprecon_unique_coords_async         test_unique_at_the_limit, test_clean_set_has_status_zero, test_plain_unique_equals_the_model,
                                      test_unique_dn_* (the plain call on the live rows), test_hierarchy_dn_* (the chain)
  eprecon_unique_coords_dn_async      test_unique_dn_numbers_the_live_rows_only
  eprecon_unique_hierarchy_dn_async   test_hierarchy_dn_numbers_the_live_rows_only (n_dev given and null, levels 1, 2, 3)
  exclusive_scan_i32_dn               under the three unique entry points.  The form follows the capacity, the mask the device count:
                                      capacity 257 takes scan_small_kernel<8>, 8193 <16>, 16385 <32>, 32769 and 69637 tile sums +
                                      scan_apply<true> (17 and 35 tiles; levels 1 and 2 of a hierarchy run the same launches over
                                      fewer live rows).  The three-launch form above 4,096 tiles needs 8.4 M rows and stays with
                                      test_sparse_gpu.test_device_scan_stays_inside_its_scratch.
  eprecon_kernel_map_async (k3, k2)   test_kernel_maps_at_the_limit, test_a_neighbour_over_the_edge_does_not_alias,
                                      test_maps_at_the_block_edge
  eprecon_kernel_map_self_async       the same
  eprecon_transpose_map_async         the same
  eprecon_grid_rank_async             test_rank_volume_of_a_non_cubic_grid, test_rank_volume_of_an_empty_list
  eprecon_point_quantize_dn_async     test_point_quantize_dn_is_the_plain_call_on_the_live_rows
  eprecon_spvcnn_points_dn_async      test_spvcnn_points_dn_is_the_three_plain_calls_on_the_live_rows
  eprecon_upsample_async (coordinates), eprecon_aligned_coords_async, eprecon_point_quantize_async: the reference chain of the two

The table-full status (bit 1) is not constructed: no legal call reaches it.
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import coord_ref as R  # noqa: E402

POISON = 0x5A5A5A5A       # dead input rows: a batch field no key holds, so one read of a dead row sets the status word
FILL = 0x6B6B6B6B         # outputs before a call: the same property, should a later level read what an earlier one left unwritten
WS_FILL = 0x01010101      # every int32 of the workspace: a stale flag that gets summed changes the count
ERR_ARG = -1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def i32(shape, value):
    return torch.full(shape, value, dtype=torch.int32, device="cuda")


def _api():
    from eprecon_amd import _lib
    return _lib, _lib.load()


class Table:
    """a raw table of the C ABI: memory of eprecon_hash_table_bytes(capacity), every byte `fill` before the first call"""

    def __init__(self, capacity, fill=0xEE):
        _lib, lib = _api()
        self.capacity = int(capacity)
        self.mem = torch.full((int(lib.eprecon_hash_table_bytes(self.capacity)),), fill, dtype=torch.uint8, device="cuda")

    @classmethod
    def for_rows(cls, n):
        return cls(_api()[1].eprecon_hash_capacity(int(n)))

    def build(self, coords, n, q=1, n_dev=None):
        _lib, lib = _api()
        if n_dev is None:
            return lib.eprecon_hash_build_async(_lib.ptr(coords), n, q, _lib.ptr(self.mem), self.capacity, _lib.current_stream())
        return lib.eprecon_hash_build_dn_async(_lib.ptr(coords), n, _lib.ptr(n_dev), q, _lib.ptr(self.mem), self.capacity,
                                               _lib.current_stream())

    def query(self, queries, q=1):
        _lib, lib = _api()
        queries = dev(queries)
        out = i32((len(queries),), FILL)
        _lib.check(lib.eprecon_hash_query_async(_lib.ptr(self.mem), self.capacity, _lib.ptr(queries), len(queries), q, _lib.ptr(out),
                                                _lib.current_stream()), "eprecon_hash_query_async")
        return host(out)

    @property
    def header(self):
        return self.mem[:8].view(torch.int32).tolist()        # (status, the count a hierarchy call leaves)

    def occupied(self):
        keys = self.mem[256:256 + 8 * self.capacity].view(torch.int64)
        return int((keys != -1).sum().item())


def _unique_raw(coords, n_cap, q, table, n_dev=None, out_rows=None):
    """eprecon_unique_coords_async / _dn_async into pattern-filled outputs and a workspace of exactly the size the library asks for,
    every int32 of it WS_FILL -> (unique [out_rows, 4], inverse [out_rows], count)"""
    _lib, lib = _api()
    rows = n_cap if out_rows is None else out_rows
    uniq, inverse, count = i32((max(rows, 1), 4), FILL), i32((max(rows, 1),), FILL), i32((1,), -7)
    nbytes = int(lib.eprecon_unique_workspace_bytes(n_cap))
    assert nbytes % 4 == 0
    ws = i32((nbytes // 4,), WS_FILL)
    if n_dev is None:
        rc = lib.eprecon_unique_coords_async(_lib.ptr(coords), n_cap, q, _lib.ptr(table.mem), table.capacity, _lib.ptr(inverse),
                                             _lib.ptr(uniq), _lib.ptr(count), _lib.ptr(ws), nbytes, _lib.current_stream())
    else:
        rc = lib.eprecon_unique_coords_dn_async(_lib.ptr(coords), n_cap, _lib.ptr(n_dev), q, _lib.ptr(table.mem), table.capacity,
                                                _lib.ptr(inverse), _lib.ptr(uniq), _lib.ptr(count), _lib.ptr(ws), nbytes,
                                                _lib.current_stream())
    _lib.check(rc, "eprecon_unique_coords")
    return host(uniq), host(inverse), int(count.item())


def _arr(rows, width=4):
    return np.array(rows, np.int32).reshape(-1, width) if width else np.array(rows, np.int32)


# ---- 1. limits of the key --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", [1, 2, 4])
def test_unique_at_the_limit(q):
    """unique rows, inverse (-1 on refused rows), status word and count of the limit set; the accepted rows are numbered as if
    the refused ones were not there; a refused query answers -1 and leaves the status word alone"""
    from eprecon_amd import _lib
    from eprecon_amd.sparse import unique_coords, unique_coords_queued
    c = R.limit_set()
    want_u, want_inv, ids, want_status = R.unique_first(R.rows_of(c), q)
    assert want_status == 1 and -1 in want_inv
    uniq, inverse, grid = unique_coords_queued(dev(c), q)
    status, count = grid.header.tolist()
    assert (status, count) == (want_status, len(want_u))
    assert np.array_equal(host(uniq)[:count], _arr(want_u)) and np.array_equal(host(inverse), _arr(want_inv, 0))
    assert np.array_equal(host(grid.query(dev(c), q)), _arr(want_inv, 0))
    queries = R.query_set()
    assert np.array_equal(host(grid.query(dev(queries), q)), _arr(R.lookup(ids, R.rows_of(queries), q), 0))
    assert grid.header.tolist() == [want_status, len(want_u)]
    with pytest.raises(_lib.EpreconError):       # the reading wrapper turns the status word into an error
        unique_coords(dev(c), q)


@pytest.mark.parametrize("q", [1, 2, 4])
def test_hash_grid_at_the_limit(q):
    """HashGrid.build + query: every accepted row answers its first row, every refused one -1; bit 0 of the status is set by
    the build and a refused query leaves the word as it was"""
    from eprecon_amd import _lib
    from eprecon_amd.sparse import HashGrid
    c = R.limit_set()
    rows = R.rows_of(c)
    first = R.first_rows(rows, q)
    g = HashGrid(len(c), torch.device("cuda")).build(dev(c), q)
    assert np.array_equal(host(g.query(dev(c), q)), _arr(first, 0))
    assert int(g.header[0].item()) == 1
    queries = R.rows_of(R.query_set())
    table = {}
    for i, r in enumerate(rows):
        if first[i] == i:
            table[R.quantise(r, q)] = i
    assert np.array_equal(host(g.query(dev(R.query_set()), q)), _arr(R.lookup(table, queries, q), 0))
    assert int(g.header[0].item()) == 1
    with pytest.raises(_lib.EpreconError):
        g.status_ok()


@pytest.mark.parametrize("q", [1, 2, 4])
def test_clean_set_has_status_zero(q):
    """rows up to two cells from the limit and batch 14, none refused at q = 1, 2, 4: status 0 through every wrapper"""
    from eprecon_amd.sparse import HashGrid, unique_coords, unique_coords_queued
    c = R.clean_set()
    want_u, want_inv, ids, want_status = R.unique_first(R.rows_of(c), q)
    assert want_status == 0
    uniq, inverse, grid = unique_coords_queued(dev(c), q)
    assert grid.header.tolist() == [0, len(want_u)]
    assert np.array_equal(host(uniq)[:len(want_u)], _arr(want_u)) and np.array_equal(host(inverse), _arr(want_inv, 0))
    u2, inv2, _ = unique_coords(dev(c), q)
    assert np.array_equal(host(u2), _arr(want_u)) and np.array_equal(host(inv2), _arr(want_inv, 0))
    queries = R.query_set()                       # refused queries leave a clean status clean
    assert np.array_equal(host(grid.query(dev(queries), q)), _arr(R.lookup(ids, R.rows_of(queries), q), 0))
    assert grid.header.tolist() == [0, len(want_u)]
    assert HashGrid(len(c), torch.device("cuda")).build(dev(c), q).status_ok()


def _check_maps(c, stride):
    """k3, the self form of k3 (from a map filled with garbage), k2 from the coarse set and the transposed map of the distinct
    accepted rows `c` at `stride`, entry for entry against the model"""
    _lib, lib = _api()
    rows = R.rows_of(c)
    n = len(rows)
    ids = {r: i for i, r in enumerate(rows)}
    assert len(ids) == n
    dc = dev(c)
    t = Table.for_rows(n)
    _lib.check(t.build(dc, n), "eprecon_hash_build_async")
    assert t.header[0] == 0 and t.occupied() == n
    st = _lib.current_stream()

    want3 = _arr(R.kernel_map(ids, rows, 3, stride), n)
    k3 = i32((27, n), FILL)
    _lib.check(lib.eprecon_kernel_map_async(_lib.ptr(t.mem), t.capacity, _lib.ptr(dc), n, 3, stride, _lib.ptr(k3), st), "kernel_map k3")
    assert np.array_equal(host(k3), want3)
    over = np.array([[not R.in_range(r[0], r[1] + dx * stride, r[2] + dy * stride, r[3] + dz * stride) for r in rows]
                     for dx, dy, dz in R.offsets(3)])
    assert (host(k3)[over] == -1).all()          # every neighbour over the edge is absent, whatever it would alias to
    self3 = i32((27, n), FILL)
    _lib.check(lib.eprecon_kernel_map_self_async(_lib.ptr(t.mem), t.capacity, _lib.ptr(dc), n, stride, _lib.ptr(self3), st),
               "kernel_map_self")
    assert np.array_equal(host(self3), want3)

    coarse, parent, _, _ = R.unique_first(rows, 2 * stride)
    if coarse:
        m = len(coarse)
        k2 = i32((8, m), FILL)
        _lib.check(lib.eprecon_kernel_map_async(_lib.ptr(t.mem), t.capacity, _lib.ptr(dev(_arr(coarse))), m, 2, stride, _lib.ptr(k2), st),
                   "kernel_map k2")
        assert np.array_equal(host(k2), _arr(R.kernel_map(ids, coarse, 2, stride), m))
    up = i32((8, n), FILL)
    _lib.check(lib.eprecon_transpose_map_async(_lib.ptr(dc), n, _lib.ptr(dev(_arr(parent, 0))), stride, _lib.ptr(up), st),
               "transpose_map")
    assert np.array_equal(host(up), _arr(R.transpose_map(rows, parent, stride), n))
    return over


@pytest.mark.parametrize("stride", [1, 2, 4])
def test_kernel_maps_at_the_limit(stride):
    """the accepted part of the limit set at quantum = stride: voxels in the corner (+LIMIT, +LIMIT, -LIMIT) whose neighbours
    step over the edge, negative and odd-negative fine coordinates for the transposed map"""
    over = _check_maps(R.accepted_set(stride), stride)
    assert over.any()


def test_a_neighbour_over_the_edge_does_not_alias():
    """voxels at +LIMIT whose +4 neighbour, packed without the range test, is the key of another voxel of the set (the carry runs
    into the next field): the answer is -1, not that voxel"""
    c, pairs = R.alias_rows()
    over = _check_maps(c, R.ALIAS_STRIDE)
    assert all(over[k, i] for i, k, _ in pairs)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_maps_at_the_block_edge(n):
    """list lengths around the 256-thread block of the map launches"""
    for stride in (1, 2, 4):
        _check_maps(R.map_rows(n, stride), stride)


# ---- 2. hash under load ----------------------------------------------------------------------------------------------------

def test_full_table_returns_every_key_and_ends_absent_probes_on_its_one_empty_slot():
    """capacity 1024 with 1,023 distinct keys, the least the C ABI accepts (the wrappers hand it 2n + 1): long probe chains,
    and an absent key ends on the table's only empty slot"""
    _lib, lib = _api()
    keys, absent = R.hash_load_rows()
    t = Table(1024)
    _lib.check(t.build(dev(keys), 1023), "eprecon_hash_build_async")
    assert t.occupied() == 1023
    assert np.array_equal(t.query(keys), np.arange(1023, dtype=np.int32))
    assert (t.query(absent) == -1).all()
    assert t.header[0] == 0


def test_three_keys_under_twenty_thousand_rows_keep_their_first_row():
    """20,000 rows race atomicMin onto three slots"""
    _lib, lib = _api()
    c = R.three_key_rows()
    t = Table.for_rows(len(c))
    _lib.check(t.build(dev(c), len(c)), "eprecon_hash_build_async")
    assert t.occupied() == 3 and t.header[0] == 0
    assert np.array_equal(t.query(c), _arr(R.first_rows(R.rows_of(c)), 0))


def test_build_refuses_a_table_without_an_empty_slot():
    """n = capacity: EPRECON_ERR_ARG before anything is launched, the table's memory keeps its pattern"""
    keys = np.concatenate([R.hash_load_rows()[0], np.array([(2, 100, 100, 100)], np.int32)])
    t = Table(1024, fill=0xA5)
    before = t.mem.clone()
    assert t.build(dev(keys), 1024) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(t.mem, before)


# ---- 3. device counts ------------------------------------------------------------------------------------------------------

CAPS = [257, 8193, 16385, 32769, 69637]          # scan forms <8>, <16>, <32>, tiled (17 tiles), tiled (35 tiles)


def live_counts(cap):
    return [c for c in (-3, 0, 1, 2047, 2048, 2049) if c < cap - 1] + [cap - 1, cap, cap + 5]


@lru_cache(maxsize=None)
def _count_model(cap, q):
    """(rows, unique, inverse) of count_rows(cap) at quantum q as arrays, computed once: a prefix of the list numbers as a prefix
    (test_coord_ref.test_a_prefix_of_the_list_numbers_as_a_prefix)"""
    c = R.count_rows(cap)
    uniq, inv, _, status = R.unique_first(R.rows_of(c), q)
    assert status == 0
    return c, _arr(uniq), _arr(inv, 0)


def _cut(inv, live):
    return int(inv[:live].max()) + 1 if live > 0 else 0


def _poisoned(c, live):
    out = c.copy()
    out[live:] = POISON
    return out


UNIQUE_DN_CASES = ([(cap, n, 1) for cap in CAPS for n in live_counts(cap)]
                   + [(cap, n, q) for cap in (257, 8193, 16385, 69637) for q in (2, 4) for n in live_counts(cap)])


@pytest.mark.parametrize("cap,n_live,q", UNIQUE_DN_CASES)
def test_unique_dn_numbers_the_live_rows_only(cap, n_live, q):
    """rows at and above the count are poison, the workspace is stale, the outputs hold a pattern: the call equals the model
    and the plain call on coords[:live], reads no dead row (status 0), sums no stale flag (count) and writes nothing past the live
    range"""
    c, want_u, want_inv = _count_model(cap, q)
    live = min(max(n_live, 0), cap)
    count = _cut(want_inv, live)
    coords = dev(_poisoned(c, live))
    t = Table.for_rows(cap)
    uniq, inverse, got = _unique_raw(coords, cap, q, t, n_dev=dev(np.array([n_live], np.int32)))
    assert got == count and t.header[0] == 0
    assert np.array_equal(uniq[:count], want_u[:count]) and np.array_equal(inverse[:live], want_inv[:live])
    assert (inverse[live:] == FILL).all() and (uniq[count:] == FILL).all()
    assert t.occupied() == count
    if live:
        assert np.array_equal(t.query(c[:live], q), want_inv[:live])
    assert (t.query(np.full((64, 4), POISON, np.int32), q) == -1).all()
    # the plain call on the live rows
    t2 = Table.for_rows(cap)
    u2, inv2, got2 = _unique_raw(coords, live, q, t2, out_rows=cap)
    assert got2 == got and t2.header[0] == 0
    assert np.array_equal(u2, uniq) and np.array_equal(inv2, inverse)
    if live:
        assert np.array_equal(t2.query(c[:live], q), want_inv[:live])


@pytest.mark.parametrize("cap", CAPS)
def test_plain_unique_equals_the_model(cap):
    """the plain call, once per capacity, into the same stale workspace"""
    c, want_u, want_inv = _count_model(cap, 1)
    t = Table.for_rows(cap)
    uniq, inverse, got = _unique_raw(dev(c), cap, 1, t)
    assert got == len(want_u) and t.header[0] == 0 and t.occupied() == got
    assert np.array_equal(uniq[:got], want_u) and np.array_equal(inverse, want_inv) and (uniq[got:] == FILL).all()


@pytest.mark.parametrize("cap,n_live", [(cap, n) for cap in CAPS for n in live_counts(cap)])
def test_hash_build_dn_inserts_the_live_rows_only(cap, n_live):
    """live keys answer their first row; dead rows, ordinary or poison, are not in the table; status 0"""
    _lib, lib = _api()
    c, _, want_inv = _count_model(cap, 1)
    live = min(max(n_live, 0), cap)
    first = _arr(R.first_rows(R.rows_of(c[:live])), 0)
    t = Table.for_rows(cap)
    _lib.check(t.build(dev(_poisoned(c, live)), cap, 1, n_dev=dev(np.array([n_live], np.int32))), "eprecon_hash_build_dn_async")
    assert t.header[0] == 0 and t.occupied() == _cut(want_inv, live)
    if live:
        assert np.array_equal(t.query(c[:live]), first)
    if live < cap:
        assert (t.query(c[live:][~_in_rows(c[live:], c[:live])]) == -1).all()      # rows that are ordinary, but dead
    assert (t.query(np.full((64, 4), POISON, np.int32)) == -1).all()


def _in_rows(a, b):
    have = set(R.rows_of(b))
    return np.array([r in have for r in R.rows_of(a)], bool)


@lru_cache(maxsize=None)
def _hierarchy_model(cap):
    c = R.count_rows(cap)
    levels = R.hierarchy(R.rows_of(c), 3)
    assert all(lv[3] == 0 for lv in levels)
    return c, [(_arr(lv[0]), _arr(lv[1], 0)) for lv in levels]


def _hierarchy_raw(coords, n_cap, n_dev, levels, rows):
    """eprecon_unique_hierarchy_dn_async into pattern-filled outputs of `rows` rows per level"""
    _lib, lib = _api()
    tables = [Table.for_rows(max(rows, n_cap)) for _ in range(levels)]
    invs = [i32((rows,), FILL) for _ in range(levels)]
    uniqs = [i32((rows, 4), FILL) for _ in range(levels)]
    summary = i32((2 * levels,), FILL)
    nbytes = int(lib.eprecon_unique_workspace_bytes(n_cap))
    ws = i32((nbytes // 4,), WS_FILL)
    vp = ctypes.c_void_p * levels
    _lib.check(lib.eprecon_unique_hierarchy_dn_async(
        _lib.ptr(coords), n_cap, _lib.ptr(n_dev), levels, vp(*[t.mem.data_ptr() for t in tables]),
        (ctypes.c_uint32 * levels)(*[t.capacity for t in tables]), vp(*[t.data_ptr() for t in invs]),
        vp(*[t.data_ptr() for t in uniqs]), _lib.ptr(summary), _lib.ptr(ws), nbytes, _lib.current_stream()),
        "eprecon_unique_hierarchy_dn_async")
    return tables, [host(t) for t in uniqs], [host(t) for t in invs], summary.tolist()


@pytest.mark.parametrize("given", [True, False], ids=["n_dev", "null"])
@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("cap", CAPS)
def test_hierarchy_dn_numbers_the_live_rows_only(cap, levels, given):
    """per level: unique rows, inverse, count and status equal the model and the chain of plain calls; the summary equals the
    tables' headers; nothing is written past a level's live range.  n_dev null: the whole list of n_cap rows is live."""
    c, model = _hierarchy_model(cap)
    counts = [n for n in (-3, 0, 1, 2049) if n < cap - 1] + [cap - 1, cap + 5] if given else [0, 1, cap]
    for n_live in counts:
        live = min(max(n_live, 0), cap)
        if given:
            coords, n_cap, n_dev = dev(_poisoned(c, live)), cap, dev(np.array([n_live], np.int32))
        else:
            coords, n_cap, n_dev = dev(c), live, None
        tables, uniqs, invs, summary = _hierarchy_raw(coords, n_cap, n_dev, levels, cap)
        n_in, src, headers = live, coords, []
        for l in range(levels):
            want_u, want_inv = model[l]
            count = _cut(want_inv, n_in)
            assert tables[l].header == [0, count], (n_live, l)
            headers += tables[l].header
            assert np.array_equal(uniqs[l][:count], want_u[:count]) and np.array_equal(invs[l][:n_in], want_inv[:n_in]), (n_live, l)
            assert (uniqs[l][count:] == FILL).all() and (invs[l][n_in:] == FILL).all(), (n_live, l)
            assert tables[l].occupied() == count
            if count:
                assert np.array_equal(tables[l].query(want_u[:count], 1 << l), np.arange(count, dtype=np.int32))
            # the chain of plain calls: level l on what the plain call of level l - 1 wrote
            t2 = Table.for_rows(cap)
            u2, inv2, got2 = _unique_raw(src, n_in, 1 << l, t2, out_rows=cap)
            assert got2 == count and t2.header[0] == 0 and np.array_equal(u2, uniqs[l]) and np.array_equal(inv2, invs[l]), (n_live, l)
            n_in, src = count, dev(u2)
        assert summary == headers, n_live


# -- the point-coordinate launch of the prefetch path

POINT_CAP = 300
POINT_COUNTS = [-3, 0, 1, 255, 256, 257, POINT_CAP, POINT_CAP + 5]
VOXEL_SIZE, RESOLUTION = 0.04, 0.05


@lru_cache(maxsize=None)
def _camera():
    """two batch elements with different origins and world-to-camera matrices (a rotation about a skew axis and a translation)"""
    rng = np.random.default_rng(120)
    origin = rng.uniform(-2, 2, (2, 3)).astype(np.float32)
    w2ac = np.zeros((2, 4, 4), np.float32)
    for b in range(2):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        w2ac[b, :3, :3], w2ac[b, :3, 3], w2ac[b, 3, 3] = q, rng.uniform(-1, 1, 3), 1
    return origin, w2ac


def _bits(t):
    return host(t.contiguous().view(torch.int32))


def _nan(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _plain_points(src, live, children, interval):
    """eprecon_upsample_async -> eprecon_aligned_coords_async -> eprecon_point_quantize_async on the live rows"""
    _lib, lib = _api()
    origin, w2ac = (dev(a) for a in _camera())
    st = _lib.current_stream()
    n_pts = 8 * live if children else live
    if children:
        up = i32((max(n_pts, 1), 4), FILL)
        _lib.check(lib.eprecon_upsample_async(None, 0, _lib.ptr(src), live, 0, interval, None, _lib.ptr(up), st), "upsample")
    else:
        up = src
    r, scaled, vox = _nan((max(n_pts, 1), 4)), _nan((max(n_pts, 1), 4)), i32((max(n_pts, 1), 4), FILL)
    _lib.check(lib.eprecon_aligned_coords_async(_lib.ptr(up), n_pts, _lib.ptr(origin), 2, VOXEL_SIZE, _lib.ptr(w2ac), _lib.ptr(r), st),
               "aligned_coords")
    _lib.check(lib.eprecon_point_quantize_async(_lib.ptr(r), n_pts, RESOLUTION, _lib.ptr(scaled), _lib.ptr(vox), st), "point_quantize")
    return n_pts, host(up[:n_pts]), _bits(r[:n_pts]), _bits(scaled[:n_pts]), host(vox[:n_pts])


@pytest.mark.parametrize("children,interval", [(0, 1), (1, 1), (1, 2)])
def test_spvcnn_points_dn_is_the_three_plain_calls_on_the_live_rows(children, interval):
    """up_coords, r_coords, scaled_xyzb and voxel_bxyz bit for bit against upsample -> aligned_coords -> point_quantize on the
    live rows (the statement-by-statement claim of spvcnn_points_dn_kernel); NaN / pattern fill kept past the live range"""
    _lib, lib = _api()
    origin, w2ac = (dev(a) for a in _camera())
    c = R.ordinary_rows(POINT_CAP, 40, 2, seed=121)
    cap_pts = 8 * POINT_CAP if children else POINT_CAP
    nan_bits = _bits(_nan((1,)))[0]
    for n_live in POINT_COUNTS:
        live = min(max(n_live, 0), POINT_CAP)
        src = dev(_poisoned(c, live))
        up, vox, n_pts = i32((cap_pts, 4), FILL), i32((cap_pts, 4), FILL), i32((1,), -7)
        r, scaled = _nan((cap_pts, 4)), _nan((cap_pts, 4))
        _lib.check(lib.eprecon_spvcnn_points_dn_async(
            _lib.ptr(src), POINT_CAP, _lib.ptr(dev(np.array([n_live], np.int32))), children, interval, _lib.ptr(origin), 2, VOXEL_SIZE,
            _lib.ptr(w2ac), RESOLUTION, _lib.ptr(up) if children else None, _lib.ptr(r), _lib.ptr(scaled), _lib.ptr(vox),
            _lib.ptr(n_pts), _lib.current_stream()), "eprecon_spvcnn_points_dn_async")
        want_n, want_up, want_r, want_scaled, want_vox = _plain_points(src, live, children, interval)
        assert int(n_pts.item()) == want_n == (8 * live if children else live), n_live
        if children:
            assert np.array_equal(host(up)[:want_n], want_up), n_live
        assert np.array_equal(_bits(r)[:want_n], want_r) and np.array_equal(_bits(scaled)[:want_n], want_scaled), n_live
        assert np.array_equal(host(vox)[:want_n], want_vox), n_live
        assert (host(up)[want_n:] == FILL).all() and (host(vox)[want_n:] == FILL).all(), n_live
        assert (_bits(r)[want_n:] == nan_bits).all() and (_bits(scaled)[want_n:] == nan_bits).all(), n_live
        if live >= 255:     # the reference chain is not vacuous: real points, both batch elements, negative cells
            assert not np.isnan(host(r)[:want_n]).any() and (want_vox[:, 1:] < 0).any() and set(want_vox[:, 0].tolist()) == {0, 1}


def test_point_quantize_dn_is_the_plain_call_on_the_live_rows():
    """and the plain call is IEEE float32 division and floor"""
    _lib, lib = _api()
    rng = np.random.default_rng(122)
    pts = np.concatenate([rng.uniform(-3, 3, (POINT_CAP, 3)), rng.integers(0, 2, (POINT_CAP, 1))], 1).astype(np.float32)
    pts[:4, :3] = [[0.05, -0.05, 0.1], [-0.0, 0.049999997, -1e-9], [2.5, -2.5, 0.15], [-0.15000001, 0.1, -0.1]]   # on and beside cell faces
    nan_bits = _bits(_nan((1,)))[0]
    st = _lib.current_stream()
    for n_live in POINT_COUNTS:
        live = min(max(n_live, 0), POINT_CAP)
        dead = pts.copy()
        dead[live:] = np.nan
        src = dev(dead)
        scaled, vox = _nan((POINT_CAP, 4)), i32((POINT_CAP, 4), FILL)
        _lib.check(lib.eprecon_point_quantize_dn_async(_lib.ptr(src), POINT_CAP, _lib.ptr(dev(np.array([n_live], np.int32))), RESOLUTION,
                                                       _lib.ptr(scaled), _lib.ptr(vox), st), "eprecon_point_quantize_dn_async")
        s2, v2 = _nan((POINT_CAP, 4)), i32((POINT_CAP, 4), FILL)
        _lib.check(lib.eprecon_point_quantize_async(_lib.ptr(src), live, RESOLUTION, _lib.ptr(s2), _lib.ptr(v2), st), "point_quantize")
        assert np.array_equal(_bits(scaled), _bits(s2)) and np.array_equal(host(vox), host(v2)), n_live
        assert (_bits(scaled)[live:] == nan_bits).all() and (host(vox)[live:] == FILL).all(), n_live
        # the plain call itself: IEEE division and floor, in float32
        want_s = (pts[:live, :3] / np.float32(RESOLUTION)).astype(np.float32)
        assert np.array_equal(host(scaled)[:live, :3], want_s) and np.array_equal(host(scaled)[:live, 3], pts[:live, 3]), n_live
        assert np.array_equal(host(vox)[:live, 1:], np.floor(want_s).astype(np.int32)), n_live
        assert np.array_equal(host(vox)[:live, 0], pts[:live, 3].astype(np.int32)), n_live


# ---- 4. rank volume --------------------------------------------------------------------------------------------------------

RANK_DIMS = (5, 7, 11)


def _grid_rank(c, n, stride, dims):
    _lib, lib = _api()
    cells = dims[0] * dims[1] * dims[2]
    rank = i32((cells + 1,), FILL)
    _lib.check(lib.eprecon_grid_rank_async(_lib.ptr(c), n, stride, *dims, _lib.ptr(rank), _lib.current_stream()),
               "eprecon_grid_rank_async")
    return host(rank)


@pytest.mark.parametrize("stride", [1, 2])
def test_rank_volume_of_a_non_cubic_grid(stride):
    """5 x 7 x 11 cells: rows on about half of them, rows negative, off the stride, at and past each extent; the volume and the
    trailing off-grid word equal the model"""
    c = R.rank_rows(stride, RANK_DIMS)
    vol, off = R.grid_rank(R.rows_of(c), stride, RANK_DIMS)
    assert off > 0
    assert np.array_equal(_grid_rank(dev(c), len(c), stride, RANK_DIMS), _arr(vol + [off], 0))


def test_rank_volume_of_an_empty_list():
    got = _grid_rank(dev(R.rank_rows(1, RANK_DIMS)), 0, 1, RANK_DIMS)
    assert (got[:-1] == -1).all() and got[-1] == 0
