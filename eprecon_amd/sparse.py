"""Host-side handles for the sparse primitives of libeprecon_hip.so: coordinate sets with their
hash grid and cached kernel maps (the role torchsparse's SparseTensor.cmaps/.kmaps and spconv's
indice pairs play in the reference), sparse convolution, and the normalisation epilogues.

Coordinates are int32[N,4] rows (batch, x, y, z) everywhere in this package; wrappers that mirror
torchsparse's xyzb order convert at their boundary.
"""
import ctypes
import os
import threading

import torch

from . import _lib, weight_cache


class IdentityCache:
    """What was derived from a tensor's rows, found again for the same tensor: a bounded FIFO keyed on the tensor OBJECT
    plus (data_ptr, torch's version counter, row count, extra) — modules.voxel_set_for, torchsparse_utils.VOXELIZATIONS.
    Writes the HIP library makes through raw pointers do not bump the version counter: a caller that refills the SAME tensor
    in place (a persistent serving buffer) must call modules.clear_coordinate_caches() at the fragment boundary, or hand over
    fresh tensors per fragment as every path in this package does.  Guarded by a lock: the pipelined serving mode calls in
    from a worker thread while the main thread runs the next fragment."""

    def __init__(self, max_entries):
        self._max, self._items, self._lock = int(max_entries), [], threading.Lock()

    @staticmethod
    def _key(t, extra):
        return (t.data_ptr(), t._version, t.shape[0], extra)

    def get(self, t, extra=None):
        key = self._key(t, extra)
        with self._lock:
            for k, ref, value in self._items:
                if ref is t and k == key:
                    return value
        return None

    def put(self, *entries):
        """entries: (tensor, extra, value) each, oldest first; the oldest entries beyond the bound drop out"""
        with self._lock:
            self._items.extend((self._key(t, extra), t, value) for t, extra, value in entries)
            del self._items[:max(0, len(self._items) - self._max)]

    def values(self):
        with self._lock:
            return [value for _, _, value in self._items]

    def clear(self):
        with self._lock:
            self._items.clear()


def _dense3d_level():
    """EPRECON_CONV_DENSE3D: 0 the dense-grid form is off (all VoxelSet.conv_map asks here; which kernel a layer gets at levels
    1 and 2 is the library's answer: DenseMap.kind)"""
    return int(os.environ.get("EPRECON_CONV_DENSE3D", "2"))


def _ld(t):
    ld, unit = t.stride()       # (two strides: a 2-D tensor)
    assert unit == 1, "row-major 2-D tensor expected"
    return ld


def _res(residual):
    """(pointer, row stride) of an optional residual operand"""
    return _lib.ptr(residual), 0 if residual is None else _ld(residual)


def _rows_out(x, out):
    """`out`, or new float32 rows of x's shape"""
    return torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device) if out is None else out


class HashGrid:
    """device hash table over a coordinate set (eprecon_hash_*)"""

    def __init__(self, n, device):
        lib = _lib.load()
        self.capacity = int(lib.eprecon_hash_capacity(int(n)))
        self.mem = torch.empty(int(lib.eprecon_hash_table_bytes(self.capacity)), dtype=torch.uint8,
                               device=device)

    @property
    def header(self):
        """int32[2] view of the table's header: (status word, count of unique keys written by the unique calls)"""
        return self.mem[:8].view(torch.int32)

    def build(self, coords, quantum=1, n_dev=None):
        """n_dev (a device int32 element): only the first min(N, *n_dev) rows of `coords` are live"""
        lib = _lib.load()
        if n_dev is not None:
            _lib.check(lib.eprecon_hash_build_dn_async(_lib.ptr(coords), coords.shape[0], _lib.ptr(n_dev), quantum,
                                                       _lib.ptr(self.mem), self.capacity, _lib.current_stream()),
                       "eprecon_hash_build_dn_async")
            return self
        _lib.check(lib.eprecon_hash_build_async(_lib.ptr(coords), coords.shape[0], quantum,
                                                _lib.ptr(self.mem), self.capacity,
                                                _lib.current_stream()), "eprecon_hash_build_async")
        return self

    def query(self, queries, quantum=1):
        lib = _lib.load()
        out = torch.empty(queries.shape[0], dtype=torch.int32, device=queries.device)
        _lib.check(lib.eprecon_hash_query_async(_lib.ptr(self.mem), self.capacity, _lib.ptr(queries),
                                                queries.shape[0], quantum, _lib.ptr(out),
                                                _lib.current_stream()), "eprecon_hash_query_async")
        return out

    def status_ok(self):
        """blocking; raises when a key was out of range or the table overflowed"""
        lib = _lib.load()
        return _lib.check(lib.eprecon_hash_status(_lib.ptr(self.mem), _lib.current_stream()),
                          "eprecon_hash_status")


def check_hash_status(status):
    """status word of a hash table (bit 0: a key out of the packable range — |coordinate| >= 2^19 - 1 or batch > 14 —, bit 1:
    table full): such voxels would otherwise silently drop out of every kernel map built on the set"""
    if status:
        raise _lib.EpreconError(f"hash grid: {'coordinate / batch index out of range' if status & 1 else 'table full'} "
                                f"(status {status}, EPRECON_ERR_UNSUPPORTED)")


def unique_coords_queued(coords, quantum=1, n_dev=None):
    """Queue the unique (quantised) voxel numbering of `coords` WITHOUT reading the count back:
    -> (unique int32[N,4] whose first M rows are written, inverse int32[N], HashGrid).  M and the table's status word land in
    grid.header (device); n_dev (a device int32 element): only the first min(N, *n_dev) rows of `coords` are live."""
    lib = _lib.load()
    coords = coords.contiguous()
    n, dev = coords.shape[0], coords.device
    grid = HashGrid(n, dev)
    inverse = torch.empty(n, dtype=torch.int32, device=dev)
    uniq = torch.empty((n, 4), dtype=torch.int32, device=dev)
    n_unique = grid.header[1:2]
    ws = _lib.workspace(lib.eprecon_unique_workspace_bytes(n), dev)
    if n_dev is None:
        _lib.check(lib.eprecon_unique_coords_async(_lib.ptr(coords), n, quantum, _lib.ptr(grid.mem), grid.capacity,
                                                   _lib.ptr(inverse), _lib.ptr(uniq), _lib.ptr(n_unique), _lib.ptr(ws), ws.numel(),
                                                   _lib.current_stream()), "eprecon_unique_coords_async")
    else:
        _lib.check(lib.eprecon_unique_coords_dn_async(_lib.ptr(coords), n, _lib.ptr(n_dev), quantum, _lib.ptr(grid.mem),
                                                      grid.capacity, _lib.ptr(inverse), _lib.ptr(uniq), _lib.ptr(n_unique),
                                                      _lib.ptr(ws), ws.numel(), _lib.current_stream()),
                   "eprecon_unique_coords_dn_async")
    return uniq, inverse, grid


def unique_hierarchy_queued(coords, levels=3, n_dev=None, summary=None):
    """unique_coords_queued for the strides 1, 2, 4 (levels <= 3) of one point cloud in ONE library call (the tables of all strides are
    reset by one launch; level l numbers the unique rows of level l - 1 at quantum 2^l, its count taken from the device):
    -> (uniqs, inverses, grids), each a list over the levels; the counts / status words sit in grids[l].header and, side by
    side, in `summary` (an int32[2 levels] device tensor of the caller's: what it reads back, no torch.cat of the headers)"""
    if not 1 <= levels <= 3:    # (the library call numbers at most three strides and would answer EPRECON_ERR_ARG)
        raise ValueError(f"unique_hierarchy_queued: levels must be 1, 2 or 3 (strides 1, 2, 4), got {levels}")
    lib = _lib.load()
    coords = coords.contiguous()
    n, dev = coords.shape[0], coords.device
    grids = [HashGrid(n, dev) for _ in range(levels)]
    invs = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(levels)]
    uniqs = [torch.empty((n, 4), dtype=torch.int32, device=dev) for _ in range(levels)]
    ws = _lib.workspace(lib.eprecon_unique_workspace_bytes(n), dev)
    vp = ctypes.c_void_p * levels
    tables = vp(*[g.mem.data_ptr() for g in grids])
    caps = (ctypes.c_uint32 * levels)(*[g.capacity for g in grids])
    inv_p, uniq_p = vp(*[t.data_ptr() for t in invs]), vp(*[t.data_ptr() for t in uniqs])
    _lib.check(lib.eprecon_unique_hierarchy_dn_async(_lib.ptr(coords), n, _lib.ptr(n_dev), levels, tables, caps, inv_p, uniq_p,
                                                     _lib.ptr(summary), _lib.ptr(ws), ws.numel(), _lib.current_stream()),
               "eprecon_unique_hierarchy_dn_async")
    return uniqs, invs, grids


def unique_coords(coords, quantum=1):
    """-> (unique int32[M,4] in first-occurrence order, inverse int32[N], HashGrid mapping key -> id).
    One host sync to learn M (the reference's torch.unique syncs as well)."""
    uniq, inverse, grid = unique_coords_queued(coords, quantum)
    # the count lands next to the table's status word (the table's 256-byte header): ONE 8-byte host read, no torch.cat
    status, m = _lib.read_counts(grid.header)
    check_hash_status(status)
    return uniq[:m], inverse, grid


DIRECT_MAX_COUT = 64   # (operand-order packings are always handed over; which kernel runs is the library's choice)
DENSE_MIN_FILL = 0.4   # a set that fills at least this share of its bounding grid takes the dense-grid convolution


class DenseMap:
    """What a 3x3x3 stride-1 convolution needs on a voxel set that lives on a dense grid: the rank volume
    int32[gx*gy*gz (+1)] (cell -> row or -1, eprecon_grid_rank_async) instead of a hash grid + [27, N] kernel map.
    Layers whose shape the tile kernel does not take fall back to the set's kernel map (built on first use)."""

    def __init__(self, vset, dims, rank=None):
        """rank: the volume when its producer wrote it already (the back-projection of a dense raster,
        back_project.dense_rank_buffer: every row on the grid by construction) — nothing is launched and nothing checked"""
        lib = _lib.load()
        self.vset, self.dims = vset, tuple(int(d) for d in dims)
        gx, gy, gz = self.dims
        if rank is not None:
            assert rank.dtype == torch.int32 and rank.numel() == gx * gy * gz + 1 and rank.device == vset.coords.device
            self.rank = rank
            return
        self.rank = torch.empty(gx * gy * gz + 1, dtype=torch.int32, device=vset.coords.device)
        _lib.check(lib.eprecon_grid_rank_async(_lib.ptr(vset.coords), vset.n, vset.stride, gx, gy, gz, _lib.ptr(self.rank),
                                               _lib.current_stream()), "eprecon_grid_rank_async")
        # rank[-1] counts the voxels that were NOT on the declared grid (their output rows would stay unwritten): checked with
        # the next blocking count read on this stream (_lib.read_counts), at no read of its own
        _lib.defer_check(self.rank[-1:], 0, "dense-grid convolution: voxels of the set are not on the grid their VoxelSet was "
                                            "declared with (rows left unwritten)")

    @property
    def shape(self):          # (K, N) like the kernel-map tensor it stands in for
        return (27, self.vset.n)

    def off_grid(self):
        """blocking: number of voxels that were not on the grid (0 for a valid set)"""
        return int(self.rank[-1].item())

    def describe(self, desc, stats=False):
        """Ask the library which dense-grid kernel it has for the 3x3x3 launch `desc` describes on this grid (x, the channel
        counts, the pending input BatchNorm, ln and accumulate are set; stats: it will write BatchNorm summaries):
        eprecon_conv_dense3d_kind, the shape rule of csrc/sparse_conv_dense3d.hip -> 0 none, 1 single-column kernel, 2 16-row
        MFMA kernel (which wants packed_weight16).  The grid stays in `desc` unless the answer is 0."""
        desc.vox_rank = self.rank.data_ptr()
        desc.grid_x, desc.grid_y, desc.grid_z = self.dims
        # (the rule asks WHETHER summaries are written; their buffer is sized once the kernel is known: any address will do)
        desc.bn_partial = 1 if stats else None
        kind = int(_lib.load().eprecon_conv_dense3d_kind(ctypes.byref(desc)))
        desc.bn_partial = None
        if not kind:
            desc.vox_rank, desc.grid_x, desc.grid_y, desc.grid_z = None, 0, 0, 0
        return kind

    def kind(self, x, cin, cout, accumulate=False, ln=False, stats=False):
        """the library's answer for a layer of this shape on x: 0 none (kernel map), 1 single-column kernel, 2 16-row MFMA
        kernel"""
        d = _lib.ConvDesc()
        d.x, d.ld_x, d.n_in, d.n_out = x.data_ptr(), x.stride(0), self.vset.n, self.vset.n
        d.kvol, d.cin, d.cout = 27, cin, cout
        d.accumulate, d.ln = int(accumulate), int(ln)
        return self.describe(d, stats)

    def takes(self, x, cin, cout, accumulate=False, ln=False, stats=False):
        return self.kind(x, cin, cout, accumulate, ln, stats) != 0


# Every packing made from a weight tensor's own storage is remembered here (weak reference to the tensor object the cache lives
# on): repack_registered() rebuilds them all in ONE launch after an optimizer step (TrainStep.run) instead of one launch per
# layer at its next use — ~190 launches per step.  (id(owner), slot) -> (weakref, shape, the cache entry's extra)
_PACK_REGISTRY = {}
_PACK_TABLE = {"key": None, "jobs": None}
_PACK, _PACK16 = "sparse.packed_weight", "sparse.packed_weight16"     # slots of weight_cache; the library's kinds 0 and 1


def _pack(weight, owner, slot, extra=()):
    """the build step of packed_weight / packed_weight16: one packing launch, registered for repack_registered"""
    import weakref
    lib = _lib.load()
    name = "eprecon_conv_pack_weight16" if slot == _PACK16 else "eprecon_conv_pack_weight"
    kvol, cin, cout = weight.shape
    w = weight.detach().contiguous()
    packed = torch.empty(int(getattr(lib, name + "_floats")(kvol, cin, cout)), dtype=torch.float32, device=weight.device)
    _lib.check(getattr(lib, name + "_async")(_lib.ptr(w), kvol, cin, cout, _lib.ptr(packed), _lib.current_stream()), name + "_async")
    if w.data_ptr() == owner.data_ptr():
        _PACK_REGISTRY[(id(owner), slot)] = (weakref.ref(owner), (kvol, cin, cout), extra)
    else:       # packed from a temporary contiguous copy: nothing a later launch could re-read
        _PACK_REGISTRY.pop((id(owner), slot), None)
    return packed


def repack_registered():
    """Rebuild every registered operand-order copy whose weight has changed since it was packed (an optimizer step changes
    them all), in one launch on the current stream; the caches' tags follow, so the layers' next packed_weight /
    packed_weight16 calls are hits.  Tensors that were freed, moved or re-shaped drop out of the registry.  -> jobs launched"""
    import numpy as np
    stale = []
    for key, (ref, shape, extra) in list(_PACK_REGISTRY.items()):
        owner, slot = ref(), key[1]
        packed = weight_cache.peek(owner, slot) if owner is not None else None
        if packed is None or not owner.is_cuda:
            del _PACK_REGISTRY[key]
        elif not weight_cache.current(owner, slot, (owner,), extra):
            stale.append((owner, slot, shape, packed, extra))
    if not stale:
        return 0
    key = tuple((o.data_ptr(), k, s, p.data_ptr()) for o, k, s, p, _ in stale)
    if _PACK_TABLE["key"] != key:     # (the table is uploaded once: pointers and shapes do not change from step to step)
        job = np.zeros(len(stale), dtype=np.dtype([("weight", "<u8"), ("packed", "<u8"), ("kvol", "<i4"), ("cin", "<i4"),
                                                   ("cout", "<i4"), ("kind", "<i4")]))
        for i, (o, k, s, p, _) in enumerate(stale):
            job[i] = (o.data_ptr(), p.data_ptr(), s[0], s[1], s[2], int(k == _PACK16))
        _PACK_TABLE["jobs"] = torch.from_numpy(job.view(np.uint8).copy()).to(stale[0][0].device)
        _PACK_TABLE["key"] = key
    lib = _lib.load()
    _lib.check(lib.eprecon_conv_pack_many_async(_lib.ptr(_PACK_TABLE["jobs"]), len(stale), _lib.current_stream()),
               "eprecon_conv_pack_many_async")
    for o, k, _, _, extra in stale:
        weight_cache.retag(o, k, (o,), extra)
    return len(stale)


def packed_weight(weight):
    """`weight` f32[27, Cin, Cout] in the operand order of the dense-grid kernel (cached: weight_cache)"""
    return weight_cache.derived(weight, _PACK, (weight,), lambda: _pack(weight, weight, _PACK))


def packed_weight16(weight, owner=None):
    """`weight` f32[K, Cin, Cout <= 80] in the operand order of the 16x16x4 MFMA kernels (16-row tile kernel, direct gather
    kernel) (cached: weight_cache).  owner: the tensor OBJECT the packing is cached on when `weight` is a transient
    view of it (a [Cin, Cout] matrix unsqueezed to K = 1)"""
    owner = weight if owner is None else owner
    shape = tuple(weight.shape)
    return weight_cache.derived(owner, _PACK16, (owner,), lambda: _pack(weight, owner, _PACK16, shape), shape)


def voxel_hierarchy(vox, levels=3, points=None):
    """The voxel sets of a point cloud at tensor strides 1, 2, 4, ... with ONE host read for all their sizes: the unique
    numbering of `vox` int32[N,4] and of each coarser stride is queued back to back (the coarser calls take the finer
    count from the device, eprecon_unique_coords_dn_async), then the `levels` counts and status words are read together.
    -> (VoxelSet at stride 1 with its downsample chain attached, inverse int32[N], tables or None).
    points = scaled f32[N,4] (levels == 3, SPVCNN): everything else a pass needs from the coordinates — CSR point lists and
    trilinear corner tables of strides 1 and 4, the strided maps, the three kernel maps — is queued by ONE library call
    behind the read (eprecon_spvcnn_geometry_async): `tables`, the dict of its 16 tensors."""
    n = vox.shape[0]
    summary = torch.empty(2 * levels, dtype=torch.int32, device=vox.device)
    uniqs, invs, grids = unique_hierarchy_queued(vox, levels, summary=summary)
    host = _lib.read_counts(summary)
    sizes = []
    for lvl in range(levels):
        check_hash_status(host[2 * lvl])
        sizes.append(host[2 * lvl + 1])
    if points is not None and levels == 3 and n > 0 and sizes[0] > 0:
        return _hierarchy_with_geometry(vox, points, grids, uniqs, invs, sizes)
    base = VoxelSet(uniqs[0][:sizes[0]], 1, grid=grids[0])
    cur = base
    for lvl in range(1, levels):
        cur = cur.downsample(pre=(uniqs[lvl][:sizes[lvl]], invs[lvl][:sizes[lvl - 1]], grids[lvl]))[0]
    return base, invs[0], None


def _hierarchy_with_geometry(vox, points, grids, uniqs, invs, sizes):
    lib = _lib.load()
    dev = vox.device
    n = vox.shape[0]
    n1, n2, n4 = sizes
    c1, c2, c4 = uniqs[0][:n1], uniqs[1][:n2], uniqs[2][:n4]
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    t = {"offsets1": i32(n1 + 1), "order1": i32(n), "idx4": i32(n), "offsets4": i32(n4 + 1), "order4": i32(n),
         "down12": i32(8, n2), "up21": i32(8, n1), "down24": i32(8, n4), "up42": i32(8, n2),
         "k1": i32(27, n1), "k2": i32(27, n2), "k4": i32(27, n4), "idx8_1": i32(n, 8), "idx8_4": i32(n, 8),
         "weight8_1": torch.empty((n, 8), dtype=torch.float32, device=dev),
         "weight8_4": torch.empty((n, 8), dtype=torch.float32, device=dev)}
    d = _lib.SpvcnnGeometryDesc()
    d.n, d.n1, d.n2, d.n4 = n, n1, n2, n4
    d.scaled, d.vox, d.inverse1 = points.data_ptr(), vox.data_ptr(), invs[0].data_ptr()
    d.coords1, d.coords2, d.coords4 = c1.data_ptr(), c2.data_ptr(), c4.data_ptr()
    d.parent2, d.parent4 = invs[1].data_ptr(), invs[2].data_ptr()
    d.table1, d.table2, d.table4 = (g.mem.data_ptr() for g in grids)
    d.capacity1, d.capacity2, d.capacity4 = (g.capacity for g in grids)
    for name, buf in t.items():
        setattr(d, name, buf.data_ptr())
    ws = _lib.workspace(lib.eprecon_spvcnn_geometry_workspace_bytes(n, n1, n4), dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(lib.eprecon_spvcnn_geometry_async(ctypes.byref(d), _lib.current_stream()), "eprecon_spvcnn_geometry_async")
    s1 = VoxelSet(c1, 1, grid=grids[0], kernel_map=t["k1"])
    s2 = VoxelSet(c2, 2, grid=grids[1], kernel_map=t["k2"])
    s4 = VoxelSet(c4, 4, grid=grids[2], kernel_map=t["k4"])
    s1.attach_downsample(s2, t["down12"], t["up21"])
    s2.attach_downsample(s4, t["down24"], t["up42"])
    return s1, invs[0], t


def clear_packed_weights(module):
    """Drop every weight-derived copy cached on `module`, its submodules and their parameters: the contract after a write
    through `p.data` (weight_cache has the rule)"""
    weight_cache.clear(module)


# point-wise layers (K = 1) on lists at least this long take the direct kernel too (a streaming [N, C_in] x [C_in, C_out <= 64]
# product: csrc/sparse_conv_direct_kernels.hpp); shorter lists are launch-bound on any kernel
K1_DIRECT_MIN_ROWS = 20000


def conv_packings(kvol, cout, rows, mapped, accumulate=False, dense_kind=0, k1_min_rows=None, image_limits=None):
    """THE hand-over rule: which operand-order copies of its weights ride along with a described launch
    -> (packed_weight, packed_weight16).  Which kernel runs is the library's choice (select_conv, csrc/sparse_conv.hip); a
    packing only makes the kernels that read it possible, and they decline without it.
    rows: output rows; mapped: the launch has a kernel map (False: identity map); dense_kind: DenseMap.describe's answer for a
    launch that stays on the dense grid; k1_min_rows: the caller's threshold for point-wise layers in place of
    K1_DIRECT_MIN_ROWS (dense2d: K1_DIRECT_2D_MIN_ROWS; 0, "any length", where a descriptor is built before the row count exists:
    SPVCNN._native_desc, whose launches csrc/spvcnn_forward.hip then holds to kK1DirectMinRows); image_limits: dense2d's
    (DIRECT_2D_MIN_ROWS, SHORT_2D_MAX_ROWS, SHORT_2D_MAX_COUT) for a 3x3 image layer"""
    if dense_kind:                 # the 16-row tile kernel reads the 16x16x4 order, the single-column kernel the plain weights
        return False, dense_kind == 2
    if accumulate:
        return False, False
    direct = cout <= DIRECT_MAX_COUT
    if kvol == 1 and not mapped:   # point-wise layers on long lists: the direct kernel as a streaming product
        return False, direct and rows >= (K1_DIRECT_MIN_ROWS if k1_min_rows is None else k1_min_rows)
    if kvol == 27 and mapped:      # short lists: split-K (and the cross-workgroup kernel) on the 32x32x2 order; long lists: the
        return True, direct        # direct gather kernel on the 16x16x4 order
    if kvol == 9 and image_limits is not None:
        direct_min_rows, short_max_rows, short_max_cout = image_limits
        if rows < direct_min_rows:     # short pixel lists: split-K, and below short_max_rows the short-list image-tile kernel
            return True, rows < short_max_rows and cout <= short_max_cout
        return False, direct           # long pixel lists: the direct gather kernel on the pixel map / the 16-row image-tile kernel
    return False, False


class VoxelSet:
    """A set of active voxels at one tensor stride: coords int32[N,4] (b,x,y,z), its hash grid and
    the kernel maps built on it.  Maps are built once and reused by every layer on the set.
    `dims` (optional): the set lives on the dense grid of dims cells of `stride` voxels starting at 0 (a raster of
    generate_grid, ops/generate_grids.py:3-10) — its 3x3x3 layers then run on the dense-grid kernel when it is full enough.
    `rank` (optional, with dims): the grid's rank volume int32[cells + 1], already written by the set's producer.
    `kernel_map` (optional): the [27, N] neighbour table, already written by the set's producer."""

    def __init__(self, coords, stride=1, grid=None, dims=None, rank=None, kernel_map=None):
        assert coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 4
        self.coords = coords.contiguous()
        self.stride = int(stride)
        self.dims = None if dims is None else tuple(int(d) for d in dims)
        self._grid = grid
        self._k3 = kernel_map
        self._down = None
        self._dense = None
        self._rank = rank        # the rank volume of `dims` when the set's producer wrote it (DenseMap)

    def attach_downsample(self, coarse, down, up):
        """the k2s2 strided set and its two maps when their producer wrote them already: what downsample() then returns"""
        self._down = (coarse, down, up)

    def built_kernel_map(self):
        """the [27, N] table if a layer or the set's producer has built it, else None; launches nothing"""
        return self._k3

    def built_downsample(self):
        """(coarse, down, up) if built or attached, else None; launches nothing"""
        return self._down

    def conv_map(self, ksize=3):
        """what a stride-1 k=3 layer on this set takes as its map: a DenseMap for a well-filled dense grid, else the
        [27, N] kernel map"""
        assert ksize == 3
        if self.dims is not None and self.n >= DENSE_MIN_FILL * self.dims[0] * self.dims[1] * self.dims[2] \
                and _dense3d_level() > 0 and self.coords.is_cuda:
            if self._dense is None:
                self._dense = DenseMap(self, self.dims, rank=self._rank)
            return self._dense
        return self.kernel_map(3)

    @property
    def n(self):
        return self.coords.shape[0]

    @property
    def grid(self):
        if self._grid is None:
            self._grid = HashGrid(self.n, self.coords.device).build(self.coords)
        return self._grid

    def _offset_map(self, centres, ksize):
        """int32[ksize^3, M]: the rows of this set at the ksize^3 offsets around each of the M rows of `centres`"""
        nbr = torch.empty((ksize ** 3, centres.shape[0]), dtype=torch.int32, device=self.coords.device)
        _lib.check(_lib.load().eprecon_kernel_map_async(_lib.ptr(self.grid.mem), self.grid.capacity,
                                                        _lib.ptr(centres), centres.shape[0], ksize, self.stride,
                                                        _lib.ptr(nbr), _lib.current_stream()),
                   "eprecon_kernel_map_async")
        return nbr

    def kernel_map(self, ksize=3):
        """int32[27, N] neighbour table of the stride-1 k=3 convolution on this set"""
        assert ksize == 3
        if self._k3 is None:
            self._k3 = self._offset_map(self.coords, 3)
        return self._k3

    def downsample(self, pre=None):
        """k2s2 strided set: -> (coarse VoxelSet, down_map int32[8, M], up_map int32[8, N]).
        pre = (unique int32[M,4], parent int32[N], HashGrid): the strided set numbered by an earlier queued call
        (voxel_hierarchy: the counts of all strides read back at once)"""
        if self._down is None:
            lib = _lib.load()
            q = 2 * self.stride
            uniq, parent, cgrid = pre if pre is not None else unique_coords(self.coords, quantum=q)
            coarse = VoxelSet(uniq, q, grid=cgrid)
            down = self._offset_map(coarse.coords, 2)
            up = torch.empty((8, self.n), dtype=torch.int32, device=self.coords.device)
            _lib.check(lib.eprecon_transpose_map_async(_lib.ptr(self.coords), self.n, _lib.ptr(parent),
                                                       self.stride, _lib.ptr(up), _lib.current_stream()),
                       "eprecon_transpose_map_async")
            self.attach_downsample(coarse, down, up)
        return self._down


def sparse_conv(x, weight, nbr=None, bias=None, out=None, relu=False, accumulate=False):
    """out[i] (op)= bias + sum_k x[nbr[k][i]] @ weight[k].  weight f32[K, Cin, Cout] (or [Cin, Cout]
    with nbr None: a per-voxel linear layer).  x / out may be column slices of wider buffers."""
    return conv_call(x, weight, nbr, bias, out, relu, accumulate, positional=True)[0]     # = sparse_conv_fused(...)[0]


def bn_summaries(rows, cout, device):
    """a buffer for the per-workgroup BatchNorm summaries of `rows` workgroups: stored channel-major, f32[3, cout, rows] (what
    the finalize reads as three contiguous runs per channel), handed out as the logical [rows, 3, cout] view"""
    return torch.empty((3, cout, max(int(rows), 1)), dtype=torch.float32, device=device).permute(2, 0, 1)


def summary_layout(partial):
    """(nblk, ld) of a [rows, 3, C] summary view over channel-major storage (bn_summaries); asserts that layout"""
    nblk, three, c = partial.shape
    s0, s1, s2 = partial.stride()
    assert three == 3 and partial.dtype == torch.float32 and s0 == 1 and s2 >= nblk and s1 == c * s2, \
        "BatchNorm summaries must be the channel-major view bn_summaries() returns"
    return nblk, s2


def attach_summaries(desc, device):
    """size the BatchNorm summaries for the kernel the library gives the described launch to (the workgroups differ from family
    to family) and attach them -> the [rows, 3, cout] view"""
    rows = max(int(_lib.load().eprecon_conv_desc_partial_rows(ctypes.byref(desc))), 1)
    partial = bn_summaries(rows, desc.cout, device)
    desc.bn_partial, desc.bn_ld = partial.data_ptr(), rows      # (bn_summaries' layout: the row stride is the row count)
    return partial


def conv_call(x, weight, nbr=None, bias=None, out=None, relu=False, accumulate=False, residual=None, res_affine=None,
              in_affine=None, in_acc=None, ln=None, image=None, stats=False, positional=False, launch=True,
              k1_min_rows=None, image_limits=None):
    """THE host path of a convolution launch, for every wrapper: operands normalised and checked, `out` allocated, the
    eprecon_conv_desc filled, the map resolved, the packings of conv_packings attached, the workspace and (stats) the BatchNorm
    summaries the library asks for, the launch -> (out, summaries or None, descriptor, temporaries).
    weight f32[K, Cin, Cout], or [Cin, Cout] (K = 1): operand-order packings are cached on the object given here; nbr: None
    (identity map), an int32[K, N] kernel map or a DenseMap; res_affine / in_affine = (scale, shift, relu): the pending BatchNorm
    of the residual / the input, applied on load; in_acc = (accumulator slice, eps, relu): the input's BatchNorm still in its
    accumulator block; ln = (gamma, beta, eps, post_relu): row-wise LayerNorm epilogue; image = (height, width, maps) of a 3x3
    image layer; k1_min_rows / image_limits: see conv_packings.
    positional: the caller has no fusion beyond the positional eprecon_sparse_conv_fused_async and takes it where the routing
    below says so (no descriptor is returned then).  launch=False: the caller finishes the descriptor (dense2d's BatchNorm
    tail) and queues it, holding the temporaries until then."""
    lib = _lib.load()
    owner = weight
    if weight.dim() == 2:
        weight = weight.unsqueeze(0)
    kvol, cin, cout = weight.shape
    weight = weight.contiguous()
    dense = isinstance(nbr, DenseMap)
    n_in, c_x = x.shape
    n_out = n_in
    if nbr is not None:
        k_map, n_out = nbr.shape
        assert dense or (nbr.dtype == torch.int32 and k_map == kvol and nbr.is_contiguous())
    assert c_x == cin and x.dtype == torch.float32
    if out is None:
        out = torch.empty((n_out, cout), dtype=torch.float32, device=x.device)
    assert out.shape == (n_out, cout)
    (ld_x, unit_x), (ld_out, unit_out) = x.stride(), out.stride()
    assert unit_x == 1 and unit_out == 1, "row-major 2-D tensors expected"
    if residual is not None:
        assert residual.shape == (n_out, cout) and residual.dtype == torch.float32
    pack, pack16 = conv_packings(kvol, cout, n_out, nbr is not None, accumulate, 0, k1_min_rows, image_limits)
    # Routing of sparse_conv_fused: a DenseMap, a 3x3x3 layer on a kernel map and every launch with a packing to hand over
    # (point-wise layers on long lists) go through the descriptor; everything else takes the positional entry point, whose
    # summaries are per 128 rows (the kernels with other workgroups decline it)
    if positional and not (dense or (x.is_cuda and ((kvol == 27 and nbr is not None) or pack or pack16))):
        partial = bn_summaries((n_out + 127) // 128, cout, x.device) if stats else None
        _lib.check(lib.eprecon_sparse_conv_fused_async(
            x.data_ptr(), n_in, ld_x, _lib.ptr(nbr), kvol, n_out, _lib.ptr(weight), cin, cout, _lib.ptr(bias),
            _lib.ptr(residual), _ld(residual) if residual is not None else 0, out.data_ptr(), ld_out, int(relu),
            int(accumulate), _lib.ptr(partial), _lib.current_stream()), "eprecon_sparse_conv_fused_async")
        return out, partial, None, None
    d = _lib.ConvDesc()
    d.x, d.n_in, d.ld_x = x.data_ptr(), n_in, ld_x
    d.kvol, d.n_out = kvol, n_out
    d.weight, d.cin, d.cout = weight.data_ptr(), cin, cout
    if bias is not None:
        d.bias = bias.data_ptr()
    if residual is not None:
        d.residual, d.ld_res = residual.data_ptr(), _ld(residual)
        if res_affine is not None:
            d.res_scale, d.res_shift, d.res_relu = _lib.ptr(res_affine[0]), _lib.ptr(res_affine[1]), int(res_affine[2])
    d.out, d.ld_out = out.data_ptr(), ld_out
    if relu:
        d.relu = 1
    if accumulate:
        d.accumulate = 1
    if in_acc is not None:
        acc, eps, in_relu = in_acc
        assert acc.c == cin
        d.in_acc, d.in_acc_ld, d.in_acc_c0, d.in_eps, d.in_relu = acc.block.data_ptr(), acc.ld, acc.c0, float(eps), int(in_relu)
    elif in_affine is not None:
        d.in_scale, d.in_shift, d.in_relu = _lib.ptr(in_affine[0]), _lib.ptr(in_affine[1]), int(in_affine[2])
    if ln is not None:
        assert cout <= 128
        d.ln, d.ln_gamma, d.ln_beta, d.ln_eps, d.ln_post_relu = 1, _lib.ptr(ln[0]), _lib.ptr(ln[1]), float(ln[2]), int(ln[3])
    if image is not None:
        d.img_h, d.img_w, d.img_maps = image
    # the map: the dense grid where the library has a kernel for this shape on it, else the (set's) kernel map
    if dense:
        kind = nbr.describe(d, stats)
        if kind:
            nbr = nbr.rank
            pack, pack16 = conv_packings(kvol, cout, n_out, True, accumulate, kind)
        else:
            nbr = nbr.vset.kernel_map(3)
            d.nbr = nbr.data_ptr()
    elif nbr is not None:
        d.nbr = nbr.data_ptr()
    keep = [weight, nbr]
    if x.is_cuda:
        if pack:
            keep.append(packed_weight(weight))
            d.packed_weight = keep[-1].data_ptr()
        if pack16:
            keep.append(packed_weight16(weight, owner))
            d.packed_weight16 = keep[-1].data_ptr()
    # scratch of the kernel pair that reduces partial sums across workgroups: the library says how much the described launch
    # wants.  Asked only where the answer can be other than 0: wide_shape_ok (csrc/sparse_conv_wide.hip) needs K = 27, a
    # kernel map, packed_weight, at least 96 input channels and no LayerNorm; the opt-in persistent form (its job counters)
    # needs EPRECON_CONV_PERSIST=1 and packed_weight16
    if (kvol == 27 and cin >= 96 and ln is None and d.packed_weight and d.nbr) or (
            d.packed_weight16 and os.environ.get("EPRECON_CONV_PERSIST", "")[:1] == "1"):
        need = int(lib.eprecon_conv_desc_workspace_bytes(ctypes.byref(d)))
        if need:
            keep.append(_lib.workspace(need, x.device))
            d.workspace, d.workspace_bytes = keep[-1].data_ptr(), need
    partial = attach_summaries(d, x.device) if stats else None
    if launch:
        _lib.check(lib.eprecon_conv_desc_async(ctypes.byref(d), _lib.current_stream()), "eprecon_conv_desc_async")
    return out, partial, d, keep


def sparse_conv_fused(x, weight, nbr=None, bias=None, out=None, relu=False, residual=None, accumulate=False,
                      bn_partial=False):
    """sparse_conv with the fused epilogues: v = conv + bias [+ out]; [relu]; [+ residual]; and, with
    bn_partial, the per-workgroup BatchNorm summaries [ceil(n/128), 3, cout] of the stored values (a bn_summaries view).
    Returns (out, partial or None)."""
    return conv_call(x, weight, nbr, bias, out, relu, accumulate, residual, stats=bn_partial, positional=True)[:2]


def sparse_conv_ln(x, weight, nbr, bias, ln_weight, ln_bias, ln_eps, out=None, relu=False, residual=None,
                   post_relu=False):
    """conv + bias [+ReLU] [+residual] -> row-wise LayerNorm [-> ReLU] in ONE launch (descriptor entry point):
    the spconv + LayerNorm blocks of the reference without a second pass over the tensor."""
    return conv_call(x, weight, nbr, bias, out, relu, False, residual, ln=(ln_weight, ln_bias, ln_eps, post_relu))[0]


def affine_rows(x, scale, shift, residual=None, relu=False, out=None):
    """out = [relu]( x * scale + shift [+ residual] ): a BatchNorm whose statistics its producer finished; out may be x"""
    n, c = x.shape
    out = _rows_out(x, out)
    _lib.check(_lib.load().eprecon_affine_rows_async(
        _lib.ptr(x), n, c, _ld(x), _lib.ptr(scale), _lib.ptr(shift), *_res(residual), int(relu), _lib.ptr(out), _ld(out),
        _lib.current_stream()), "eprecon_affine_rows_async")
    return out


def conv_stats(x, weight, nbr=None, in_affine=None, out=None, bias=None):
    """Convolution whose epilogue also writes the per-workgroup BatchNorm summaries of its output
    (descriptor entry point: any kernel of the family may be chosen).  in_affine = (scale, shift, relu): the
    producer's pending BatchNorm applied while gathering.  Returns (out, partial).  An empty list launches nothing."""
    rows = x.shape[0] if nbr is None else nbr.shape[1]
    return conv_call(x, weight, nbr, bias, out, in_affine=in_affine, stats=True, launch=rows > 0)[:2]


def bn_affine(partial, gamma, beta, eps, out=None):
    """summaries -> the BatchNorm in affine form (scale, shift), to be applied by a consumer on load; out: the (scale, shift)
    slices to fill"""
    c = partial.shape[2]
    nblk, ld = summary_layout(partial)
    scale, shift = torch.empty((2, c), dtype=torch.float32, device=partial.device) if out is None else out
    _lib.check(_lib.load().eprecon_batchnorm_finalize_affine_async(
        partial.data_ptr(), nblk, ld, c, _lib.ptr(gamma), _lib.ptr(beta), float(eps), scale.data_ptr(), shift.data_ptr(),
        _lib.current_stream()), "eprecon_batchnorm_finalize_affine_async")
    return scale, shift


def batchnorm_apply_partials(x, partial, gamma=None, beta=None, eps=1e-5, residual=None, relu=False, out=None,
                             res_affine=None):
    """second half of the train-mode BatchNorm from producer-side summaries (conv_stats);
    res_affine = (scale, shift): the residual carries a pending BatchNorm of its own, applied on load"""
    lib = _lib.load()
    n, c = x.shape
    assert partial.shape[1:] == (3, c)
    nblk, ld = summary_layout(partial)
    out = _rows_out(x, out)
    # mean / var scratch is a per-call buffer (not the shared grow-only workspace): independent branches
    # of the 2D stack run concurrently on several streams
    ws = torch.empty((lib.eprecon_batchnorm_apply_workspace_bytes(c),), dtype=torch.uint8, device=x.device)
    res_scale, res_shift = (None, None) if res_affine is None else res_affine[:2]
    _lib.check(lib.eprecon_batchnorm_apply_partials_async(
        _lib.ptr(x), n, c, _ld(x), _lib.ptr(partial), nblk, ld, _lib.ptr(gamma), _lib.ptr(beta), float(eps), *_res(residual),
        _lib.ptr(res_scale), _lib.ptr(res_shift), int(relu), _lib.ptr(out), _ld(out), None, None, _lib.ptr(ws), ws.numel(),
        _lib.current_stream()), "eprecon_batchnorm_apply_partials_async")
    return out


def batchnorm_train(x, gamma=None, beta=None, eps=1e-5, residual=None, relu=False, out=None):
    """train-mode BatchNorm over all rows (+ optional residual add and ReLU); out may be x"""
    lib = _lib.load()
    n, c = x.shape
    out = _rows_out(x, out)
    ws = _lib.workspace(lib.eprecon_batchnorm_workspace_bytes(n, c), x.device)
    _lib.check(lib.eprecon_batchnorm_train_async(
        _lib.ptr(x), n, c, _ld(x), _lib.ptr(gamma), _lib.ptr(beta), float(eps), *_res(residual), int(relu), _lib.ptr(out),
        _ld(out), None, None, _lib.ptr(ws), ws.numel(), _lib.current_stream()), "eprecon_batchnorm_train_async")
    return out


def rowwise_layernorm(x, gamma=None, beta=None, eps=1e-5, residual=None, pre_relu=False, post_relu=False,
                      out=None):
    """y = [relu]( LN( [relu](x) [+ residual] ) * gamma + beta ) per row; out may be x"""
    n, c = x.shape
    out = _rows_out(x, out)
    _lib.check(_lib.load().eprecon_rowwise_layernorm_async(
        _lib.ptr(x), n, c, _ld(x), *_res(residual), _lib.ptr(gamma), _lib.ptr(beta), float(eps), int(pre_relu), int(post_relu),
        _lib.ptr(out), _ld(out), _lib.current_stream()), "eprecon_rowwise_layernorm_async")
    return out


# ------------------------------------------------------------------------------------------------
# the per-voxel heads (Linear4xTrans) as one launch: csrc/heads.hip
# ------------------------------------------------------------------------------------------------
def _pack_mlp_weight(wt):
    """Wt f32[K][M] (in x out) -> f32[ceil(M/16)][ceil(K/16)][64][4] in the operand order of eprecon_mlp4x_async:
    block (t, c), lane 16 q + m, component i = Wt[16 c + 4 q + i][16 t + m]"""
    k, m = wt.shape
    kc, mt = (k + 15) // 16, (m + 15) // 16
    w = torch.zeros((16 * kc, 16 * mt), dtype=torch.float32, device=wt.device)
    w[:k, :m] = wt
    return w.view(kc, 4, 4, mt, 16).permute(3, 0, 1, 4, 2).contiguous().view(-1)


def _pad16(v, n=None):
    n = v.shape[0] if n is None else n
    out = torch.zeros(((n + 15) // 16 * 16,), dtype=torch.float32, device=v.device)
    out[:v.shape[0]] = v
    return out


def mlp4x_supported(channels, out_channels):
    return bool(_lib.load().eprecon_mlp4x_supported(int(channels), int(out_channels)))


def pack_mlp4x(mod):
    """the parameters of a Linear4xTrans in the kernel's operand order, ONE flat buffer (cached: weight_cache)
    -> dict name -> tensor view"""
    l1, n1, l2, n2, l3 = mod.linear1, mod.norm1, mod.linear2, mod.norm2, mod.linear3

    def build():
        with torch.no_grad():
            parts = {"w1": _pack_mlp_weight(l1.weight.t()), "b1": _pad16(l1.bias), "g1": _pad16(n1.weight), "be1": _pad16(n1.bias),
                     "w2": _pack_mlp_weight(l2.weight.t()), "b2": _pad16(l2.bias), "g2": _pad16(n2.weight), "be2": _pad16(n2.bias),
                     "w3": _pack_mlp_weight(l3.weight.t()), "b3": _pad16(l3.bias)}
            flat = torch.cat([v for v in parts.values()])        # (every part is a multiple of 16 floats: 16-byte aligned views)
            views, off = {}, 0
            for name, v in parts.items():
                views[name] = flat[off:off + v.numel()]
                off += v.numel()
        return views
    return weight_cache.derived(mod, "sparse.pack_mlp4x", (l1.weight, l1.bias, n1.weight, n1.bias, l2.weight, l2.bias, n2.weight,
                                                           n2.bias, l3.weight, l3.bias), build)


def mlp4x(mods, x, outs=None):
    """y_h = Linear4xTrans_h(x) for the 1 or 2 modules `mods` of equal shape (TSDF and occupancy heads share their input rows):
    one launch.  x f32[n, >= C] (row pitch free), -> list of f32[n, C_out]"""
    lib = _lib.load()
    m0 = mods[0]
    c, cout = m0.linear1.in_features, m0.linear3.out_features
    n = x.shape[0]
    assert x.dtype == torch.float32 and x.stride(1) == 1 and x.shape[1] >= c and 1 <= len(mods) <= 2
    d = _lib.Mlp4xDesc()
    d.x, d.ld_x, d.n = x.data_ptr(), x.stride(0), n
    d.channels, d.out_channels, d.heads, d.residual = c, cout, len(mods), int(m0.use_residual)
    d.eps1, d.eps2 = float(m0.norm1.eps), float(m0.norm2.eps)
    if outs is None:
        outs = [torch.empty((n, cout), dtype=torch.float32, device=x.device) for _ in mods]
    keep = []
    for h, (mod, y) in enumerate(zip(mods, outs)):
        assert mod.linear1.in_features == c and mod.linear3.out_features == cout
        pk = pack_mlp4x(mod)
        keep.append(pk)
        hd = d.head[h]
        for name in ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "w3", "b3"):
            setattr(hd, name, pk[name].data_ptr())
        hd.y, hd.ld_y = y.data_ptr(), y.stride(0)
    _lib.check(lib.eprecon_mlp4x_async(ctypes.byref(d), _lib.current_stream()), "eprecon_mlp4x_async")
    return outs
