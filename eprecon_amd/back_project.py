"""Multi-view back-projection — host-side mirror of the reference operators, running on
libeprecon_hip.so (csrc/back_project.hip).

  back_project(...)        same signature / return as ops/back_project.py:5-80
  Back_Project.forward     same signature / return as models/occupancy_initialization.py:189-261
  view_variance(...)       the sampling + mean/variance block of
                           Occupancy_Initialization.forward (models/occupancy_initialization.py:79-128)

"Nothing to do" is signalled by returning None exactly where the reference does.  Device memory,
streams and the host sync on n_valid are PyTorch's; everything else is the HIP library.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib

MODE_MEAN, MODE_MEAN_DEPTH, MODE_VARIANCE = 0, 1, 2
LAYOUT_NCHW, LAYOUT_NHWC = 0, 1


def mark_dense(coords, dims, interval, batch=1):
    """Tag `coords` (int32[B*Dx*Dy*Dz, 4]) as the dense x-major raster of a dims grid at spacing `interval` — what
    generate_grids.dense_coords / ops/generate_grids.py:3-10 produce.  A plain attribute (lost by any op that makes a new
    tensor); nothing in the library branches on it since the brick kernel of round 2 was removed."""
    coords._eprecon_dense = (tuple(int(d) for d in dims), int(interval), int(batch))
    return coords


def dense_rank_buffer(coords, dims, interval):
    """-> an int32[N + 1] device buffer for the rank volume (`rank_out` of run / run_async / view_variance) when `coords` is
    tagged as the one-element dense raster of exactly this grid (mark_dense) and EPRECON_INIT_GLUE is on, else None: the
    gather then writes entry -> output row (or -1) while it compacts, and sparse.DenseMap has nothing left to build"""
    tag = getattr(coords, "_eprecon_dense", None)
    want = (tuple(int(d) for d in dims), int(interval), 1)
    if tag != want or not coords.is_cuda or coords.shape[0] != want[0][0] * want[0][1] * want[0][2]:
        return None
    if not _lib.load().eprecon_init_glue():
        return None
    return torch.empty(coords.shape[0] + 1, dtype=torch.int32, device=coords.device)


def _prep_feats(feats):
    """feats: [V, B, C, H, W] (logical shape).  Channels-last storage (stride of C == 1) is passed
    through without a copy; anything else is made NCHW-contiguous."""
    v, b, c, h, w = feats.shape
    if feats.dtype != torch.float32:
        feats = feats.float()
    want = (b * h * w * c, h * w * c, 1, w * c, c)
    if all(sz == 1 or st == ws for sz, st, ws in zip(feats.shape, feats.stride(), want)):
        return feats, LAYOUT_NHWC  # (strides of size-1 dimensions are irrelevant)
    return feats.contiguous(), LAYOUT_NCHW


def _prep_inputs(coords, origin, krcam, v, b, dev):
    """-> (coords int32[N, 4], origin f32[B, 3], krcam f32[V, B, 4, 4]), contiguous and on `dev`, for V views of B batch elements"""
    _lib.need_device(dev)
    coords_i = (coords if coords.dtype == torch.int32 else coords.to(torch.int32)).contiguous()
    origin_f = origin.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    krcam_f = krcam.to(device=dev, dtype=torch.float32).contiguous()
    assert krcam_f.shape == (v, b, 4, 4) and origin_f.shape[0] == b
    return coords_i, origin_f, krcam_f


def _alloc_outputs(n, v, c, mode, want_grid, want_mean, dev, count=None):
    """the output tensors of one call, sized for n valid rows (count: the count half's, when there was one)"""
    f32 = dict(dtype=torch.float32, device=dev)
    return {"feats": torch.empty((n, c + 1 if mode == MODE_MEAN_DEPTH else c), **f32),
            "coords": torch.empty((n, 4), dtype=torch.int32, device=dev),
            "count": torch.empty((n,), **f32) if count is None else count,
            "mean": torch.empty((n, c), **f32) if want_mean else None,
            "grid": torch.empty((v * n * 2,), **f32) if want_grid else None,
            "mask": torch.empty((v * n,), dtype=torch.uint8, device=dev) if want_grid else None}


def _set_outputs(d, t, rank=None, phase=0):
    """the outputs of a _lib.BpCall by field name; t: _alloc_outputs(...) or, for a count half, {"count": ...}; rank: `rank_out`"""
    if rank is not None:
        assert d.batch == 1 and rank.dtype == torch.int32 and rank.is_contiguous() and rank.numel() == d.n + 1
    d.phase, d.count, d.rank = phase, _lib.ptr(t.get("count")), _lib.ptr(rank)
    d.out_feats, d.out_mean, d.out_coords = _lib.ptr(t.get("feats")), _lib.ptr(t.get("mean")), _lib.ptr(t.get("coords"))
    d.out_grid, d.out_mask = _lib.ptr(t.get("grid")), _lib.ptr(t.get("mask"))
    return d


def _call(inputs, feats, shape, layout, voxel_size, min_view, mode, t, n_valid_dev, ws, rank=None, phase=0, d=None):
    """-> a _lib.BpCall (d: the one to fill) of these arguments, by field name.  inputs: _prep_inputs(...), or None for a level
    without a list; t, rank, phase: _set_outputs.  The caller keeps every tensor alive: the descriptor holds plain addresses."""
    d = _lib.BpCall() if d is None else d
    if inputs is not None:
        d.coords, d.origin, d.krcam = (_lib.ptr(x) for x in inputs)
    d.n, d.voxel_size, d.feats, d.feats_layout = 0 if inputs is None else inputs[0].shape[0], float(voxel_size), _lib.ptr(feats), layout
    d.n_views, d.batch, d.channels, d.height, d.width = shape
    d.min_view, d.mode, d.n_valid_dev, d.workspace, d.workspace_bytes = int(min_view), mode, _lib.ptr(n_valid_dev), _lib.ptr(ws), ws.numel()
    return _set_outputs(d, t, rank, phase)


def _result(t, v, n_valid, per_batch, want_grid, want_mean, sliced=True):
    """what run() returns, from the tensors of _alloc_outputs; sliced=False: every row is valid (n_valid == N)"""
    cut = (lambda x, k=1: x[:k * n_valid]) if sliced else (lambda x, k=1: x)
    res = {"feats": cut(t["feats"]), "coords": cut(t["coords"]), "count": t["count"], "n_valid": n_valid,
           "n_valid_per_batch": per_batch}
    if want_grid:
        res["grid"] = cut(t["grid"], v * 2).view(v, n_valid, 2)
        res["mask"] = cut(t["mask"], v).view(v, n_valid).bool()
    if want_mean:
        res["mean"] = cut(t["mean"])
    return res


class PendingBackProject:
    """A back-projection whose kernels are queued on a stream; `result()` waits for the valid counts
    (pinned host copy + event) and returns what `run()` returns.  Lets independent levels be issued
    back to back without a host round trip between them."""

    def __init__(self, tensors, n, v, c, batch, min_valid_per_batch, read, want_grid, want_mean):
        self._t, self._n, self._v, self._c, self._batch = tensors, n, v, c, batch
        self._min_valid, self._read = min_valid_per_batch, read
        self._want_grid, self._want_mean = want_grid, want_mean

    def result(self):
        return self.result_from(self._read.result())     # (deferred checks pending at queue time rode along: _lib.PinnedRead)

    def result_from(self, counts):
        """counts: the 1 + B values of `n_valid_dev` as read by the caller (hold_read: together with other counts)"""
        if any(x < self._min_valid for x in counts[1:]):
            return None  # reference: `return None`
        return _result(self._t, self._v, counts[0], counts[1:], self._want_grid, self._want_mean)


class CountedBackProject:
    """the count half of a back-projection (count_async), to be handed to run_async(counted=...) with the maps"""

    def __init__(self, shape, inputs, call, count, n_valid_dev, ws, stream, mailbox=None, early=False):
        self.shape, self.inputs, self.call, self.count = shape, inputs, call, count      # call: the _lib.BpCall that was queued
        self.n_valid_dev, self.ws, self.stream = n_valid_dev, ws, stream
        # mailbox: the _lib.MailboxRead whose slot `call` carries, or None (the counts are copied); early: the count half has
        # published into it already (count_async), so the gather half is handed none
        self.mailbox, self.early = mailbox, early


def count_async(coords, origin, voxel_size, feats_shape, krcam, min_view, mode=MODE_MEAN, stream=None):
    """Queue the half of a back-projection that needs no maps — visible views per voxel, valid totals per tile — for
    channels-last maps of logical shape feats_shape = (V, B, C, H, W) that may not exist yet.  stream: another stream to
    queue it on behind the work queued so far (run_async waits for it); buffers are allocated on the current stream.
    Same launches as the one-call form (eprecon_bp_call::phase)."""
    lib = _lib.load()
    dev = coords.device
    shape = v, b, c, h, w = tuple(int(x) for x in feats_shape)
    inputs = _prep_inputs(coords, origin, krcam, v, b, dev)
    n = coords.shape[0]
    count = torch.empty((n,), dtype=torch.float32, device=dev)
    n_valid_dev = torch.empty((1 + b,), dtype=torch.int32, device=dev)
    # a buffer of the call's own, not the stream's grow-only scratch: it has to survive until the gather half has run
    ws = torch.empty((lib.eprecon_back_project_workspace_bytes(n, b, v, c, h, w, LAYOUT_NHWC),), dtype=torch.uint8, device=dev)

    call = _call(inputs, None, shape, LAYOUT_NHWC, voxel_size, min_view, mode, {"count": count}, n_valid_dev, ws, phase=1)
    # The counts are final once the count has run.  With a count mailbox the count half publishes them itself (one more
    # one-workgroup launch, on `stream`), and the host has them long before the gather half is even queued.
    mb = _lib.mailbox_read(1 + b) if n > 0 else None
    if mb is not None:
        call.counts_host, call.counts_seq = mb.payload_dev, mb.seq

    def queue():
        _lib.check(lib.eprecon_back_project_call_async(ctypes.byref(call), _lib.current_stream()), "eprecon_back_project_call_async")
        if mb is not None:
            mb.queued(n_valid_dev)
    if stream is None:
        queue()
    else:
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            queue()
    return CountedBackProject(shape, inputs + (float(voxel_size), int(min_view), mode), call, count, n_valid_dev, ws, stream,
                              mailbox=mb, early=mb is not None)


class PreparedMaps:
    """a level of prepare_levels_async without a list: `nhwc` is its maps [V, B, C, H, W] stored channels-last (inside `ws`
    for NCHW input), valid for work that waits for `stream` (None: the stream the launch was queued on)"""

    def __init__(self, nhwc, ws, stream):
        self.nhwc, self.ws, self.stream = nhwc, ws, stream


class PendingLevels:
    """The gather halves of prepare_levels_async's levels — run_async(..., hd.nhwc, ..., hold_read=True, counted=hd) for every
    handle hd — behind ONE read of their counts: a count mailbox slot per level when the handles carry them (nothing is
    queued), else one pinned read of the tensor the counts are slices of (queued here: behind the last gather on the current
    stream; the deferred checks pending there ride along).  results() -> what every PendingBackProject.result() would
    have returned, one blocking read in all."""

    def __init__(self, pends, handles):
        self._pends, self._offsets, self._host = list(pends), [hd.n_valid_off for hd in handles], None
        assert len(self._pends) == len(self._offsets) and all(hd.n_valid_all is handles[0].n_valid_all for hd in handles)
        assert all(p.n_valid_dev.data_ptr() == hd.n_valid_dev.data_ptr() for p, hd in zip(self._pends, handles))
        self._slots = [hd.mailbox for hd in handles]        # (prepare_levels_async: every level has one, or none has)
        self._read = None if all(m is not None for m in self._slots) else _lib.PinnedRead(handles[0].n_valid_all)

    def results(self):
        if self._host is None and self._read is None:
            _lib.count_host_read()
            self._host = [None] * (self._offsets[-1] + 1 + self._pends[-1]._batch)
            for m, p, o in zip(self._slots, self._pends, self._offsets):
                self._host[o:o + 1 + p._batch] = m.wait()
        elif self._host is None:
            self._host = self._read.result()
        return [p.result_from(self._host[o:o + 1 + p._batch]) for p, o in zip(self._pends, self._offsets)]


def prepare_levels_async(levels, stream=None):
    """Queue the first halves of up to four back-projections as ONE launch (eprecon_back_project_prepare_levels_async): per level
    the re-layout of NCHW maps and the count.  levels: tuples (coords, origin, voxel_size, feats, krcam, min_view[, mode]) as
    run_async takes them; coords None: the level's maps are re-laid out only.  stream: as for count_async.  Workspaces and counts
    are the call's own; the counters of all levels are slices of one int32 tensor (`.n_valid_all`, from `.n_valid_off`).
    -> one handle per level: a CountedBackProject hd whose `.nhwc` is the level's maps stored channels-last (inside its
    workspace for NCHW input) — the gather half is run_async(coords, origin, voxel_size, hd.nhwc, krcam, min_view, mode,
    counted=hd) — or a PreparedMaps for a level without a list.
    EPRECON_BP_LEVELS=0: the same work, one launch per level."""
    lib = _lib.load()
    if not 1 <= len(levels) <= 4:
        raise _lib.EpreconError("prepare_levels_async takes one to four levels")
    dev = levels[0][3].device
    rows = []
    for lv in levels:
        coords, origin, voxel_size, feats, krcam, min_view = lv[:6]
        mode = lv[6] if len(lv) > 6 else MODE_MEAN
        shape = tuple(int(x) for x in feats.shape)
        feats_c, layout = _prep_feats(feats)
        inputs = None if coords is None else _prep_inputs(coords, origin, krcam, shape[0], shape[1], dev)
        rows.append((shape, feats_c, layout, inputs, float(voxel_size), int(min_view), mode))
    n_valid_all = torch.empty((sum(1 + r[0][1] for r in rows if r[3] is not None),), dtype=torch.int32, device=dev)
    descs = (_lib.BpCall * len(rows))()
    # a count mailbox slot per level with a list, or none at all (an empty list has no publisher; PendingLevels reads either
    # every level's slot or the one tensor)
    listed = [r for r in rows if r[3] is not None]
    slots = [_lib.mailbox_read(1 + r[0][1]) if r[3][0].shape[0] > 0 else None for r in listed]
    slots = iter(slots if all(m is not None for m in slots) else [None] * len(listed))
    handles, off = [], 0
    for d, (shape, feats_c, layout, inputs, voxel_size, min_view, mode) in zip(descs, rows):
        v, b, c, h, w = shape
        n = 0 if inputs is None else inputs[0].shape[0]
        # buffers of the call's own, not the stream's grow-only scratch: they have to survive until the gather halves have run
        ws = torch.empty((lib.eprecon_back_project_workspace_bytes(n, b, v, c, h, w, layout),), dtype=torch.uint8, device=dev)
        count = None if inputs is None else torch.empty((n,), dtype=torch.float32, device=dev)
        n_valid_dev = None if inputs is None else n_valid_all[off:off + 1 + b]
        _call(inputs, feats_c, shape, layout, voxel_size, min_view, mode, {"count": count}, n_valid_dev, ws, d=d)
        nhwc = feats_c
        if layout == LAYOUT_NCHW:
            o = lib.eprecon_back_project_workspace_maps_offset(n, b)
            nhwc = ws[o:o + 4 * v * b * c * h * w].view(torch.float32).view(v, b, h, w, c).permute(0, 1, 4, 2, 3)
        if inputs is None:
            handles.append(PreparedMaps(nhwc, (ws, feats_c), stream))
            continue
        mb = next(slots)
        if mb is not None:      # (published by the level's gather half, or by the scan launch of a long list, queued here)
            d.counts_host, d.counts_seq = mb.payload_dev, mb.seq
        hd = CountedBackProject(shape, inputs + (voxel_size, min_view, mode), d, count, n_valid_dev, ws, stream, mailbox=mb)
        hd.nhwc, hd.feats, hd.n_valid_all, hd.n_valid_off = nhwc, feats_c, n_valid_all, off
        handles.append(hd)
        off += 1 + b

    def queue():
        _lib.check(lib.eprecon_back_project_prepare_levels_async(ctypes.byref(descs), len(rows), _lib.current_stream()),
                   "eprecon_back_project_prepare_levels_async")
        for hd in handles:
            if getattr(hd, "mailbox", None) is not None:
                hd.mailbox.queued(hd.n_valid_dev)
    if stream is None:
        queue()
    else:
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            queue()
    return handles


def run_async(coords, origin, voxel_size, feats, krcam, min_view, mode=MODE_MEAN, min_valid_per_batch=1,
              want_grid=False, want_mean=False, hold_read=False, extra_words=0, rank_out=None, counted=None):
    """Queue the back-projection on the current stream and return a PendingBackProject.
    hold_read: no host copy of the counts is queued — the caller reads `.n_valid_dev` itself, together with whatever else it
    queued on the device count `.n_valid_dev[0:1]` of the compacted rows `.coords_all` (torchsparse_utils.SpvcnnPrefetch), and
    hands the values to result_from().  extra_words: `.n_valid_dev` gets that many more int32 behind the 1 + B counts (the caller's
    own counts, so that one tensor is read).  rank_out: dense_rank_buffer(...)'s buffer, or None.
    counted: count_async(...)'s result for these very arguments — only the gather half is queued here."""
    lib = _lib.load()
    dev = feats.device
    shape = v, b, c, h, w = tuple(feats.shape)
    inputs = _prep_inputs(coords, origin, krcam, v, b, dev)
    n = coords.shape[0]
    feats_c, layout = _prep_feats(feats)
    t = _alloc_outputs(n, v, c, mode, want_grid, want_mean, dev, count=None if counted is None else counted.count)
    if counted is not None:
        assert layout == LAYOUT_NHWC and counted.shape == shape and not extra_words
        assert counted.inputs[3:] == (float(voxel_size), int(min_view), mode) and counted.count.shape[0] == n
        inputs, n_valid_dev, ws = counted.inputs[:3], counted.n_valid_dev, counted.ws
        if counted.stream is not None:
            torch.cuda.current_stream(dev).wait_stream(counted.stream)
    else:
        n_valid_dev = torch.empty((1 + b + int(extra_words),), dtype=torch.int32, device=dev)
        ws = _lib.workspace(lib.eprecon_back_project_workspace_bytes(n, b, v, c, h, w, layout), dev)
    # The counts' way to the host: the count mailbox slot the count half took (counted.mailbox), else one taken here unless the
    # caller reads the counts itself (hold_read) or nobody would publish (an empty list); without a slot, a pinned copy.
    mb, early = (counted.mailbox, counted.early) if counted is not None else (None, False)
    if mb is None and not hold_read and n > 0:
        mb = _lib.mailbox_read(1 + b)
    if counted is not None:     # the descriptor of the count half, with the maps and the outputs
        call = _lib.BpCall.from_buffer_copy(counted.call)
        call.feats, call.feats_layout = _lib.ptr(feats_c), layout
        _set_outputs(call, t, rank_out, phase=2)
    else:
        call = _call(inputs, feats_c, shape, layout, voxel_size, min_view, mode, t, n_valid_dev, ws, rank_out)
    # (early: the count half has published already; the gather half writes the same counts to the device and is handed no slot)
    call.counts_host, call.counts_seq = (mb.payload_dev, mb.seq) if mb is not None and not early else (None, 0)
    _lib.check(lib.eprecon_back_project_call_async(ctypes.byref(call), _lib.current_stream()), "eprecon_back_project_call_async")
    if mb is not None and not early:
        mb.queued(n_valid_dev)
    read = None if hold_read else mb if mb is not None else _lib.PinnedRead(n_valid_dev[:1 + b])
    # inputs stay referenced until result(): the kernels may still be reading them
    t["_keep"] = (*inputs, feats_c, n_valid_dev, ws if counted is not None else None)
    pend = PendingBackProject(t, n, v, c, b, int(min_valid_per_batch), read, want_grid, want_mean)
    pend.n_valid_dev, pend.coords_all = n_valid_dev, t["coords"]
    return pend


def run(coords, origin, voxel_size, feats, krcam, min_view, mode=MODE_MEAN, min_valid_per_batch=1,
        want_grid=False, want_mean=False, rank_out=None):
    """Low-level entry: returns None (reference: `return None`) or a dict of device tensors
    {feats [n_valid, C(+1)], coords int32 [n_valid, 4], count f32 [N], n_valid, (grid, mask, mean)}."""
    lib = _lib.load()
    dev = feats.device
    shape = v, b, c, h, w = tuple(feats.shape)
    inputs = _prep_inputs(coords, origin, krcam, v, b, dev)
    n = coords.shape[0]
    feats_c, layout = _prep_feats(feats)
    t = _alloc_outputs(n, v, c, mode, want_grid, want_mean, dev)
    n_valid_dev = torch.empty((1 + b,), dtype=torch.int32, device=dev)
    ws = _lib.workspace(lib.eprecon_back_project_workspace_bytes(n, b, v, c, h, w, layout), dev)
    call = _call(inputs, feats_c, shape, layout, voxel_size, min_view, mode, t, n_valid_dev, ws, rank_out)

    if min_view <= 0 and b == 1 and n >= max(int(min_valid_per_batch), 1):
        # every voxel is valid (the view count is never negative; the one batch element owns all rows): nothing to wait for.
        # The count is still produced on the device and checked with the level's next blocking read (a batch index out of
        # range is the one way a row can drop out).
        _lib.check(lib.eprecon_back_project_call_async(ctypes.byref(call), _lib.current_stream()), "eprecon_back_project_call_async")
        _lib.defer_check(n_valid_dev[0:1], n, "back-projection with min_view <= 0: rows with a batch index out of range")
        return _result(t, v, n, [n], want_grid, want_mean, sliced=False)
    n_valid_host = (ctypes.c_int32 * (1 + b))()
    _lib.count_host_read()
    rc = lib.eprecon_back_project_call(ctypes.byref(call), int(min_valid_per_batch), ctypes.cast(n_valid_host, ctypes.c_void_p),
                                       _lib.current_stream())
    _lib.drain_deferred()          # (the library copied the counts itself: pending checks are verified here, when there are any)
    if not _lib.check(rc, "eprecon_back_project_call"):
        return None
    return _result(t, v, int(n_valid_host[0]), [int(x) for x in n_valid_host[1:]], want_grid, want_mean)


def back_project(coords, origin, voxel_size, feats, KRcam, min_view_number):
    """ops/back_project.py:5-80.  Returns [features f32[N_valid, C+1] (last channel = normalised
    mean depth), coords float32[N_valid, 4], count f32[N]] or None when a batch has no valid voxel."""
    res = run(coords, origin, voxel_size, feats, KRcam, min_view_number, MODE_MEAN_DEPTH)
    if res is None:
        return None
    # the reference concatenates onto torch.empty(0, 4) (float32), so its coords come back as float
    return [res["feats"], res["coords"].to(torch.float32), res["count"]]


def _forward_list(res, coords):
    """Back_Project.forward's return value from run()'s dict: the coordinates come back in the dtype they came in"""
    out_coords = res["coords"] if coords.dtype == torch.int32 else res["coords"].to(coords.dtype)
    return [res["feats"], out_coords, res.get("grid"), res.get("mask"), res["count"]]


class Back_Project(nn.Module):
    """models/occupancy_initialization.py:185-261.  `forward` returns
    [features f32[N_valid, C], coords (input dtype)[N_valid, 4], im_grid, mask, count f32[N]].

    The reference's only caller consumes entries 0, 1 and 4 (models/neucon_network.py:374-378);
    materialising im_grid f32[V, N_valid, 2] and mask bool[V, N_valid] costs 9 extra bytes per
    (view, voxel), so they are produced only when `return_projection` is True, else None."""

    def __init__(self, dim, return_projection=False):
        super().__init__()
        self.return_projection = return_projection

    def forward(self, coords, origin, voxel_size, feats, KRcam, min_view_number):
        if torch.is_grad_enabled() and feats.requires_grad:
            from . import autograd as AG    # training: the gathered features carry the gradient to the image maps
            res = AG.back_project(coords, origin, voxel_size, feats, KRcam, min_view_number, MODE_MEAN)
        else:
            res = run(coords, origin, voxel_size, feats, KRcam, min_view_number, MODE_MEAN,
                      want_grid=self.return_projection)
        return None if res is None else _forward_list(res, coords)


def get_img_feats(coords, origin, voxel_size, feats, KRcam, min_view_number):
    """models/occupancy_initialization.py:264-323 (imported by models/neucon_network.py:20, never called there): the view-mean
    features f32[N_valid, C] of the voxels seen by at least `min_view_number` views — entry 0 of Back_Project.forward; an
    empty [0, C] tensor where the reference's loop would have concatenated nothing."""
    res = run(coords, origin, voxel_size, feats, KRcam, min_view_number, MODE_MEAN, min_valid_per_batch=0)
    if res is None:
        return torch.empty((0, feats.shape[2]), dtype=feats.dtype, device=feats.device)
    return res["feats"]


def forward_behind(module, coords, origin, voxel_size, feats, KRcam, min_view_number, behind):
    """Back_Project.forward with more work queued on the DEVICE count of its valid rows in front of the one host read:
    behind(valid_coords int32[N,4] (first n_valid rows live), n_valid_dev int32[1], extra_out int32[behind.n_extra]) ->
    finish(n_valid, host_extra).  -> (what forward returns, finish(...)'s result | None).  Inference only."""
    pend = run_async(coords, origin, voxel_size, feats, KRcam, min_view_number, MODE_MEAN, want_grid=module.return_projection,
                     hold_read=True, extra_words=behind.n_extra)
    nb = pend.n_valid_dev.numel() - behind.n_extra
    finish = behind(pend.coords_all, pend.n_valid_dev[0:1], pend.n_valid_dev[nb:])
    host = _lib.read_counts(pend.n_valid_dev)
    res = pend.result_from(host[:nb])
    if res is None:
        return None, None
    return _forward_list(res, coords), finish(res["n_valid"], host[nb:])


def view_variance(coords, origin, voxel_size, feats_fused, KRcam, min_view_number, min_valid=1000, rank_out=None):
    """Per-voxel population variance over the visible views of the fused 32-channel maps
    (models/occupancy_initialization.py:79-128).  Returns None when fewer than `min_valid` voxels
    are valid (:107-108), else dict(var, mean, coords, count, n_valid)."""
    if torch.is_grad_enabled() and feats_fused.requires_grad:
        from . import autograd as AG
        res = AG.back_project(coords, origin, voxel_size, feats_fused, KRcam, min_view_number, MODE_VARIANCE,
                              min_valid_per_batch=min_valid, want_mean=True)
    else:
        res = run(coords, origin, voxel_size, feats_fused, KRcam, min_view_number, MODE_VARIANCE,
                  min_valid_per_batch=min_valid, want_mean=True, rank_out=rank_out)
    if res is None:
        return None
    res["var"] = res.pop("feats")
    return res


def to_channels_last(feats):
    """[V, B, C, H, W] -> same logical tensor stored [V, B, H, W, C] with the HIP re-layout kernel,
    for callers that back-project the same maps more than once."""
    lib = _lib.load()
    v, b, c, h, w = feats.shape
    src = feats.float().contiguous()
    dst = torch.empty((v, b, h, w, c), dtype=torch.float32, device=feats.device)
    _lib.check(lib.eprecon_nchw_to_nhwc_async(_lib.ptr(src), _lib.ptr(dst), v * b, c, h * w,
                                               _lib.current_stream()), "eprecon_nchw_to_nhwc_async")
    return dst.permute(0, 1, 4, 2, 3)
