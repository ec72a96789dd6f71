"""Gradient clipping and Adam as this project's own launches (csrc/optim.hip) — the last stage of an optimisation step,
main.py:308-310 of the reference:

    opt = FusedAdam(model.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=0)
    loss.backward()
    norm = opt.clip_and_step(max_norm=1.0)      # device scalar: the gradients' global L2 norm before clipping
    opt.zero_grad()

clip_and_step = torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.Adam.step() + sparse.repack_registered(),
in three launches whatever the number of parameters (four with finish="launch") and without a host read.  The gradients' sum of squares is
accumulated in double and reduced in a fixed order (no atomics): a step is bit-identical from run to run.  The clipped
gradients are NOT written back: after the step .grad holds the unclipped values.

`state` holds torch's keys and dtypes (step: f32 scalar on the host, exp_avg, exp_avg_sq), so state_dict() and
load_state_dict() interchange with torch.optim.Adam in both directions.
"""
import ctypes

import numpy as np
import torch

from . import _lib

CHUNK = 4096          # floats a workgroup owns at most: a 27*96*96 weight spreads over 61 workgroups, a bias costs one
N_SCALAR_SLOTS = 4    # pinned staging buffers of the per-step scalars (and the tables, when they change), used in turn

SEGMENT_DTYPE = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8")])
CHUNK_DTYPE = np.dtype([("segment", "<i4"), ("start", "<i4"), ("count", "<i4"), ("flags", "<i4")])
assert SEGMENT_DTYPE.itemsize == ctypes.sizeof(_lib.AdamSegment) and CHUNK_DTYPE.itemsize == ctypes.sizeof(_lib.AdamChunk)


def build_chunk_table(sizes, pointers, chunk=CHUNK):
    """Host only.  sizes[s]: floats of segment s; pointers[s] = (param, grad, exp_avg, exp_avg_sq) addresses of its first
    element.  -> CHUNK_DTYPE array: the segments in order, each cut at multiples of `chunk` from its own start, with the
    alignment flags of include/eprecon_hip.h (a chunk start is 16-byte aligned exactly when the segment's is)."""
    assert chunk > 0 and chunk % 4 == 0
    n = np.asarray(sizes, dtype=np.int64).reshape(-1)
    ptrs = np.asarray(pointers, dtype=np.uint64).reshape(-1, 4)
    bad = np.flatnonzero((n <= 0) | (n >= 2 ** 31))
    if bad.size:
        raise ValueError(f"segment {int(bad[0])}: {int(n[bad[0]])} floats (1 .. 2^31 - 1 supported)")
    aligned = (ptrs % np.uint64(16)) == 0
    flags = np.where(aligned.all(axis=1), _lib.ADAM_ALL_ALIGNED, 0) | np.where(aligned[:, 1], _lib.ADAM_GRAD_ALIGNED, 0)
    counts = (n + chunk - 1) // chunk
    first = np.cumsum(counts) - counts                       # a segment's first chunk
    segment = np.repeat(np.arange(len(n), dtype=np.int64), counts)
    table = np.zeros(int(counts.sum()), dtype=CHUNK_DTYPE)
    start = (np.arange(len(table), dtype=np.int64) - first[segment]) * chunk
    table["segment"], table["start"], table["count"], table["flags"] = segment, start, np.minimum(chunk, n[segment] - start), flags[segment]
    return table


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (amsgrad off, maximize off) over ONE parameter group of fp32 device tensors.
    finish: "launch" — a one-workgroup launch sums the chunks' partial sums of squares; "resum" — every workgroup of the
    update launch sums them itself.  The same bits either way; DESIGN.md 7ae has the timing behind the default."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, finish="resum"):
        if finish not in ("launch", "resum"):
            raise ValueError(f"finish={finish!r}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        assert len(self.param_groups) == 1, "FusedAdam takes one parameter group"
        self.finish = finish
        self._entries = None       # per parameter of the group: [parameter, exp_avg address, exp_avg_sq address]
        self._step_store = None    # f32[parameters] on the host: every state's 'step' is a 0-d view of its element
        self._tables = None        # the device tables of the last step and what they were built from
        self._slots = []           # [pinned staging buffer, event of the last copy out of it], used in turn
        self._slot = 0
        self.launches = 0          # of the last step, the weight repack included
        self._bind()               # (a parameter this class cannot take raises here, by name)

    def _bind(self):
        """validate the group's parameters and tie the states that exist to the per-step bookkeeping"""
        group = self.param_groups[0]
        names = group.get("param_names")
        self._entries = []
        self._step_store = torch.zeros(len(group["params"]), dtype=torch.float32)
        for i, p in enumerate(group["params"]):
            name = names[i] if names else i
            if p.requires_grad and (p.dtype != torch.float32 or not p.is_cuda):
                raise ValueError(f"FusedAdam: parameter {name!r} of shape {tuple(p.shape)} is {p.dtype} on {p.device}: "
                                 "fp32 tensors on the GPU only")
            if p.requires_grad and not p.is_contiguous():
                raise ValueError(f"FusedAdam: parameter {name!r} of shape {tuple(p.shape)} is not contiguous")
            entry = [p, None, None]
            st = self.state.get(p)
            if st:
                self._step_store[i] = float(st["step"])
                st["step"] = self._step_store[i]
                entry[1:] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            self._entries.append(entry)
        self._tables = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        assert len(self.param_groups) == 1, "FusedAdam takes one parameter group"
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay"):
            raise ValueError("FusedAdam: amsgrad, maximize and decoupled_weight_decay are not implemented")
        self._bind()

    def _stage(self, nbytes):
        """a pinned buffer of at least nbytes whose last copy to the device has run"""
        if len(self._slots) < N_SCALAR_SLOTS:
            self._slots.append([torch.empty(0, dtype=torch.uint8, pin_memory=True), None])
        slot = self._slots[self._slot % len(self._slots)]
        self._slot += 1
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0].numel() < nbytes:
            slot[0] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return slot

    @torch.no_grad()
    def clip_and_step(self, max_norm=1.0):
        """-> the gradients' global L2 norm as a device scalar (None when max_norm is None or no parameter has a gradient)"""
        group = self.param_groups[0]
        beta1, beta2 = group["betas"]
        if len(self._entries) != len(group["params"]):
            self._bind()
        index, p_ptrs, g_ptrs, grads = [], [], [], []
        for i, entry in enumerate(self._entries):
            p = entry[0]
            g = p.grad
            if g is None or not p.requires_grad:
                continue                                   # skipped whole, as torch does: no decay, no step count
            if not g.is_contiguous():
                g = g.contiguous()                         # (for this step; the copy lives until the launches are queued)
            if entry[1] is None:
                st = self.state[p]
                st["step"] = self._step_store[i]
                st["exp_avg"] = torch.zeros(p.shape, dtype=p.dtype, device=p.device)
                st["exp_avg_sq"] = torch.zeros(p.shape, dtype=p.dtype, device=p.device)
                entry[1:] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            index.append(i)
            p_ptrs.append(p.data_ptr())
            g_ptrs.append(g.data_ptr())
            grads.append(g)
        self.launches = 0
        if not index:
            return None
        device = self._entries[index[0]][0].device
        key = (index, p_ptrs, g_ptrs)
        nseg = len(index)
        scalar_bytes = (8 * nseg + 15) // 16 * 16
        rebuild = self._tables is None or self._tables["key"] != key
        if rebuild:
            names = group.get("param_names")
            for i, g in zip(index, grads):
                p = self._entries[i][0]
                if g.dtype != torch.float32 or g.device != p.device or g.is_sparse or p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError(f"FusedAdam: parameter {names[i] if names else i!r}: gradient {g.dtype} on {g.device}, "
                                     f"parameter {p.dtype} (contiguous: {p.is_contiguous()}): dense fp32 on the parameter's GPU only")
            segs = np.zeros(nseg, dtype=SEGMENT_DTYPE)
            segs["param"], segs["grad"] = p_ptrs, g_ptrs
            segs["exp_avg"] = [self._entries[i][1] for i in index]
            segs["exp_avg_sq"] = [self._entries[i][2] for i in index]
            sizes = [self._entries[i][0].numel() for i in index]
            chunks = build_chunk_table(sizes, segs.view(np.uint64).reshape(nseg, 4))
            total = scalar_bytes + segs.nbytes + chunks.nbytes
            self._tables = {"key": key, "index": np.asarray(index), "floats": int(sum(sizes)), "nchunks": len(chunks),
                            "segs": segs.view(np.uint8), "chunks": chunks.view(np.uint8),
                            # [per-segment scalars | segment table | chunk table], every part 16-byte aligned
                            "dev": torch.empty(total, dtype=torch.uint8, device=device),
                            "partials": torch.empty(len(chunks), dtype=torch.float64, device=device)}
        tab = self._tables

        # Every parameter's own bias corrections, formed in float64 (torch/optim/adam.py does so in Python floats), and, when
        # they changed, the tables: one non-blocking copy out of a pinned buffer that is not written again before it has run.
        store = self._step_store.numpy()
        store[tab["index"]] += 1.0
        steps = store[tab["index"]].astype(np.float64)
        scal = np.empty((nseg, 2), dtype=np.float32)
        scal[:, 0] = group["lr"] / (1.0 - np.power(beta1, steps))
        scal[:, 1] = np.sqrt(1.0 - np.power(beta2, steps))
        nbytes = tab["dev"].numel() if rebuild else 8 * nseg
        slot = self._stage(nbytes)
        host = slot[0].numpy()
        host[:8 * nseg] = scal.reshape(-1).view(np.uint8)
        if rebuild:
            host[scalar_bytes:scalar_bytes + tab["segs"].size] = tab["segs"]
            host[scalar_bytes + tab["segs"].size:nbytes] = tab["chunks"]
        tab["dev"][:nbytes].copy_(slot[0][:nbytes], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()

        lib = _lib.load()
        stream = _lib.current_stream()
        base = tab["dev"].data_ptr()
        segs_dev, chunks_dev, nchunks = base + scalar_bytes, base + scalar_bytes + tab["segs"].size, tab["nchunks"]
        partials = tab["partials"].data_ptr()
        norm_coef = None
        clip = max_norm is not None
        if clip:
            norm_coef = torch.empty(2, dtype=torch.float32, device=device)
            _lib.check(lib.eprecon_grad_sqsum_async(segs_dev, chunks_dev, nchunks, partials, stream), "eprecon_grad_sqsum_async")
            self.launches += 1
            if self.finish == "launch":
                _lib.check(lib.eprecon_grad_norm_finish_async(partials, nchunks, float(max_norm), norm_coef.data_ptr(), stream),
                           "eprecon_grad_norm_finish_async")
                self.launches += 1
        resum = clip and self.finish == "resum"
        _lib.check(lib.eprecon_adam_update_async(segs_dev, chunks_dev, nchunks, base, 1.0 - beta1, beta2, 1.0 - beta2, group["eps"],
                                                 group["weight_decay"], partials if resum else None,
                                                 float(max_norm) if clip else 0.0, _lib.ptr(norm_coef), stream),
                   "eprecon_adam_update_async")
        self.launches += 1
        # the launch wrote through raw pointers: tell autograd, whose version counters the layers' weight caches key on
        torch.autograd.graph.increment_version([self._entries[i][0] for i in index])
        # every weight has changed: all operand-order copies rebuilt by one launch
        from .sparse import repack_registered
        self.launches += 1 if repack_registered() else 0
        return norm_coef[0] if clip else None

    def step(self, closure=None):
        """Adam without clipping"""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.clip_and_step(max_norm=None)
        return loss

    def bytes_moved(self):
        """algorithmic bytes of the last clip_and_step's launches: the norm reads the gradients once; the update reads
        parameter, gradient and both moments and writes parameter and both moments"""
        return 0 if self._tables is None else (4 + 28) * self._tables["floats"]
