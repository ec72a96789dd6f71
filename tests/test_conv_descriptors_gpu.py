"""What the convolution wrappers hand to the library, call by call, against a record taken before their host path was folded
into one descriptor builder (tests/golden/conv_descs.json; its header names the commit).

The loaded library's eprecon_conv_desc_async and eprecon_sparse_conv_fused_async (and eprecon_sparse_conv_async, the latter
without residual and summaries, which sparse_conv called before the change) are wrapped with Python callables that copy
their arguments and forward them, so every launch still happens.  Per launch the record holds the entry point, every integer
and float field of the descriptor that is not 0, the pointer fields that are not null, the byte offsets of x / out / residual
from the tensors the case passed, the workspace the library wants for the launch and whether the attached one covers it, and
the kernel family that took it (_lib.last_conv_kernel); per wrapper call also the shape and strides of the returned summaries.
(The attached workspace_bytes itself is not in the record: before the change it was the size of a grow-only buffer, which
depends on what ran earlier in the process.  The wide-family case below pins it to the library's count.)

Only the public wrappers are used (sparse.sparse_conv / sparse_conv_fused / sparse_conv_ln / conv_stats, DenseMap,
dense2d.conv_bn_launch), so this file runs on either side of the change:

    python tests/test_conv_descriptors_gpu.py --record <commit> [<file>]      # rewrites the golden file on a GPU

The cases are the smallest shapes on either side of every rule by which a packing (packed_weight / packed_weight16), the dense
grid or a workspace rides along with a launch; the row thresholds are lowered to 1,000 (500 for the short image lists).
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_descs.json")
THRESHOLDS = {"sparse": {"K1_DIRECT_MIN_ROWS": 1000},
              "dense2d": {"DIRECT_2D_MIN_ROWS": 1000, "SHORT_2D_MAX_ROWS": 500, "K1_DIRECT_2D_MIN_ROWS": 1000}}
POSITIONAL = ("x", "n_in", "ld_x", "nbr", "kvol", "n_out", "weight", "cin", "cout", "bias", "residual", "ld_res", "out", "ld_out",
              "relu", "accumulate", "bn_partial")


class Patched:
    """module attributes and environment variables set for a `with` block (the --record main has no monkeypatch fixture)"""

    def __init__(self, env=None):
        self.env, self.saved = dict(env or {}), []

    def __enter__(self):
        import importlib
        for mod, attrs in THRESHOLDS.items():
            m = importlib.import_module("eprecon_amd." + mod)
            for name, value in attrs.items():
                self.saved.append((m, name, getattr(m, name)))
                setattr(m, name, value)
        self.old_env = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        return self

    def __exit__(self, *exc):
        for m, name, value in self.saved:
            setattr(m, name, value)
        for k, v in self.old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


class Recorder:
    """wraps the two convolution entry points (and the 16x16x4 packing call, counted) of the loaded library"""
    NAMES = ("eprecon_conv_desc_async", "eprecon_sparse_conv_fused_async", "eprecon_conv_pack_weight16_async",
             "eprecon_sparse_conv_async")

    def __init__(self):
        from eprecon_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.launches, self.packs16, self.steps = [], 0, []

    def __enter__(self):
        self.real = {n: getattr(self.lib, n) for n in self.NAMES}
        desc_fields = [(n, t) for n, t in self._lib.ConvDesc._fields_]

        def desc_async(dref, stream):
            d = self._lib.ConvDesc.from_buffer_copy(dref._obj)
            rc = self.real["eprecon_conv_desc_async"](dref, stream)
            rec = {"entry": "desc", "fields": {}, "pointers": [], "raw": {}}
            for name, ctype in desc_fields:
                v = getattr(d, name)
                if ctype is ctypes.c_void_p:
                    if v:
                        rec["pointers"].append(name)
                        rec["raw"][name] = v
                elif name != "workspace_bytes" and v != 0:
                    rec["fields"][name] = v
            need = int(self.lib.eprecon_conv_desc_workspace_bytes(ctypes.byref(d)))
            rec["workspace_need"], rec["workspace_covers"] = need, bool(d.workspace) and d.workspace_bytes >= need
            rec["workspace_bytes"] = int(d.workspace_bytes)
            rec["family"] = self._lib.last_conv_kernel() if rc == 0 and d.n_out > 0 else None
            self.launches.append(rec)
            return rc

        def plain_async(*a):
            # (the entry point without residual and summaries, which the library forwards to the fused one: recorded as that call)
            return fused_async(*a[:10], None, 0, *a[10:14], None, a[14], real="eprecon_sparse_conv_async", real_args=a)

        def fused_async(*args, real="eprecon_sparse_conv_fused_async", real_args=None):
            rc = self.real[real](*(args if real_args is None else real_args))
            rec = {"entry": "positional", "fields": {}, "pointers": [], "raw": {}}
            for name, v in zip(POSITIONAL, args):
                if name in ("x", "nbr", "weight", "bias", "residual", "out", "bn_partial"):
                    if v:
                        rec["pointers"].append(name)
                        rec["raw"][name] = v
                elif v != 0:
                    rec["fields"][name] = v
            rec["family"] = self._lib.last_conv_kernel() if rc == 0 and rec["fields"].get("n_out") else None
            self.launches.append(rec)
            return rc

        def pack16(*args):
            self.packs16 += 1
            return self.real["eprecon_conv_pack_weight16_async"](*args)

        for name, fn in zip(self.NAMES, (desc_async, fused_async, pack16, plain_async)):
            setattr(self.lib, name, fn)
        return self

    def __exit__(self, *exc):
        for name, fn in self.real.items():
            setattr(self.lib, name, fn)
        return False

    def step(self, what, fn, x, residual=None):
        """one wrapper call: fn() -> (out rows, summaries or None); the launches it made, with the offsets of their x / out /
        residual from the tensors of this call"""
        self.launches = []
        out, partial = fn()
        base = {"x": x, "out": out, "residual": residual}
        launches = []
        for rec in self.launches:
            raw = rec.pop("raw")
            rec["offsets"] = {k: raw[k] - t.data_ptr() for k, t in base.items() if k in raw and t is not None}
            launches.append(rec)
        entry = {"what": what, "launches": launches,
                 "summaries": None if partial is None else {"shape": list(partial.shape), "stride": list(partial.stride())}}
        self.steps.append(entry)
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# inputs

def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def mixed_map(rng, n, kvol=27):
    nbr = np.where(rng.random((kvol, n)) < 0.6, rng.integers(0, max(n, 1), (kvol, n)), -1).astype(np.int32)
    nbr[kvol // 2] = np.arange(n)
    return torch.from_numpy(nbr).cuda()


def down_map(rng, n):
    live = rng.random((8, n)) < 0.5
    live[rng.integers(0, 8, n), np.arange(n)] = True
    nbr = np.full((8, n), -1, np.int32)
    nbr[live] = rng.permutation(int(live.sum()))
    return torch.from_numpy(nbr).cuda(), int(live.sum())


def operands(rng, n_in, n_out, k, cin, cout, wdim=3):
    x = t32(rng.uniform(-1, 1, (n_in, cin)))
    w = t32(rng.normal(0, 1, (k, cin, cout) if wdim == 3 else (cin, cout)) / np.sqrt(k * cin))
    vec = lambda c, lo=0.5, hi=1.5: t32(rng.uniform(lo, hi, c))
    # (pending BatchNorms as the package makes them: rows of one fresh [2, C] tensor)
    aff_in, aff_out = t32(rng.uniform(0.5, 1.5, (2, cin))), t32(rng.uniform(0.5, 1.5, (2, cout)))
    return dict(x=x, w=w, bias=vec(cout, -0.5, 0.5), res=t32(rng.uniform(-1, 1, (n_out, cout))), gamma=vec(cout), beta=vec(cout, -0.3, 0.3),
                aff_in=aff_in, aff_out=aff_out, prior=t32(rng.uniform(-1, 1, (n_out, cout))))


def through_all_wrappers(rec, tag, o, nbr, ln=True, accumulate=True):
    """the four sparse wrappers on one set of operands"""
    from eprecon_amd import sparse as SP
    x, w, bias, res = o["x"], o["w"], o["bias"], o["res"]
    rec.step(f"{tag} sparse_conv", lambda: (SP.sparse_conv(x, w, nbr, bias, relu=True), None), x)
    rec.step(f"{tag} fused residual", lambda: SP.sparse_conv_fused(x, w, nbr, bias, None, True, res), x, res)
    rec.step(f"{tag} fused bn_partial", lambda: SP.sparse_conv_fused(x, w, nbr, None, bn_partial=True), x)
    if ln:
        rec.step(f"{tag} ln", lambda: (SP.sparse_conv_ln(x, w, nbr, bias, o["gamma"], o["beta"], 1e-5, relu=True, residual=res,
                                                         post_relu=True), None), x, res)
    rec.step(f"{tag} conv_stats in_affine", lambda: SP.conv_stats(x, w, nbr, in_affine=(o["aff_in"][0], o["aff_in"][1], True)), x)
    rec.step(f"{tag} conv_stats bias", lambda: SP.conv_stats(x, w, nbr, bias=bias), x)
    if accumulate:
        rec.step(f"{tag} sparse_conv accumulate", lambda: (SP.sparse_conv(x, w, nbr, bias, o["prior"].clone(), accumulate=True), None), x)
        rec.step(f"{tag} fused accumulate bn_partial",
                 lambda: SP.sparse_conv_fused(x, w, nbr, None, o["prior"].clone(), accumulate=True, bn_partial=True), x)


# ---------------------------------------------------------------------------------------------------------------------------
# cases: name -> (environment, function of (recorder, rng))

def case_k27(rec, rng):
    nbr = mixed_map(rng, 200)
    for cout in (32, 64, 65):
        through_all_wrappers(rec, f"cout{cout}", operands(rng, 200, 200, 27, 32, cout), nbr)


def case_k1(rec, rng):
    from eprecon_amd import sparse as SP
    for n in (999, 1000):
        for cout in (64, 65):
            for wdim in (2, 3):
                o = operands(rng, n, n, 1, 32, cout, wdim)
                x, w = o["x"], o["w"]
                tag = f"rows{n} cout{cout} w{wdim}d"
                rec.step(f"{tag} sparse_conv", lambda: (SP.sparse_conv(x, w, None, o["bias"]), None), x)
                rec.step(f"{tag} fused bn_partial", lambda: SP.sparse_conv_fused(x, w, None, bn_partial=True), x)
                rec.step(f"{tag} conv_stats", lambda: SP.conv_stats(x, w), x)
                rec.step(f"{tag} accumulate", lambda: (SP.sparse_conv(x, w, None, None, o["prior"].clone(), accumulate=True), None), x)


def case_k8_down(rec, rng):
    nbr, n_in = down_map(rng, 500)
    through_all_wrappers(rec, "down", operands(rng, n_in, 500, 8, 16, 8), nbr, accumulate=False)


def case_dense(rec, rng):
    from eprecon_amd import sparse as SP
    dims = (9, 13, 17)
    cells = np.argwhere(rng.random(dims) < 0.9)
    coords = np.concatenate([np.zeros((len(cells), 1), np.int64), cells], 1).astype(np.int32)
    vs = SP.VoxelSet(torch.from_numpy(coords).cuda(), 1, dims=dims)
    dm = SP.DenseMap(vs, dims)
    n = len(coords)
    for cin, cout in ((32, 1), (32, 16), (32, 32), (40, 32), (32, 48)):
        through_all_wrappers(rec, f"{cin}to{cout}", operands(rng, n, n, 27, cin, cout), dm)
    torch.cuda.synchronize()
    assert dm.off_grid() == 0


def d2_step(rec, tag, o, k, grid, x=None, residual=None, **kw):
    from eprecon_amd import dense2d as D2
    x = D2.Act(o["x"]) if x is None else x

    def run():
        act = D2.conv_bn_launch(o["w"], o["bias"], o["gamma"], o["beta"], 1e-5, k, x, grid, residual=residual, **kw)
        return act.rows, None
    rec.step(tag, run, x.rows, None if residual is None else residual.rows)


def case_dense2d(rec, rng):
    from eprecon_amd import dense2d as D2
    dev = torch.device("cuda", torch.cuda.current_device())
    for (maps, h, w), couts in (((1, 20, 24), (40, 81)), ((1, 20, 40), (40,)), ((1, 25, 40), (64, 65))):
        grid = D2.PixelGrid(maps, h, w, dev)
        for cout in couts:
            d2_step(rec, f"3x3 {h}x{w} cout{cout}", operands(rng, grid.n, grid.n, 9, 24, cout), 3, grid)
    for h, w in ((27, 37), (25, 40)):          # 999 and 1,000 pixels
        grid = D2.PixelGrid(1, h, w, dev)
        d2_step(rec, f"1x1 rows{grid.n}", operands(rng, grid.n, grid.n, 1, 48, 24), 1, grid)
    grid = D2.PixelGrid(1, 20, 24, dev)
    o = operands(rng, grid.n, grid.n, 9, 24, 24)
    d2_step(rec, "3x3 pending affines", o, 3, grid, x=D2.Act(o["x"], o["aff_in"][0], o["aff_in"][1], True),
            residual=D2.Act(o["res"], o["aff_out"][0], o["aff_out"][1], True), pre_relu=True)
    with D2.bn_pass(D2.BnArena(dev, words=1 << 14)):
        d2_step(rec, "3x3 in a bn_pass", o, 3, grid)
        d2_step(rec, "1x1 in a bn_pass", operands(rng, grid.n, grid.n, 1, 24, 24), 1, grid)


def case_wide(rec, rng):
    from eprecon_amd import sparse as SP
    o = operands(rng, 4096, 4096, 27, 96, 65)
    nbr = mixed_map(rng, 4096)
    x, w = o["x"], o["w"]
    rec.step("fused relu bn_partial", lambda: SP.sparse_conv_fused(x, w, nbr, o["bias"], None, True, bn_partial=True), x)
    rec.step("conv_stats", lambda: SP.conv_stats(x, w, nbr), x)
    rec.step("ln (no workspace: the wide kernels decline LayerNorm)",
             lambda: (SP.sparse_conv_ln(x, w, nbr, None, o["gamma"], o["beta"], 1e-5), None), x)


def case_empty(rec, rng):
    from eprecon_amd import sparse as SP
    w = operands(rng, 1, 1, 27, 32, 24)["w"]
    x, nbr = torch.empty((0, 32), device="cuda"), torch.empty((27, 0), dtype=torch.int32, device="cuda")
    rec.step("conv_stats, no rows", lambda: SP.conv_stats(x, w, nbr), x)


CASES = {
    "k27_map200": ({}, case_k27),
    "k1_identity": ({}, case_k1),
    "k8_down500": ({}, case_k8_down),
    "dense_level2": ({"EPRECON_CONV_DENSE3D": "2"}, case_dense),
    "dense_level1": ({"EPRECON_CONV_DENSE3D": "1"}, case_dense),
    "dense_level0": ({"EPRECON_CONV_DENSE3D": "0"}, case_dense),
    "dense2d": ({}, case_dense2d),
    "wide": ({}, case_wide),
    "stats_no_rows": ({}, case_empty),
}


def run_case(name):
    """-> (steps as recorded, the output rows of every step)"""
    import zlib
    env, fn = CASES[name]
    outs = []
    with Patched(env), Recorder() as rec:
        real_step = rec.step

        def step(*a, **kw):
            outs.append(real_step(*a, **kw))
        rec.step = step
        fn(rec, np.random.default_rng(zlib.crc32(name.encode())))
        torch.cuda.synchronize()
    return rec.steps, outs


def comparable(steps):
    """what the golden file holds of a run (the attached workspace_bytes depends on the process's history before the change)"""
    steps = json.loads(json.dumps(steps))
    for s in steps:
        for rec in s["launches"]:
            rec.pop("workspace_bytes", None)
    return steps


# ---------------------------------------------------------------------------------------------------------------------------
# tests

@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_wrappers_hand_over_what_they_did(golden, name):
    steps, outs = run_case(name)
    want = golden["cases"][name]
    got = comparable(steps)
    assert [s["what"] for s in got] == [s["what"] for s in want]
    for g, w in zip(got, want):
        assert g == w, f"{name}: {g['what']}"
    # the same bits on a second run
    steps2, outs2 = run_case(name)
    assert comparable(steps2) == got
    for s, a, b in zip(steps, outs, outs2):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), f"{name}: {s['what']}: run-to-run"


@pytest.mark.gpu
def test_conv_stats_without_rows_launches_nothing():
    steps, outs = run_case("stats_no_rows")
    assert steps[0]["launches"] == [] and steps[0]["summaries"]["shape"] == [1, 3, 24] and tuple(outs[0].shape) == (0, 24)


@pytest.mark.gpu
def test_wide_workspace_is_the_library_s_byte_count():
    steps, _ = run_case("wide")
    for s in steps[:2]:
        (rec,) = s["launches"]
        assert rec["family"] == "spconv_wide_kernel" and "workspace" in rec["pointers"], s["what"]
        assert rec["workspace_need"] > 0 and rec["workspace_bytes"] == rec["workspace_need"], s["what"]
    (rec,) = steps[2]["launches"]
    assert "workspace" not in rec["pointers"] and rec["workspace_bytes"] == 0


@pytest.mark.gpu
def test_packing_of_a_2d_weight_is_cached_on_its_owner():
    """a [Cin, Cout] weight becomes a transient [1, Cin, Cout] view in the wrapper: its packing must be found again through
    the object the caller holds"""
    from eprecon_amd import sparse as SP
    from eprecon_amd import weight_cache
    rng = np.random.default_rng(5)
    o = operands(rng, 1000, 1000, 1, 32, 64, wdim=2)
    with Patched(), Recorder() as rec:
        rec.step("first", lambda: (SP.sparse_conv(o["x"], o["w"]), None), o["x"])
        first = rec.packs16
        rec.step("second", lambda: (SP.sparse_conv(o["x"], o["w"]), None), o["x"])
        rec.step("third, with summaries", lambda: SP.conv_stats(o["x"], o["w"]), o["x"])
        torch.cuda.synchronize()
    assert first == 1 and rec.packs16 == 1
    assert all("packed_weight16" in s["launches"][0]["pointers"] for s in rec.steps)
    assert weight_cache.peek(o["w"], "sparse.packed_weight16") is not None


def record(commit, path):
    cases = {name: comparable(run_case(name)[0]) for name in CASES}
    doc = {"recorded_on": commit,
           "about": "tests/test_conv_descriptors_gpu.py --record: per wrapper call the launches it handed to the library. "
                    "Integer / float fields that are 0 and pointer fields that are null are left out.",
           "thresholds": THRESHOLDS, "cases": cases}
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{path}: {sum(len(s['launches']) for c in cases.values() for s in c)} launches in "
          f"{sum(len(c) for c in cases.values())} wrapper calls of {len(cases)} cases")


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    assert len(sys.argv) >= 3 and sys.argv[1] == "--record", __doc__
    record(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else GOLDEN)
