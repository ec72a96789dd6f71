"""GPU parity of the sparse primitives (hash grid, unique, kernel maps, MFMA gather-GEMM conv,
BatchNorm / LayerNorm epilogues) against the numpy oracle.  Index results bit-exact; fp32
features within 1e-3 (observed ~1e-5)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import sparse as OS  # noqa: E402
from test_oracle_sparse import random_coords  # noqa: E402

TOL = 1e-3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("n,stride", [(1, 1), (777, 1), (50000, 2), (200000, 1)])
def test_hash_build_query(n, stride):
    from eprecon_amd.sparse import HashGrid
    rng = np.random.default_rng(n)
    c = random_coords(rng, n, extent=60, batch=3, stride=stride)
    g = HashGrid(len(c), torch.device("cuda")).build(dev(c))
    assert g.status_ok()
    assert np.array_equal(g.query(dev(c)).cpu().numpy(), np.arange(len(c), dtype=np.int32))
    q = random_coords(rng, 5000, extent=70, batch=3, stride=stride)
    assert np.array_equal(g.query(dev(q)).cpu().numpy(), OS.Index(c).lookup(q))


def _scan_scratch_ints(lib, n):
    """what the library asks for a scan over n elements: the only contract there is for the scratch"""
    return int(lib.eprecon_exclusive_scan_scratch_ints(n))


def _scan(lib, dx, n, out, tot, scratch, stream=None):
    from eprecon_amd import _lib
    _lib.check(lib.eprecon_exclusive_scan_async(_lib.ptr(dx), n, _lib.ptr(out), _lib.ptr(tot), _lib.ptr(scratch),
                                                _lib.current_stream() if stream is None else stream.cuda_stream),
               "eprecon_exclusive_scan_async")


def _scan_case(n, seed=None):
    x = np.random.default_rng(n if seed is None else seed).integers(0, 9, n).astype(np.int32)
    return x, np.concatenate([[0], np.cumsum(x[:-1], dtype=np.int64)]).astype(np.int32)


SCAN_GUARD = 0x5ca7c4ed


@pytest.mark.parametrize("n", [1, 63, 2049, 8192, 8193, 16385, 32768, 32769, 100003, 320868, 2500001])
def test_device_scan_all_forms(n):
    """the exclusive scan behind every compaction: one workgroup / one pass up to 32,768 elements, tile sums + apply beyond —
    against numpy, the grand total included, twice, and 70 launches in a row into the same scratch (a call keeps no state)"""
    from eprecon_amd import _lib
    lib = _lib.load()
    x, want = _scan_case(n)
    dx = dev(x)
    scratch = torch.empty(_scan_scratch_ints(lib, n), dtype=torch.int32, device="cuda")

    def run():
        out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        tot = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        _scan(lib, dx, n, out, tot, scratch)
        return out.cpu().numpy(), int(tot.item())
    for _ in range(2):
        got, tot = run()
        assert np.array_equal(got, want) and tot == int(x.sum())
    if n in (100003, 320868):
        for _ in range(70):
            got, tot = run()
        assert np.array_equal(got, want) and tot == int(x.sum())


@pytest.mark.parametrize("n", [32769, 100003, 4096 * 2048 + 1])
def test_device_scan_stays_inside_its_scratch(n):
    """the scratch is exactly what eprecon_exclusive_scan_scratch_ints answers, with 64 guard words behind it, at the smallest
    length that reaches each long form: tile sums + scan_apply<true> (17 tiles; 49 tiles), and above 4,096 tiles tile sums +
    scan_sums_inplace + scan_apply<false> (4,097 tiles).  The whole buffer starts as the guard pattern, and a second launch
    into the same buffer meets what the first one left: a scan depends on nothing it finds in its scratch."""
    from eprecon_amd import _lib
    lib = _lib.load()
    x, want = _scan_case(n)
    tiles = _scan_scratch_ints(lib, n)
    assert tiles >= (n + 2047) // 2048
    buf = torch.full((tiles + 64,), SCAN_GUARD, dtype=torch.int32, device="cuda")
    dx = dev(x)
    for _ in range(2):
        out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        tot = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        _scan(lib, dx, n, out, tot, buf)
        assert bool((buf[tiles:] == SCAN_GUARD).all())
        assert np.array_equal(out.cpu().numpy(), want) and int(tot.item()) == int(x.sum()) < 2 ** 27


def test_device_scans_on_two_streams_keep_their_state_apart():
    """two streams, each with its own input (17 and 49 tiles), scratch and outputs: 70 scans per stream, queued
    alternately from the host, every one into a scratch refilled with the guard pattern on its own stream.  Every output and
    total is compared on the device; one host read per stream at the end."""
    from eprecon_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lanes = []
    for n in (32769, 100003):
        x, want = _scan_case(n)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            lanes.append(dict(n=n, st=st, dx=dev(x), want=dev(want), total=int(x.sum()),
                              scratch=torch.empty(_scan_scratch_ints(lib, n), dtype=torch.int32, device="cuda"),
                              out=torch.empty(n, dtype=torch.int32, device="cuda"),
                              tot=torch.empty(1, dtype=torch.int32, device="cuda"),
                              ok=torch.ones((), dtype=torch.bool, device="cuda")))
    for _ in range(70):
        for a in lanes:
            with torch.cuda.stream(a["st"]):
                a["scratch"].fill_(SCAN_GUARD)
                a["out"].fill_(-7)
                a["tot"].fill_(-7)
                _scan(lib, a["dx"], a["n"], a["out"], a["tot"], a["scratch"], a["st"])
                a["ok"] &= (a["out"] == a["want"]).all() & (a["tot"][0] == a["total"])
    for a in lanes:
        with torch.cuda.stream(a["st"]):
            assert bool(a["ok"].item()), a["n"]
    torch.cuda.synchronize()


def test_device_scan_replays_under_a_graph():
    """two scans (17 and 49 tiles, a scratch each) captured back to back in one graph on one stream, replayed three times with
    the inputs overwritten in between: a replay depends on nothing the one before it left in the scratch"""
    from eprecon_amd import _lib
    lib = _lib.load()
    ns = (32769, 100003)
    cases = [[_scan_case(n, seed) for n in ns] for seed in (11, 12)]
    dx = [dev(x) for x, _ in cases[0]]
    scratch = [torch.empty(_scan_scratch_ints(lib, n), dtype=torch.int32, device="cuda") for n in ns]
    out = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in ns]
    tot = [torch.full((1,), -7, dtype=torch.int32, device="cuda") for n in ns]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i, n in enumerate(ns):
            _scan(lib, dx[i], n, out[i], tot[i], scratch[i])
    for replay in range(3):
        case = cases[replay % 2]
        for i in range(2):
            dx[i].copy_(dev(case[i][0]))
            out[i].fill_(-7)
            tot[i].fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for i in range(2):
            x, want = case[i]
            assert np.array_equal(out[i].cpu().numpy(), want) and int(tot[i].item()) == int(x.sum())


def test_hash_rejects_out_of_range_keys():
    from eprecon_amd import _lib
    from eprecon_amd.sparse import HashGrid
    c = np.array([[0, 1, 2, 3], [0, 600000, 0, 0]], np.int32)
    g = HashGrid(2, torch.device("cuda")).build(dev(c))
    with pytest.raises(_lib.EpreconError):
        g.status_ok()


def test_unique_raises_on_out_of_range_voxels():
    """production path: the status word travels with the voxel count (no extra synchronisation) and raises"""
    from eprecon_amd import _lib
    from eprecon_amd.sparse import unique_coords
    c = np.array([[0, 1, 2, 3], [0, 1, 2, 3], [15, 0, 0, 0]], np.int32)      # batch index 15 cannot be packed
    with pytest.raises(_lib.EpreconError):
        unique_coords(dev(c), 1)


@pytest.mark.parametrize("q", [1, 2, 4])
def test_unique_first_occurrence(q):
    from eprecon_amd.sparse import unique_coords
    rng = np.random.default_rng(5 + q)
    c = random_coords(rng, 30000, extent=25, batch=2)
    c = np.concatenate([c, c[rng.integers(0, len(c), 9000)]])
    rng.shuffle(c)
    u, inv, grid = unique_coords(dev(c), q)
    ru, rinv = OS.unique_first(c, q)
    assert np.array_equal(u.cpu().numpy(), ru) and np.array_equal(inv.cpu().numpy(), rinv)
    # the table now returns voxel ids
    assert np.array_equal(grid.query(dev(c), q).cpu().numpy(), rinv)


def test_kernel_maps():
    from eprecon_amd.sparse import VoxelSet
    rng = np.random.default_rng(9)
    c = random_coords(rng, 40000, extent=22, batch=2, stride=2)
    vs = VoxelSet(dev(c), stride=2)
    assert np.array_equal(vs.kernel_map(3).cpu().numpy(), OS.kernel_map(c, c, 3, 2))
    coarse, down, up = vs.downsample()
    rc, rparent = OS.unique_first(c, 4)
    assert coarse.stride == 4 and np.array_equal(coarse.coords.cpu().numpy(), rc)
    assert np.array_equal(down.cpu().numpy(), OS.kernel_map(c, rc, 2, 2))
    assert np.array_equal(up.cpu().numpy(), OS.transpose_map(c, rparent, 2))
    # a second level on the coarse set
    c2, d2, u2 = coarse.downsample()
    rc2, rp2 = OS.unique_first(rc, 8)
    assert np.array_equal(c2.coords.cpu().numpy(), rc2)
    assert np.array_equal(d2.cpu().numpy(), OS.kernel_map(rc, rc2, 2, 4))


@pytest.mark.parametrize("n,extent,stride", [(1, 4, 1), (300, 6, 1), (40000, 22, 2), (150000, 60, 1)])
def test_self_kernel_map_with_half_the_probes_is_the_same_table(n, extent, stride):
    """eprecon_kernel_map_self_async (the 13 offsets below the centre looked up, their mirror images filled in: the geometry calls
    of an SPVCNN pass / a GRU level use it on the sets the unique numbering produced) == eprecon_kernel_map_async == the oracle"""
    from eprecon_amd import _lib
    from eprecon_amd.sparse import VoxelSet
    rng = np.random.default_rng(n)
    c = random_coords(rng, n, extent=extent, batch=2, stride=stride)
    vs = VoxelSet(dev(c), stride=stride)
    full = vs.kernel_map(3)
    half = torch.full_like(full, 12345)
    grid = vs.grid
    _lib.check(_lib.load().eprecon_kernel_map_self_async(_lib.ptr(grid.mem), grid.capacity, _lib.ptr(vs.coords), vs.n, stride,
                                                         _lib.ptr(half), _lib.current_stream()), "eprecon_kernel_map_self_async")
    assert torch.equal(full, half)
    if n <= 40000:
        assert np.array_equal(half.cpu().numpy(), OS.kernel_map(c, c, 3, stride))


@pytest.mark.parametrize("cin,cout", [(32, 32), (74, 8), (138, 16), (80, 32), (128, 128), (192, 96),
                                      (16, 1), (12, 24), (64, 96)])
def test_sparse_conv_k3(cin, cout):
    from eprecon_amd.sparse import VoxelSet, sparse_conv
    rng = np.random.default_rng(cin * 1000 + cout)
    c = random_coords(rng, 3001, extent=9, batch=1)
    x = rng.standard_normal((len(c), cin)).astype(np.float32)
    w = (rng.standard_normal((27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    vs = VoxelSet(dev(c))
    nbr = OS.kernel_map(c, c, 3, 1)
    got = sparse_conv(dev(x), dev(w), vs.kernel_map(3), dev(b)).cpu().numpy()
    ref = OS.sparse_conv(x, nbr, w, b)
    assert np.abs(got - ref).max() < TOL
    # A = I check with an asymmetric weight: catches row/column transposition in the MFMA layout
    if cin == cout:
        eye = np.zeros((27, cin, cout), np.float32)
        eye[13] = np.eye(cin) + np.triu(np.ones((cin, cin), np.float32), 1) * 0.5
        got = sparse_conv(dev(x), dev(eye), vs.kernel_map(3)).cpu().numpy()
        assert np.abs(got - x @ eye[13]).max() < 1e-4


def test_sparse_conv_strided_transposed_k1_and_slices():
    from eprecon_amd.sparse import VoxelSet, sparse_conv
    rng = np.random.default_rng(77)
    c = random_coords(rng, 20011, extent=14, batch=2)
    vs = VoxelSet(dev(c))
    coarse, down, up = vs.downsample()
    rc, rparent = OS.unique_first(c, 2)
    x = rng.standard_normal((len(c), 32)).astype(np.float32)
    wd = rng.standard_normal((8, 32, 64)).astype(np.float32) * 0.1
    y = sparse_conv(dev(x), dev(wd), down)
    yref = OS.sparse_conv(x, OS.kernel_map(c, rc, 2, 1), wd)
    assert np.abs(y.cpu().numpy() - yref).max() < TOL
    wu = rng.standard_normal((8, 64, 48)).astype(np.float32) * 0.1
    # transposed conv writes straight into the left slice of a concat buffer (torchsparse.cat)
    cat = torch.zeros((len(c), 48 + 32), device="cuda")
    cat[:, 48:] = dev(x)
    sparse_conv(y, dev(wu), up, out=cat[:, :48])
    zref = OS.sparse_conv(yref, OS.transpose_map(c, rparent, 1), wu)
    assert np.abs(cat[:, :48].cpu().numpy() - zref).max() < TOL
    assert torch.equal(cat[:, 48:], dev(x))
    # k = 1 linear layer reading the right slice, fused ReLU, then accumulate
    w1 = rng.standard_normal((32, 40)).astype(np.float32)
    o = sparse_conv(cat[:, 48:], dev(w1), relu=True)
    assert np.abs(o.cpu().numpy() - np.maximum(x @ w1, 0)).max() < TOL
    o2 = sparse_conv(cat[:, 48:], dev(w1), out=o.clone(), accumulate=True)
    assert np.abs(o2.cpu().numpy() - (np.maximum(x @ w1, 0) + x @ w1)).max() < TOL


@pytest.mark.parametrize("n,c", [(1, 8), (1000, 1), (5000, 24), (70001, 96), (3000, 128)])
def test_batchnorm_and_layernorm(n, c):
    from eprecon_amd.sparse import batchnorm_train, rowwise_layernorm
    rng = np.random.default_rng(n + c)
    x = (rng.standard_normal((n, c)) * 2 + 0.5).astype(np.float32)
    r = rng.standard_normal((n, c)).astype(np.float32)
    g = rng.standard_normal(c).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    if n > 1:
        got = batchnorm_train(dev(x), dev(g), dev(b), 1e-5, dev(r), True).cpu().numpy()
        assert np.abs(got - OS.batchnorm_train(x, g, b, 1e-5, r, True)).max() < TOL
        xin = dev(x)
        assert batchnorm_train(xin, dev(g), dev(b), out=xin) is xin  # in place
        assert np.abs(xin.cpu().numpy() - OS.batchnorm_train(x, g, b)).max() < TOL
    if c > 1:
        got = rowwise_layernorm(dev(x), dev(g), dev(b), 1e-5, dev(r), True, False).cpu().numpy()
        assert np.abs(got - OS.layernorm_rows(x, g, b, 1e-5, r, True, False)).max() < TOL
        got = rowwise_layernorm(dev(x), dev(g), dev(b), post_relu=True).cpu().numpy()
        assert np.abs(got - OS.layernorm_rows(x, g, b, post_relu=True)).max() < TOL


@pytest.mark.parametrize("cin,cout,k", [(32, 32, 3), (32, 16, 3), (16, 16, 3), (128, 32, 1), (32, 32, 1), (24, 40, 3),
                                        (8, 100, 1)])
def test_sparse_conv_with_fused_layernorm(cin, cout, k):
    """conv [+ReLU] [+residual] -> LayerNorm [-> ReLU] in one launch == the oracle's conv followed by its
    row-wise LayerNorm (the SubM + LayerNorm blocks of models/modules.py:440-482)"""
    from eprecon_amd.sparse import VoxelSet, sparse_conv_ln
    rng = np.random.default_rng(cin * 100 + cout + k)
    c = random_coords(rng, 2777, extent=9, batch=1)
    x = rng.standard_normal((len(c), cin)).astype(np.float32)
    kv = k ** 3
    w = (rng.standard_normal((kv, cin, cout)) / np.sqrt(kv * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    g = rng.standard_normal(cout).astype(np.float32)
    be = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((len(c), cout)).astype(np.float32)
    vs = VoxelSet(dev(c))
    nbr_d = vs.kernel_map(3) if k == 3 else None
    nbr = OS.kernel_map(c, c, 3, 1) if k == 3 else np.arange(len(c), dtype=np.int32)[None]
    y = OS.sparse_conv(x, nbr, w, b)
    # SubMconv3dBlock: ReLU(LN(conv))
    got = sparse_conv_ln(dev(x), dev(w), nbr_d, dev(b), dev(g), dev(be), 1e-5, post_relu=True).cpu().numpy()
    assert np.abs(got - OS.layernorm_rows(y, g, be, 1e-5, post_relu=True)).max() < TOL
    # residual blocks: LN(res + ReLU(conv)), written into a channel slice of a wider buffer
    wide = torch.zeros((len(c), cout + 8), device="cuda")
    out = sparse_conv_ln(dev(x), dev(w), nbr_d, dev(b), dev(g), dev(be), 1e-5, out=wide[:, 4:4 + cout], relu=True,
                         residual=dev(res))
    ref = OS.layernorm_rows(y, g, be, 1e-5, res, True, False)
    assert np.abs(out.cpu().numpy() - ref).max() < TOL
    assert not wide[:, :4].any() and not wide[:, 4 + cout:].any()


@pytest.mark.parametrize("cin,cout", [(81, 32), (139, 96), (75, 48), (51, 24), (5, 8)])
def test_sparse_conv_ragged_channels_with_padded_pitch(cin, cout):
    """SPVCNN stem channel counts: rows with a pitch rounded up to 4 floats take the 16-byte gather path;
    whatever sits in the pad lanes (here NaN) must not reach the result"""
    from eprecon_amd.sparse import VoxelSet, sparse_conv
    rng = np.random.default_rng(cin + cout)
    c = random_coords(rng, 2500, extent=8, batch=1)
    x = rng.standard_normal((len(c), cin)).astype(np.float32)
    w = (rng.standard_normal((27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    vs = VoxelSet(dev(c))
    cp = (cin + 3) & ~3
    buf = torch.full((len(c), cp), float("nan"), device="cuda")
    buf[:, :cin] = dev(x)
    got = sparse_conv(buf[:, :cin], dev(w), vs.kernel_map(3), dev(b)).cpu().numpy()
    ref = OS.sparse_conv(x, OS.kernel_map(c, c, 3, 1), w, b)
    assert np.isfinite(got).all() and np.abs(got - ref).max() < TOL


def _last_conv_kernel(arm, fn):
    """run fn() with the one-shot conv profiler armed: -> (result, name of the kernel family that took the launch)"""
    import ctypes
    from eprecon_amd import _lib
    lib = _lib.load()
    lib.eprecon_profile_conv_arm(*arm)
    out = fn()
    rows, name = ctypes.c_int64(0), ctypes.c_char_p()
    assert lib.eprecon_profile_conv_ms(ctypes.byref(rows), ctypes.byref(name)) >= 0
    return out, name.value.decode()


@pytest.mark.parametrize("cin,cout", [(48, 24), (32, 32), (24, 24), (16, 16), (74, 8), (96, 48), (64, 64), (140, 16)])
def test_direct_gather_kernel_on_a_long_list(cin, cout):
    """the long-list form of the 3x3x3 convolution (spconv_direct16_kernel: operands straight from L2 into the 16x16x4 MFMAs,
    no LDS staging) with every epilogue the layers use: bias + ReLU + residual, the producer's pending BatchNorm on the
    gathered values + summaries of the output, row-wise LayerNorm"""
    from eprecon_amd import sparse as SP
    rng = np.random.default_rng(cin * 131 + cout)
    c = random_coords(rng, 41003, extent=34, batch=1)
    n = len(c)
    x = rng.standard_normal((n, cin)).astype(np.float32)
    w = (rng.standard_normal((27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((n, cout)).astype(np.float32)
    vs = SP.VoxelSet(dev(c))
    nbr_d = vs.kernel_map(3)
    nbr = OS.kernel_map(c, c, 3, 1)
    cp = (cin + 3) & ~3
    buf = torch.full((n, cp), float("nan"), device="cuda")       # ragged channel counts sit on a padded pitch
    buf[:, :cin] = dev(x)
    dx, dw, db = buf[:, :cin], dev(w), dev(b)
    ref = OS.sparse_conv(x, nbr, w, b)
    (y, part), name = _last_conv_kernel((27, cin, cout, 1000), lambda: SP.sparse_conv_fused(
        dx, dw, nbr_d, db, relu=True, residual=dev(res), bn_partial=True))
    assert name == "spconv_direct16_kernel"
    want = np.maximum(ref, 0) + res
    assert np.abs(y.cpu().numpy() - want).max() < TOL
    part = part.cpu().numpy().astype(np.float64)                     # [blocks, 3, cout]: (count, mean, M2) of the stored rows
    assert part.shape[0] == (n + 127) // 128 and part[:, 0, 0].sum() == n
    cnt, mean, m2 = part[:, 0], part[:, 1], part[:, 2]
    tot_mean = (cnt * mean).sum(0) / n
    tot_m2 = (m2 + cnt * (mean - tot_mean) ** 2).sum(0)
    assert np.abs(tot_mean - want.mean(0)).max() < 1e-4 and np.abs(tot_m2 / n - want.var(0)).max() < 1e-3
    # pending BatchNorm (+ ReLU) of the producer applied while gathering; missing neighbours stay zero
    sc = rng.uniform(0.5, 1.5, cin).astype(np.float32)
    sh = rng.standard_normal(cin).astype(np.float32)
    y2, _ = SP.conv_stats(dx, dw, nbr_d, in_affine=(dev(sc), dev(sh), True))
    ref2 = OS.sparse_conv(np.maximum(x * sc + sh, 0), nbr, w)
    assert np.abs(y2.cpu().numpy() - ref2).max() < TOL
    # LN(res + ReLU(conv)) into a channel slice of a wider buffer
    g, be = rng.standard_normal(cout).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
    wide = torch.zeros((n, cout + 8), device="cuda")
    out = SP.sparse_conv_ln(dx, dw, nbr_d, db, dev(g), dev(be), 1e-5, out=wide[:, 4:4 + cout], relu=True, residual=dev(res))
    assert np.abs(out.cpu().numpy() - OS.layernorm_rows(ref, g, be, 1e-5, res, True, False)).max() < TOL
    assert not wide[:, :4].any() and not wide[:, 4 + cout:].any()


@pytest.mark.parametrize("form", ["padded", "persist"])
@pytest.mark.parametrize("cin,cout", [(48, 24), (74, 8), (32, 24), (24, 24), (80, 40), (16, 16), (32, 32)])
def test_direct_kernel_forms_agree(monkeypatch, form, cin, cout):
    """Round 6: the last 8 columns of C_out = 16 m + 8 on v_mfma_f32_4x4x1_16B_f32 (default; the (48, 24) / (74, 8) / (24, 24)
    cases of the test above run it) against the padded 16-column tile (EPRECON_CONV_TAIL8=0), and the persistent form with the
    packing resident in LDS and 32-row jobs pulled from device counters (EPRECON_CONV_PERSIST=1: per-job BatchNorm summaries).
    Every form against the oracle; the summaries of every form must describe the same output."""
    from eprecon_amd import sparse as SP
    rng = np.random.default_rng(cin * 17 + cout)
    c = random_coords(rng, 41003, extent=34, batch=1)
    n = len(c)
    x = rng.standard_normal((n, cin)).astype(np.float32)
    w = (rng.standard_normal((27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    vs = SP.VoxelSet(dev(c))
    nbr_d = vs.kernel_map(3)
    nbr = OS.kernel_map(c, c, 3, 1)
    cp = (cin + 3) & ~3
    buf = torch.full((n, cp), float("nan"), device="cuda")
    buf[:, :cin] = dev(x)
    dx, dw, db = buf[:, :cin], dev(w), dev(b)
    sc = rng.uniform(0.5, 1.5, cin).astype(np.float32)
    sh = rng.standard_normal(cin).astype(np.float32)
    want = OS.sparse_conv(np.maximum(x * sc + sh, 0), nbr, w, b)

    def run():
        (y, part), name = _last_conv_kernel((27, cin, cout, 1000), lambda: SP.conv_stats(dx, dw, nbr_d, in_affine=(dev(sc), dev(sh), True), bias=db))
        assert name == "spconv_direct16_kernel"
        return y.cpu().numpy(), part.cpu().numpy().astype(np.float64)

    y0, p0 = run()
    monkeypatch.setenv("EPRECON_CONV_TAIL8" if form == "padded" else "EPRECON_CONV_PERSIST", "0" if form == "padded" else "1")
    y1, p1 = run()
    persist_takes_it = form == "persist" and ((cin + 15) // 16) * (1024 * (cout // 16) + 512 * (cout % 16 == 8)) <= 4864
    assert p1.shape[0] == ((n + 31) // 32 if persist_takes_it else (n + 127) // 128)
    for y, part in ((y0, p0), (y1, p1)):
        assert np.abs(y - want).max() < TOL
        cnt, mean, m2 = part[:, 0], part[:, 1], part[:, 2]
        assert cnt[:, 0].sum() == n
        tot_mean = (cnt * mean).sum(0) / n
        tot_m2 = (m2 + cnt * (mean - tot_mean) ** 2).sum(0)
        assert np.abs(tot_mean - want.mean(0)).max() < 1e-4 and np.abs(tot_m2 / n - want.var(0)).max() < 1e-3
    assert np.abs(y0 - y1).max() < 1e-4
    # the persistent form zeroes its own job counters, the head of the stream's grow-only workspace: dirty counters would make
    # it skip every row or run past the list — a launch into a workspace full of 0xFF, and one more into what that launch left
    if persist_takes_it:
        from eprecon_amd import _lib
        _lib.workspace(512, torch.device("cuda", torch.cuda.current_device())).fill_(0xFF)
        y2, _ = run()
        assert np.array_equal(y1, y2)
        y2, _ = run()
        assert np.array_equal(y1, y2)


def test_persistent_form_asks_for_its_counters(monkeypatch):
    """EPRECON_CONV_PERSIST=1, 48 -> 24 on the shortest list the form takes (8,192 rows): the workspace query answers its job
    counters and the summaries are per 32-row job; the same descriptor WITHOUT the workspace is refused (EPRECON_ERR_WORKSPACE)
    before anything is launched — it must not end up on the 128-row kernel, whose summaries the caller did not size.  One row
    fewer and the launch is the per-tile kernel's: no workspace, 128-row blocks.  (EPRECON_CONV_SPLITK=0: up to 256 workgroups
    of 128 rows the split-K kernel goes first, so the shortest list the form takes reaches the direct family only without it.)"""
    import ctypes
    from eprecon_amd import _lib
    from eprecon_amd import sparse as SP
    lib = _lib.load()
    monkeypatch.setenv("EPRECON_CONV_PERSIST", "1")
    monkeypatch.setenv("EPRECON_CONV_SPLITK", "0")
    g = torch.Generator().manual_seed(3)
    for n in (8192, 8191):
        nbr = torch.randint(-1, n, (27, n), generator=g, dtype=torch.int32).cuda()
        x, w = torch.randn((n, 48), generator=g).cuda(), (torch.randn((27, 48, 24), generator=g) / 36).cuda()
        out = torch.full((n, 24), -7.0, device="cuda")
        _, part, d, keep = SP.conv_call(x, w, nbr, out=out, stats=True, launch=False)
        need = int(lib.eprecon_conv_desc_workspace_bytes(ctypes.byref(d)))
        if n < 8192:
            assert need == 0 and part.shape[0] == (n + 127) // 128
            continue
        assert need >= 512 and d.workspace and d.workspace_bytes >= need and part.shape[0] == n // 32
        d.workspace, d.workspace_bytes = None, 0
        assert int(lib.eprecon_conv_desc_workspace_bytes(ctypes.byref(d))) == need         # the query does not depend on it
        assert int(lib.eprecon_conv_desc_partial_rows(ctypes.byref(d))) == n // 32
        with pytest.raises(_lib.EpreconError, match="error -2"):
            _lib.check(lib.eprecon_conv_desc_async(ctypes.byref(d), _lib.current_stream()), "eprecon_conv_desc_async")
        assert bool((out == -7.0).all())


BF16X3_BUDGET = 2.0 ** -14      # of the term-magnitude sum  sum_k |a_k| |w_k|  of an output (3 * 2^-16 by construction)


@pytest.mark.parametrize("cin,cout", [(48, 24), (74, 8), (32, 24), (24, 24), (80, 40), (16, 16), (96, 48), (40, 64)])
def test_bf16x3_opt_in_is_within_its_error_budget(monkeypatch, cin, cout):
    """Round 6 (SURVEY section 7 "with an error budget"): EPRECON_CONV_BF16X3=1 runs the direct gather kernel's
    products on the bf16 matrix pipe as a_hi w_hi + a_hi w_lo + a_lo w_hi (both operands split in registers from the fp32
    loads, fp32 accumulate).  Never the default: the library's figures and parity claims are the exact-fp32 path's.  Budget:
    every output within 2^-14 of the sum of its terms' magnitudes (measured: ~2^-17), i.e. 1e-3 parity holds with room; the
    BatchNorm summaries describe the stored values; the default path is untouched by the switch being compiled in."""
    from eprecon_amd import sparse as SP
    rng = np.random.default_rng(cin * 19 + cout)
    c = random_coords(rng, 41003, extent=34, batch=1)
    n = len(c)
    x = rng.standard_normal((n, cin)).astype(np.float32)
    w = (rng.standard_normal((27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    vs = SP.VoxelSet(dev(c))
    nbr_d = vs.kernel_map(3)
    nbr = OS.kernel_map(c, c, 3, 1)
    cp = (cin + 3) & ~3
    buf = torch.full((n, cp), float("nan"), device="cuda")
    buf[:, :cin] = dev(x)
    dx, dw, db = buf[:, :cin], dev(w), dev(b)
    sc = rng.uniform(0.5, 1.5, cin).astype(np.float32)
    sh = rng.standard_normal(cin).astype(np.float32)
    a = np.maximum(x * sc + sh, 0)      # (fp32, one rounding per op: what the kernel's fmaf + max compute up to 1 ulp)

    def conv64(a64, w64):                # the oracle's sum (oracle/sparse.py: sparse_conv) carried in float64
        out = np.zeros((n, cout))
        for k in range(27):
            m = nbr[k] >= 0
            out[m] += a64[nbr[k][m]] @ w64[k]
        return out
    want = conv64(a.astype(np.float64), w.astype(np.float64)) + b
    scale = conv64(np.abs(a).astype(np.float64), np.abs(w).astype(np.float64)) + np.abs(b)

    def run():
        (y, part), name = _last_conv_kernel((27, cin, cout, 1000), lambda: SP.conv_stats(dx, dw, nbr_d, in_affine=(dev(sc), dev(sh), True), bias=db))
        assert name == "spconv_direct16_kernel"
        return y.cpu().numpy(), part.cpu().numpy().astype(np.float64)

    y0, _ = run()
    monkeypatch.setenv("EPRECON_CONV_BF16X3", "1")
    y1, part = run()
    monkeypatch.delenv("EPRECON_CONV_BF16X3")
    y2, _ = run()
    assert np.array_equal(y0, y2)                                   # the switch is read per launch; off = the exact path
    e32 = (np.abs(y0 - want) / scale).max()
    ebf = (np.abs(y1 - want) / scale).max()
    print(f"{cin}->{cout}: fp32 path {e32:.2e}, bf16x3 {ebf:.2e} of sum |a||w| (max |y - want|: {np.abs(y0 - want).max():.2e} / {np.abs(y1 - want).max():.2e})")
    assert e32 < 2.0 ** -20 and ebf < BF16X3_BUDGET
    assert np.abs(y1 - want).max() < TOL
    cnt, mean, m2 = part[:, 0], part[:, 1], part[:, 2]
    assert cnt[:, 0].sum() == n
    tot_mean = (cnt * mean).sum(0) / n
    tot_m2 = (m2 + cnt * (mean - tot_mean) ** 2).sum(0)
    assert np.abs(tot_mean - y1.mean(0)).max() < 1e-4 and np.abs(tot_m2 / n - y1.var(0)).max() < 1e-3


@pytest.mark.parametrize("cin,cout", [(96, 48), (48, 48), (48, 24), (80, 40)])
def test_stage_depth_rule_changes_the_schedule_not_the_bits(monkeypatch, cin, cout):
    """Round 6: on medium lists (a few workgroups per CU) the direct kernel runs with fewer chunks per prefetch stage when that
    lets one more workgroup share a CU and saves a wave of workgroups (70,001 rows = 547 workgroups against 512 slots).  The
    arithmetic and its order are the same: bit-identical to EPRECON_CONV_STAGE_DEPTH=0."""
    from eprecon_amd import sparse as SP
    rng = np.random.default_rng(cin + cout)
    c = random_coords(rng, 70001, extent=40, batch=1)
    n = len(c)
    vs = SP.VoxelSet(dev(c))
    nbr_d = vs.kernel_map(3)
    x = dev(rng.standard_normal((n, cin)).astype(np.float32))
    w = dev((rng.standard_normal((27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32))
    (y0, p0), name = _last_conv_kernel((27, cin, cout, 1000), lambda: SP.conv_stats(x, w, nbr_d))
    assert name == "spconv_direct16_kernel"
    monkeypatch.setenv("EPRECON_CONV_STAGE_DEPTH", "0")
    y1, p1 = SP.conv_stats(x, w, nbr_d)
    assert torch.equal(y0, y1) and torch.equal(p0, p1)
    ref = OS.sparse_conv(x.cpu().numpy()[:4000 * 0 + n], OS.kernel_map(c, c, 3, 1), w.cpu().numpy()) if cin == 48 and cout == 24 else None
    if ref is not None:
        assert np.abs(y0.cpu().numpy() - ref).max() < TOL


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("cin,cout", [(48, 24), (96, 48), (80, 40), (32, 24), (48, 48), (16, 16), (64, 8), (76, 8), (24, 24),
                                      (40, 24), (8, 16), (56, 32)])
def test_interleaved_schedule_changes_the_schedule_not_the_bits(monkeypatch, cin, cout, affine):
    """Round 6: layers whose consume step holds no launch-uniform branch (no 8-channel or ragged last chunk; with or without a
    pending BatchNorm + ReLU of the input) run on instantiations of the direct kernel that spread the next stage's loads among
    this stage's MFMAs instead of issuing them in a burst behind a scheduling fence.  The products enter every accumulator in the
    same order: bit-identical to EPRECON_CONV_INTERLEAVE=0, summaries included.  (24, 24), (40, 24), (8, 16) have an 8-channel
    last chunk and one stage per offset: their own instantiations (modes 3 / 4); (56, 32) — two stages per offset — stays on the
    general form and must not change either.  Odd and even stage counts both occur (the live-offset count of a wave varies)."""
    from eprecon_amd import sparse as SP
    rng = np.random.default_rng(cin * 7 + cout)
    c = random_coords(rng, 41003, extent=34, batch=1)
    n = len(c)
    vs = SP.VoxelSet(dev(c))
    nbr_d = vs.kernel_map(3)
    x = dev(rng.standard_normal((n, cin)).astype(np.float32))
    w = dev((rng.standard_normal((27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32))
    aff = (dev(rng.uniform(0.5, 1.5, cin).astype(np.float32)), dev(rng.standard_normal(cin).astype(np.float32)), True) if affine else None
    (y0, p0), name = _last_conv_kernel((27, cin, cout, 1000), lambda: SP.conv_stats(x, w, nbr_d, in_affine=aff))
    assert name == "spconv_direct16_kernel"
    monkeypatch.setenv("EPRECON_CONV_INTERLEAVE", "0")
    y1, p1 = SP.conv_stats(x, w, nbr_d, in_affine=aff)
    assert torch.equal(y0, y1) and torch.equal(p0, p1)
    if affine:      # ... and without the ReLU (the branch-free form selects it with a bit mask)
        monkeypatch.delenv("EPRECON_CONV_INTERLEAVE")
        aff2 = (aff[0], aff[1], False)
        y2, _ = SP.conv_stats(x, w, nbr_d, in_affine=aff2)
        monkeypatch.setenv("EPRECON_CONV_INTERLEAVE", "0")
        y3, _ = SP.conv_stats(x, w, nbr_d, in_affine=aff2)
        assert torch.equal(y2, y3) and not torch.equal(y2, y0)
    xa = x.cpu().numpy()
    if affine:
        xa = np.maximum(xa * aff[0].cpu().numpy() + aff[1].cpu().numpy(), 0)
    assert np.abs(y0.cpu().numpy() - OS.sparse_conv(xa, OS.kernel_map(c, c, 3, 1), w.cpu().numpy())).max() < TOL


@pytest.mark.parametrize("n,cin,cout", [(204, 64, 128), (204, 128, 128), (1532, 160, 96), (1532, 64, 64), (1532, 32, 64),
                                        (7561, 32, 32), (9415, 192, 96)])
def test_short_list_kernel(monkeypatch, n, cin, cout):
    """SPVCNN's stride-2 / stride-4 levels and the coarse ConvGRU: the split-K kernel with 4 / 8 / 16 waves per workgroup
    (pipelined stages, narrow inputs included), with the producer's pending BatchNorm on load and the BatchNorm summaries
    of the output in 32-row blocks"""
    from eprecon_amd import sparse as SP
    monkeypatch.setenv("EPRECON_CONV_WIDEK", "0")      # (the 9,415-row case is the cross-workgroup kernel's by default)
    rng = np.random.default_rng(n + cin + cout)
    extent = max(4, int(round((n / 0.3) ** (1 / 3))))
    c = random_coords(rng, n, extent=extent, batch=1)
    n = len(c)
    x = rng.standard_normal((n, cin)).astype(np.float32)
    w = (rng.standard_normal((27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    vs = SP.VoxelSet(dev(c))
    nbr_d, nbr = vs.kernel_map(3), OS.kernel_map(c, c, 3, 1)
    sc = rng.uniform(0.5, 1.5, cin).astype(np.float32)
    sh = rng.standard_normal(cin).astype(np.float32)
    (y, part), name = _last_conv_kernel((27, cin, cout, 1), lambda: SP.conv_stats(
        dev(x), dev(w), nbr_d, in_affine=(dev(sc), dev(sh), True)))
    assert name == "spconv_splitk_kernel"
    ref = OS.sparse_conv(np.maximum(x * sc + sh, 0), nbr, w)
    assert np.abs(y.cpu().numpy() - ref).max() < TOL
    part = part.cpu().numpy().astype(np.float64)
    assert part.shape[0] == (n + 31) // 32 and part[:, 0, 0].sum() == n
    cnt, mean, m2 = part[:, 0], part[:, 1], part[:, 2]
    tot_mean = (cnt * mean).sum(0) / n
    tot_m2 = (m2 + cnt * (mean - tot_mean) ** 2).sum(0)
    assert np.abs(tot_mean - ref.mean(0)).max() < 1e-4 and np.abs(tot_m2 / n - ref.var(0)).max() < 1e-3
    # Round 6: with 16-byte gathers on packed weights the launch takes the branch-free instantiation (packed weights a compile-time
    # fact, every slab its four chunks, the pending BatchNorm its own instantiation: a stage's loads and MFMAs are one basic block).
    # The same products in the same order: bit-identical to the general form (EPRECON_CONV_SPLITK_FAST=0), with and without
    # the pending BatchNorm, with and without its ReLU.
    for aff in ((dev(sc), dev(sh), True), (dev(sc), dev(sh), False), None):
        monkeypatch.delenv("EPRECON_CONV_SPLITK_FAST", raising=False)
        y0, p0 = SP.conv_stats(dev(x), dev(w), nbr_d, in_affine=aff)
        monkeypatch.setenv("EPRECON_CONV_SPLITK_FAST", "0")
        y1, p1 = SP.conv_stats(dev(x), dev(w), nbr_d, in_affine=aff)
        assert torch.equal(y0, y1) and torch.equal(p0, p1)
    assert torch.equal(y0.cpu(), torch.from_numpy(OS.sparse_conv(x, nbr, w))) or np.abs(y0.cpu().numpy() - OS.sparse_conv(x, nbr, w)).max() < TOL


@pytest.mark.parametrize("n,cin,cout", [(9415, 192, 96), (11880, 160, 80), (6000, 128, 128), (4200, 100, 72), (30011, 96, 96)])
def test_medium_list_wide_kernel(n, cin, cout):
    """medium lists with wide channels (the coarsest level's ConvGRU, SPVCNN's up-stage): 128-row workgroups over all columns,
    weight slabs shared through LDS, the 27 offsets split across workgroups, partial sums added in order by the reduce kernel
    which runs the shared epilogue (bias + ReLU + residual, pending BatchNorm on load, 128-row summaries)"""
    from eprecon_amd import sparse as SP
    rng = np.random.default_rng(n + cin + cout)
    extent = max(4, int(round((n / 0.3) ** (1 / 3))))
    c = random_coords(rng, n, extent=extent, batch=1)
    n = len(c)
    x = rng.standard_normal((n, cin)).astype(np.float32)
    w = (rng.standard_normal((27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((n, cout)).astype(np.float32)
    vs = SP.VoxelSet(dev(c))
    nbr_d, nbr = vs.kernel_map(3), OS.kernel_map(c, c, 3, 1)
    ref = OS.sparse_conv(x, nbr, w, b)
    (y, part), name = _last_conv_kernel((27, cin, cout, 1), lambda: SP.sparse_conv_fused(
        dev(x), dev(w), nbr_d, dev(b), relu=True, residual=dev(res), bn_partial=True))
    assert name == "spconv_wide_kernel"
    want = np.maximum(ref, 0) + res
    assert np.abs(y.cpu().numpy() - want).max() < TOL
    part = part.cpu().numpy().astype(np.float64)
    assert part.shape[0] == (n + 127) // 128 and part[:, 0, 0].sum() == n
    cnt, mean, m2 = part[:, 0], part[:, 1], part[:, 2]
    tot_mean = (cnt * mean).sum(0) / n
    tot_m2 = (m2 + cnt * (mean - tot_mean) ** 2).sum(0)
    assert np.abs(tot_mean - want.mean(0)).max() < 1e-4 and np.abs(tot_m2 / n - want.var(0)).max() < 1e-3
    sc = rng.uniform(0.5, 1.5, cin).astype(np.float32)
    sh = rng.standard_normal(cin).astype(np.float32)
    y2, _ = SP.conv_stats(dev(x), dev(w), nbr_d, in_affine=(dev(sc), dev(sh), True))
    ref2 = OS.sparse_conv(np.maximum(x * sc + sh, 0), nbr, w)
    assert np.abs(y2.cpu().numpy() - ref2).max() < TOL


@pytest.mark.parametrize("n,cin,cout,kernel", [(41003, 48, 24, "spconv_direct16_kernel"), (50021, 140, 16, "spconv_direct16_kernel"),
                                               (9415, 192, 96, "spconv_wide_kernel"), (12000, 96, 48, "spconv_splitk_kernel")])
def test_dead_offsets_are_skipped_not_multiplied(n, cin, cout, kernel):
    """voxel sets whose kernel maps are mostly / entirely -1: (a) no two voxels adjacent — ConvGRU's second gate convolution
    runs on such a set (already scaled coordinates divided by the resolution again, models/modules.py:216-217): only the centre
    offset is live and the kernels skip the other 26 —, (b) thin sheets two voxels thick, where whole 32-row groups miss the
    out-of-plane offsets.  Same results as the oracle that sums over the live pairs only."""
    from eprecon_amd import sparse as SP
    rng = np.random.default_rng(n + cin)
    side = int(np.ceil(n ** (1 / 3))) + 1
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)
    iso = g[rng.permutation(len(g))[:n]] * 3                        # spacing 3: no neighbours at all
    sheet = np.stack(np.meshgrid(np.arange(2), np.arange(120), np.arange(max(n // 240, 2)), indexing="ij"), -1).reshape(-1, 3)
    for xyz in (iso, sheet[:n]):
        c = np.concatenate([np.zeros((len(xyz), 1), np.int64), xyz], 1).astype(np.int32)
        x = rng.standard_normal((len(c), cin)).astype(np.float32)
        w = (rng.standard_normal((27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        vs = SP.VoxelSet(dev(c))
        nbr = OS.kernel_map(c, c, 3, 1)
        (y, part), name = _last_conv_kernel((27, cin, cout, 1), lambda: SP.sparse_conv_fused(dev(x), dev(w), vs.kernel_map(3), dev(b),
                                                                                             bn_partial=True))
        if xyz is iso:
            assert (nbr >= 0).sum() == len(c)                       # the centre offset only
        assert name == kernel
        ref = OS.sparse_conv(x, nbr, w, b)
        assert np.abs(y.cpu().numpy() - ref).max() < TOL
        assert float(part[:, 0, 0].sum()) == len(c)


@pytest.mark.parametrize("cin,cout", [(48, 48), (48, 24), (8, 32), (74, 8), (32, 24), (192, 64)])
def test_pointwise_layers_on_long_lists_take_the_direct_kernel(monkeypatch, cin, cout):
    """K = 1 (a per-voxel Linear: SConv3d's skip, SPVCNN's 1x1 convolutions and point MLPs, the fused heads) on a long list:
    the direct kernel as a streaming [N, C_in] x [C_in, C_out] product, with the epilogues those layers use, against the
    oracle and against the kernels short lists stay on"""
    from eprecon_amd import sparse as SP
    monkeypatch.setattr(SP, "K1_DIRECT_MIN_ROWS", 1000)
    rng = np.random.default_rng(cin * 7 + cout)
    n = 50021
    x = rng.standard_normal((n, cin)).astype(np.float32)
    w = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((n, cout)).astype(np.float32)
    cp = (cin + 3) & ~3
    buf = torch.full((n, cp + 4), float("nan"), device="cuda")        # a column slice of a wider buffer, ragged channel counts padded
    buf[:, :cin] = dev(x)
    dx, dw, db = buf[:, :cin], dev(w), dev(b)
    ref = x @ w + b
    (y, part), name = _last_conv_kernel((1, cin, cout, 1), lambda: SP.sparse_conv_fused(dx, dw, None, db, relu=True, residual=dev(res),
                                                                                        bn_partial=True))
    assert name == "spconv_direct16_kernel"
    want = np.maximum(ref, 0) + res
    assert np.abs(y.cpu().numpy() - want).max() < TOL
    part = part.cpu().numpy().astype(np.float64)
    assert part.shape[0] == (n + 127) // 128 and part[:, 0, 0].sum() == n
    tot_mean = (part[:, 0] * part[:, 1]).sum(0) / n
    assert np.abs(tot_mean - want.mean(0)).max() < 1e-4
    # plain call (bias only) through sparse_conv, the producer's pending BatchNorm on load, LayerNorm epilogue
    assert np.abs(SP.sparse_conv(dx, dw, None, db).cpu().numpy() - ref).max() < TOL
    sc, sh = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.standard_normal(cin).astype(np.float32)
    y2, _ = SP.conv_stats(dx, dw, None, in_affine=(dev(sc), dev(sh), True))
    assert np.abs(y2.cpu().numpy() - np.maximum(x * sc + sh, 0) @ w).max() < TOL
    g, be = rng.standard_normal(cout).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
    yl = SP.sparse_conv_ln(dx, dw, None, db, dev(g), dev(be), 1e-5, post_relu=True)
    assert np.abs(yl.cpu().numpy() - OS.layernorm_rows(ref, g, be, 1e-5, None, False, True)).max() < TOL
    # the short-list kernels give the same values
    monkeypatch.setattr(SP, "K1_DIRECT_MIN_ROWS", 10 ** 9)
    y_old, name_old = _last_conv_kernel((1, cin, cout, 1), lambda: SP.sparse_conv(dx, dw, None, db))
    assert name_old != "spconv_direct16_kernel"
    assert np.abs(y_old.cpu().numpy() - ref).max() < TOL


def test_repack_registered_rebuilds_every_packing_in_one_launch():
    """after an in-place update of the weights (an optimizer step), sparse.repack_registered() rebuilds the operand-order copies
    of all of them with one eprecon_conv_pack_many_async launch: the same bits as a fresh per-layer packing, into the same
    buffers, and the caches' tags follow (the layers' next packed_weight / packed_weight16 calls are hits)"""
    from eprecon_amd import sparse as SP
    rng = np.random.default_rng(3)
    shapes = [(27, 48, 24), (27, 96, 48), (27, 32, 32), (1, 24, 24), (27, 76, 8), (27, 160, 96), (9, 40, 64)]
    ws = [torch.nn.Parameter(dev(rng.standard_normal(s).astype(np.float32))) for s in shapes]
    first = []
    for w in ws:
        first.append((SP.packed_weight(w), SP.packed_weight16(w) if w.shape[2] <= 64 else None))
    assert SP.repack_registered() == 0                                  # nothing has changed
    with torch.no_grad():
        for w in ws:
            w.mul_(1.5).add_(0.25)
    n16 = sum(1 for w in ws if w.shape[2] <= 64)
    assert SP.repack_registered() == len(ws) + n16
    for w, (p0, p16) in zip(ws, first):
        assert SP.packed_weight(w) is p0 and (p16 is None or SP.packed_weight16(w) is p16)      # hits, same buffers
        fresh = torch.nn.Parameter(w.detach().clone())
        assert torch.equal(SP.packed_weight(fresh), p0)
        if p16 is not None:
            assert torch.equal(SP.packed_weight16(fresh), p16)
    assert SP.repack_registered() == 0
    del ws, first
