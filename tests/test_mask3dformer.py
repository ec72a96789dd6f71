"""Mask-transformer head: CPU check of the post-processing against the reference golden vectors;
GPU checks of the decoder (reference state_dict) and of the exact nearest-voxel kernel."""
import os

import numpy as np
import pytest
import torch


def mask3d_inputs(seed=11, c=16):
    rng = np.random.default_rng(seed)
    cells = rng.permutation(np.argwhere(np.ones((10, 10, 10), bool)))[:320] * 4
    c2 = cells[:300]
    c1 = rng.permutation(cells)[:220]
    c1 = np.unique(np.concatenate([c1, c2[:150]]), axis=0)
    c0 = np.unique(np.concatenate([rng.permutation(cells)[:90], c2[100:200]]), axis=0)
    feats = [rng.standard_normal((1, c, len(x))).astype(np.float32) for x in (c0, c1, c2)]
    mask_feat = rng.standard_normal((1, c, len(c2))).astype(np.float32)
    return [c0, c1, c2], feats, mask_feat


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "mask3dformer.npz"))


def test_panoptic_post_matches_reference(gold):
    from eprecon_amd.mask3dformer import panoptic_post
    res = panoptic_post({"pred_logits": torch.from_numpy(gold["pred_logits"]),
                         "pred_masks": torch.from_numpy(gold["pred_masks"])})
    seg, info = res["panoptic_seg"]
    assert seg.dtype == torch.int32 and np.array_equal(seg.numpy(), gold["panoptic_seg"])
    got = np.array([[d["id"], int(d["isthing"]), d["category_id"]] for d in info], np.int64).reshape(-1, 3)
    assert np.array_equal(got, gold["segments"])


def test_panoptic_inference_stuff_merging_and_overlap_rule():
    from eprecon_amd.mask3dformer import panoptic_inference
    q, n = 5, 40
    cls = torch.full((q, 21), -5.0)
    for k, c in enumerate([1, 1, 5, 5, 0]):   # two "wall" queries merge, two chairs stay apart, one empty
        cls[k, c] = 5.0
    m = torch.full((q, n), -6.0)
    m[0, 0:10] = 6.0
    m[1, 10:18] = 6.0
    m[2, 18:26] = 6.0
    m[3, 26:30] = 6.0
    m[3, 18:26] = 5.0   # mostly loses its area to query 2 -> overlap rule drops it? area 4 of 12 < 0.5
    m[4, 30:40] = 6.0
    seg, info = panoptic_inference(cls, m)
    assert [d["category_id"] for d in info] == [1, 5]
    assert seg[0:18].eq(1).all() and seg[18:26].eq(2).all() and seg[26:40].eq(0).all()


@pytest.mark.gpu
def test_panoptic_post_on_the_device_matches_reference_and_the_tensor_path(gold):
    """the two-launch HIP form (owner / confidence / per-query counts in one pass, ids in a second) == the reference's
    golden segmentation, and == the tensor-op path on a larger random case with ties, dropped queries and merged stuff"""
    from eprecon_amd.mask3dformer import panoptic_inference, panoptic_post
    res = panoptic_post({"pred_logits": torch.from_numpy(gold["pred_logits"]).cuda(),
                         "pred_masks": torch.from_numpy(gold["pred_masks"]).cuda()})
    seg, info = res["panoptic_seg"]
    assert seg.dtype == torch.int32 and np.array_equal(seg.cpu().numpy(), gold["panoptic_seg"])
    got = np.array([[d["id"], int(d["isthing"]), d["category_id"]] for d in info], np.int64).reshape(-1, 3)
    assert np.array_equal(got, gold["segments"])
    torch.manual_seed(5)
    q, n = 80, 50021
    cls = torch.randn(q, 21)
    m = torch.randn(q, n) - 6.0
    for k in range(q):                # every query owns a block of voxels (plus noise elsewhere) and has a clear class
        m[k, 600 * k:600 * (k + 1)] += 9.0
        cls[k, [0, 1, 2, 5, 9, 17][k % 6]] += 6.0      # "no object" for every sixth, two stuff classes (merged), things
    m[7] = m[3]                       # exact ties between two queries' logits
    cls[7] = cls[3]
    m[:, -100:] = -20.0               # voxels nobody is confident about
    with torch.no_grad():
        seg_d, info_d = panoptic_inference(cls.cuda(), m.cuda())
        strided = m.t().contiguous().cuda().t()       # same values, voxel-major storage: the tensor-op path on the same device
        assert strided.stride(1) != 1
        seg_h, info_h = panoptic_inference(cls.cuda(), strided)
    assert info_d == info_h and len(info_h) > 3, (info_d, info_h)
    assert torch.equal(seg_d, seg_h), int((seg_d != seg_h).sum())


@pytest.mark.gpu
def test_decoder_matches_reference_golden(gold):
    from eprecon_amd.mask3dformer import MultiScaleMaskedTransformerDecoder
    dec = MultiScaleMaskedTransformerDecoder(mask_classification=True, num_classes=20, hidden_dim=16, num_queries=12,
                                             nheads=4, dim_feedforward=64, dec_layers=4, pre_norm=False, mask_dim=16)
    sd = {k[4:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd__")}
    r = dec.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    dec = dec.cuda()
    coords, feats, mask_feat = mask3d_inputs()
    with torch.no_grad():
        out = dec([torch.from_numpy(f).cuda() for f in feats], [torch.from_numpy(c)[None].cuda() for c in coords],
                  torch.from_numpy(mask_feat).cuda(), (40, 40, 40))
    np.testing.assert_allclose(out["pred_logits"].cpu().numpy(), gold["pred_logits"], atol=2e-4)
    np.testing.assert_allclose(out["pred_masks"].cpu().numpy(), gold["pred_masks"], atol=2e-4)
    np.testing.assert_allclose(out["aux_outputs"][-1]["pred_masks"].cpu().numpy(), gold["aux_last_masks"], atol=2e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("q", [2, 4])
def test_nearest_voxel_is_exact_argmin(q):
    from eprecon_amd.mask3dformer import nearest_fine_index
    rng = np.random.default_rng(q)
    occ = rng.random((24, 24, 24)) < 0.05
    fine = rng.permutation(np.argwhere(occ))
    anc = np.unique(fine // q * q, axis=0)
    # queries: ancestors of fine voxels, plus coarse cells with no descendant (ring / far searches)
    extra = rng.integers(-3, 9, size=(200, 3)) * q
    coarse = np.concatenate([rng.permutation(anc), extra, np.array([[400, 400, 400]])])
    got = nearest_fine_index(torch.from_numpy(coarse).cuda(), torch.from_numpy(fine).cuda(), q).cpu().numpy()
    d = ((coarse[:, None, :].astype(np.int64) - fine[None].astype(np.int64)) ** 2).sum(-1)
    assert np.array_equal(got, d.argmin(1))


@pytest.mark.gpu
def test_decoder_at_cfg4_size_matches_reference_golden(golden_dir):
    """the production decoder (80 queries, 48 channels, 8 heads, 6 layers: models/neucon_network.py:59-71) on 10k / 22k / 30k
    voxels per level — the size the HIP-graph-replayed query side and the SDPA path are tuned for — against the reference's
    own MultiScaleMaskedTransformerDecoder.forward + panoptic_post run on the CPU (tests/golden/make_golden.py)"""
    import sys
    sys.path.insert(0, golden_dir)
    from cases import mask3d_inputs_at_size
    from eprecon_amd.mask3dformer import MultiScaleMaskedTransformerDecoder, panoptic_post
    gold = np.load(os.path.join(golden_dir, "mask3dformer_at_size.npz"))
    dec = MultiScaleMaskedTransformerDecoder(mask_classification=True, num_classes=20, hidden_dim=48, num_queries=80,
                                             nheads=8, dim_feedforward=192, dec_layers=6, pre_norm=False, mask_dim=48)
    sd = {k[4:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd__")}
    r = dec.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    dec = dec.cuda()
    coords, feats, mask_feat = mask3d_inputs_at_size()
    assert [len(c) for c in coords] == gold["n_per_level"].tolist()
    with torch.no_grad():
        for _ in range(3):   # the third call replays the captured query-side graphs
            out = dec([torch.from_numpy(f).cuda() for f in feats], [torch.from_numpy(c)[None].cuda() for c in coords],
                      torch.from_numpy(mask_feat).cuda(), (96, 96, 96))
        post = panoptic_post({"pred_logits": out["pred_logits"], "pred_masks": out["pred_masks"]})
    cols = gold["mask_cols"]
    masks = out["pred_masks"][0].cpu().numpy()
    # fp32 sums over up to 30k keys in another order than the CPU's: 1e-3 (north_star's tolerance), observed ~1e-4
    np.testing.assert_allclose(out["pred_logits"].cpu().numpy(), gold["pred_logits"], atol=1e-3)
    np.testing.assert_allclose(masks[:, cols], gold["pred_masks_sampled"], atol=1e-3)
    np.testing.assert_allclose(out["aux_outputs"][-1]["pred_masks"][0].cpu().numpy()[:, cols], gold["aux_last_masks_sampled"], atol=1e-3)
    np.testing.assert_allclose(masks.astype(np.float64).sum(1), gold["pred_masks_rowsum"], rtol=1e-4, atol=0.5)
    # labels: identical wherever the decision does not hang on the last bits (margin of the winning query's score x mask)
    seg = post["panoptic_seg"][0].cpu().numpy()
    decided = gold["label_margin"] > 2e-3
    assert decided.mean() > 0.5
    assert np.array_equal(seg[decided], gold["panoptic_seg"][decided])
    got = np.array([[d["id"], int(d["isthing"]), d["category_id"]] for d in post["panoptic_seg"][1]], np.int64).reshape(-1, 3)
    assert np.array_equal(got, gold["segments"])


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_fine,identity", [(10007, 30011, False), (30011, 30011, True), (63, 500, False), (4097, 4097, True)])
def test_masked_attention_kernel_matches_dense_sdpa(n, n_fine, identity):
    """csrc/decoder.hip against the dense formulation of models/mask3dformer.py:383-397,441-443: mask = sigmoid(mask logits at
    the level's voxels) < 0.5, an all-blocked query attends to everything, nn.MultiheadAttention's scaled softmax per head"""
    import torch.nn.functional as F
    from eprecon_amd.mask3dformer import masked_attention
    g = torch.Generator().manual_seed(n)
    h, nq, d = 8, 80, 6
    q = torch.randn((1, h, nq, d), generator=g).cuda()
    k = (torch.randn((n, h * d), generator=g) * 1.5).cuda()
    v = torch.randn((n, h * d), generator=g).cuda()
    logits_t = torch.randn((n_fine, nq), generator=g).cuda()
    logits_t[:, 3] = -5.0           # query 3: every key blocked -> attends to all keys
    logits_t[:, 7] = 4.0            # query 7: nothing blocked
    logits_t[:, 11] = -5.0
    rows = None if identity else torch.randint(0, n_fine, (n,), generator=g).to(torch.int32).cuda()
    if not identity:
        logits_t[rows[5].long(), 11] = 2.0   # query 11: exactly one allowed key
    out = torch.full((1, h, nq, d), float("nan"), device="cuda")
    masked_attention(q, k, v, logits_t, rows, out, 1.0 / d ** 0.5)
    sel = logits_t if identity else logits_t.index_select(0, rows.long())
    blocked = (sel.t().sigmoid() < 0.5)
    blocked = blocked & ~blocked.all(dim=-1, keepdim=True)
    split = lambda t: t.view(n, h, d).transpose(0, 1).unsqueeze(0)
    ref = F.scaled_dot_product_attention(q, split(k), split(v), attn_mask=~blocked)
    assert torch.isfinite(out).all()
    assert float((out - ref).abs().max()) < 2e-5
    # without a mask
    masked_attention(q, k, v, None, None, out, 1.0 / d ** 0.5)
    assert float((out - F.scaled_dot_product_attention(q, split(k), split(v))).abs().max()) < 2e-5
    # deterministic: a second run gives the same bits
    again = torch.empty_like(out)
    masked_attention(q, k, v, None, None, again, 1.0 / d ** 0.5)
    assert torch.equal(out, again)


@pytest.mark.gpu
def test_decoder_level_inputs_match_the_torch_sequence():
    """src = feats + level_embed, keys = src + Fourier position encoding (models/mask3dformer.py:346-357) in one launch"""
    from eprecon_amd.mask3dformer import MultiScaleMaskedTransformerDecoder, decoder_level_inputs
    torch.manual_seed(3)
    dec = MultiScaleMaskedTransformerDecoder(mask_classification=True, num_classes=20, hidden_dim=48, num_queries=80,
                                             nheads=8, dim_feedforward=192, dec_layers=6, pre_norm=False, mask_dim=48).cuda()
    n = 5003
    coords4 = torch.randint(0, 96, (n, 4), dtype=torch.int32).cuda()
    xyz = coords4[:, 1:]                                       # a strided view, as NeuConNet hands it over
    feats = torch.randn((n, 56)).cuda()[:, :48]                # rows with a pitch
    with torch.no_grad():
        src, keys = decoder_level_inputs(xyz, feats, dec.level_embed.weight[1], dec.pos_enc.gauss_B, (96, 96, 96))
        pos = dec.get_pos_encs([xyz[None]], (96, 96, 96))[0]   # [1, 48, N]
        ref_src = feats + dec.level_embed.weight[1][None]
    assert float((src - ref_src).abs().max()) == 0.0
    assert float((keys - (ref_src + pos[0].t())).abs().max()) < 2e-5


@pytest.mark.gpu
def test_fused_voxel_side_equals_the_dense_path_at_cfg4_size(golden_dir):
    """the decoder with the HIP voxel side against the same decoder on PyTorch ops (dense [Q, N] masks + SDPA)"""
    import sys
    sys.path.insert(0, golden_dir)
    from cases import mask3d_inputs_at_size
    from eprecon_amd.mask3dformer import MultiScaleMaskedTransformerDecoder
    gold = np.load(os.path.join(golden_dir, "mask3dformer_at_size.npz"))
    dec = MultiScaleMaskedTransformerDecoder(mask_classification=True, num_classes=20, hidden_dim=48, num_queries=80,
                                             nheads=8, dim_feedforward=192, dec_layers=6, pre_norm=False, mask_dim=48)
    dec.load_state_dict({k[4:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd__")}, strict=True)
    dec = dec.cuda()
    coords, feats, mask_feat = mask3d_inputs_at_size()
    args = ([torch.from_numpy(f).cuda() for f in feats], [torch.from_numpy(c)[None].cuda() for c in coords],
            torch.from_numpy(mask_feat).cuda(), (96, 96, 96))
    with torch.no_grad():
        assert dec.use_fused_voxel_side
        fused = dec(*args)
        dec.use_fused_voxel_side = False
        dense = dec(*args)
    assert fused["pred_masks"].shape == dense["pred_masks"].shape
    # (six layers of fp32 sums over up to 30k keys in two different orders: observed 2e-4 on the class logits)
    assert float((fused["pred_logits"] - dense["pred_logits"]).abs().max()) < 5e-4
    assert float((fused["pred_masks"] - dense["pred_masks"]).abs().max()) < 1e-3
    for a, b in zip(fused["aux_outputs"], dense["aux_outputs"]):
        assert float((a["pred_logits"] - b["pred_logits"]).abs().max()) < 5e-4


@pytest.mark.gpu
@pytest.mark.parametrize("j", [0, 5])
def test_query_side_kernels_match_the_torch_modules(j):
    """csrc/decoder.hip query_side_a / _b against the PyTorch modules they replace (cross-attention out-projection + LN,
    nn.MultiheadAttention self-attention, FFN, decoder_norm + class / mask embeddings, next layer's projected queries)"""
    from eprecon_amd.mask3dformer import MultiScaleMaskedTransformerDecoder
    torch.manual_seed(11 + j)
    dec = MultiScaleMaskedTransformerDecoder(mask_classification=True, num_classes=20, hidden_dim=48, num_queries=80,
                                             nheads=8, dim_feedforward=192, dec_layers=6, pre_norm=False, mask_dim=48).cuda()
    for prm in dec.parameters():                      # biases / LayerNorm parameters away from their 0 / 1 defaults
        if prm.dim() == 1:
            prm.data.normal_(0.3, 0.5)
    o_attn = torch.randn((1, 8, 80, 6), device="cuda")
    state = torch.randn((80, 48), device="cuda")
    qe = dec.query_embed.weight.unsqueeze(1)
    with torch.no_grad():
        ref_state, ref_cls, ref_me, ref_q = dec._query_side(j, o_attn, state.unsqueeze(1), qe)
        pack = dec._query_side_pack(state.device)
        outs = torch.full((3, 80, 48), float("nan"), device="cuda")
        cls_out = torch.full((80, 21), float("nan"), device="cuda")
        ws = torch.empty((4, 80, 48), device="cuda")
        got_state, got_cls, got_me, got_q = dec._query_side_hip(pack, j, o_attn, state, outs, cls_out, ws)
    assert float((got_state - ref_state[:, 0]).abs().max()) < 2e-5
    assert float((got_cls - ref_cls).abs().max()) < 5e-5
    assert float((got_me - ref_me).abs().max()) < 5e-5
    if j == 5:
        assert ref_q is None and got_q is None
    else:
        assert got_q.shape == ref_q.shape and float((got_q - ref_q).abs().max()) < 5e-5


@pytest.mark.gpu
def test_decoder_follows_rewritten_and_replaced_weights(golden_dir):
    """The decoder keeps copies of its weights (the fused path's transposed matrices and static first head, the graph path's
    captured query side).  After (a) a write through `p.data` + sparse.clear_packed_weights and (b) replaced Parameter objects
    (load_state_dict(assign=True), no clear call), both must agree with the PyTorch-module path of the same decoder, which
    reads the live weights, within the tolerances of test_fused_voxel_side_equals_the_dense_path_at_cfg4_size, and must differ
    from their own result before the change by ten times those.  (The decoder is the cfg4 one on the small inputs: the
    16-channel decoder of test_decoder_matches_reference_golden has 4 channels per head, which the fused path does not take.)"""
    from eprecon_amd import weight_cache
    from eprecon_amd.mask3dformer import MultiScaleMaskedTransformerDecoder
    from eprecon_amd.sparse import clear_packed_weights
    gold = np.load(os.path.join(golden_dir, "mask3dformer_at_size.npz"))
    dec = MultiScaleMaskedTransformerDecoder(mask_classification=True, num_classes=20, hidden_dim=48, num_queries=80,
                                             nheads=8, dim_feedforward=192, dec_layers=6, pre_norm=False, mask_dim=48)
    dec.load_state_dict({k[4:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd__")}, strict=True)
    dec = dec.cuda()
    coords, feats, mask_feat = mask3d_inputs(c=48)
    args = ([torch.from_numpy(f).cuda() for f in feats], [torch.from_numpy(c)[None].cuda() for c in coords],
            torch.from_numpy(mask_feat).cuda(), (40, 40, 40))
    tol = {"pred_logits": 5e-4, "pred_masks": 1e-3}

    def run(fused, graph):
        dec.use_fused_voxel_side, dec.use_hip_graph = fused, graph
        with torch.no_grad():
            out = dec(*args)
        return {k: out[k].clone() for k in tol}

    def step(before=None):
        got = {"fused": run(True, False), "graph": run(False, True)}
        assert weight_cache.peek(dec, "mask3dformer.query_side_pack") is not None       # the paths meant did run
        assert weight_cache.peek(dec, "mask3dformer.static_plan") is not None
        live = run(False, False)
        for path, out in got.items():
            for k, t in tol.items():
                err = float((out[k] - live[k]).abs().max())
                moved = None if before is None else float((out[k] - before[path][k]).abs().max())
                print(f"{path} {k}: against the live weights {err:.3g}, against its result before the change {moved}")
                assert err < t, (path, k, err)
                assert moved is None or moved >= 10 * t, (path, k, moved)
        return got

    first = step()
    for p in dec.parameters():                  # (a) neither the version counter nor the pointer moves
        p.data.mul_(1.25)
    clear_packed_weights(dec)
    second = step(first)
    dec.load_state_dict({k: v * 0.5 for k, v in dec.state_dict().items()}, assign=True)      # (b) new objects, no clear call
    step(second)
