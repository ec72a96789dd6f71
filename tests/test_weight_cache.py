"""The weight-cache contract (eprecon_amd/weight_cache.py) on CPU tensors: the cache itself, every getter that runs without a
GPU through the same sequence of weight changes, and one clear call over a tree of modules."""
import pytest
import torch
import torch.nn as nn


def test_derived_hits_peeks_slots_extra_and_retag():
    from eprecon_amd import weight_cache as WC
    w = torch.arange(6.0).reshape(2, 3)
    built = []

    def build():
        built.append(1)
        return w.t().contiguous()

    assert WC.peek(w, "a") is None and not built                       # peek builds nothing
    a = WC.derived(w, "a", (w,), build)
    assert WC.derived(w, "a", (w,), build) is a and len(built) == 1     # a hit: the identical object
    assert WC.peek(w, "a") is a and WC.peek(w, "b") is None
    b = WC.derived(w, "b", (w,), lambda: w * 2)                         # a second slot on the same owner
    assert WC.peek(w, "a") is a and WC.peek(w, "b") is b and WC.derived(w, "a", (w,), build) is a
    e1 = WC.derived(w, "e", (w,), build, extra=(1, 2, 3))
    assert WC.derived(w, "e", (w,), build, extra=(1, 2, 3)) is e1
    assert WC.derived(w, "e", (w,), build, extra=(1, 3, 2)) is not e1   # extra is part of the tag
    w.add_(1.0)                                                          # a new version: stale
    assert WC.peek(w, "a") is a and not WC.current(w, "a", (w,))
    a.copy_(w.t())                                                       # rewritten in place, as repack_registered does
    WC.retag(w, "a", (w,))
    n = len(built)
    assert WC.current(w, "a", (w,)) and WC.derived(w, "a", (w,), build) is a and len(built) == n
    assert WC.derived(w, "b", (w,), lambda: w * 2) is not b             # the other slot was not retagged


def _decoder():
    from eprecon_amd.mask3dformer import MultiScaleMaskedTransformerDecoder
    return MultiScaleMaskedTransformerDecoder(mask_classification=True, num_classes=20, hidden_dim=48, num_queries=80, nheads=8,
                                              dim_feedforward=192, dec_layers=6, pre_norm=False, mask_dim=48)


def _case(name):
    """-> (module, getter, view of the cached value, the same numbers from the live weights, (submodule, parameter name))"""
    torch.manual_seed(3)
    if name == "linear_wt":
        from eprecon_amd.modules import _linear_wt
        m = nn.Linear(6, 5)
        return m, lambda: _linear_wt(m), lambda v: v, lambda: m.weight.detach().t(), (m, "weight")
    if name == "merged_skip":
        from eprecon_amd.modules import ConvGRU
        m = ConvGRU(hidden_dim=8, input_dim=8, pres=1, vres=0.04)
        lz, lr = m.convz.point_transforms[0], m.convr.point_transforms[0]
        return (m, m._merged_skip, lambda v: torch.cat([v[0].flatten(), v[1]]),
                lambda: torch.cat([torch.cat([lz.weight.detach().t(), lr.weight.detach().t()], 1).flatten(), lz.bias.detach(),
                                   lr.bias.detach()]), (lr, "weight"))
    if name == "dense2d_packed_weight":
        from eprecon_amd.dense2d import packed_weight
        m = nn.Conv2d(4, 6, 3, padding=1)
        return m, lambda: packed_weight(m), lambda v: v, lambda: m.weight.detach().permute(2, 3, 1, 0).reshape(9, 4, 6), (m, "weight")
    if name == "dw_taps":
        from eprecon_amd.backbone import _dw_taps
        m = nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=False)
        return m, lambda: _dw_taps(m), lambda v: v, lambda: m.weight.detach().reshape(8, 9).t(), (m, "weight")
    if name == "pack_mlp4x":
        from eprecon_amd.modules import Linear4xTrans
        from eprecon_amd.sparse import _pack_mlp_weight, pack_mlp4x
        m = Linear4xTrans(24, 1)
        return (m, lambda: pack_mlp4x(m), lambda v: torch.cat([v["w3"], v["g1"][:96]]),        # (norm1 spans 4 C)
                lambda: torch.cat([_pack_mlp_weight(m.linear3.weight.detach().t()), m.norm1.weight.detach()]), (m.linear3, "weight"))
    assert name == "query_side_pack"
    m = _decoder()
    ff = m.transformer_ffn_layers[0]

    def live():       # a transposed weight, and the static head of the untouched queries
        with torch.no_grad():
            return torch.cat([ff.linear1.weight.t().flatten(), m.class_embed(m.decoder_norm(m.query_feat.weight)).flatten()])
    return (m, lambda: m._query_side_pack(torch.device("cpu")),
            lambda v: torch.cat([v["layers"][0]["ffn1_wt"].flatten(), v["cls0"].flatten()]), live, (ff.linear1, "weight"))


@pytest.mark.parametrize("name", ["linear_wt", "merged_skip", "dense2d_packed_weight", "dw_taps", "pack_mlp4x", "query_side_pack"])
def test_every_cpu_getter_follows_the_one_contract(name):
    from eprecon_amd.sparse import clear_packed_weights
    mod, get, view, live, (sub, pname) = _case(name)

    def follows(v):
        return torch.allclose(view(v), live(), rtol=0, atol=1e-6)

    v1 = get()
    assert get() is v1 and follows(v1)                                   # (a) a hit
    with torch.no_grad():
        for p in mod.parameters():
            p.mul_(1.25)
    v2 = get()
    assert v2 is not v1 and follows(v2) and get() is v2                  # (b) an in-place write that bumps the version
    for p in mod.parameters():
        p.data.mul_(1.25)
    assert get() is v2 and not follows(v2)                               # (c) a write through .data: still a hit, stale
    clear_packed_weights(mod)
    v3 = get()
    assert v3 is not v2 and follows(v3) and get() is v3                  # (d) the contract after one
    mod.load_state_dict({k: v * 0.5 if v.is_floating_point() else v.clone() for k, v in mod.state_dict().items()}, assign=True)
    v4 = get()
    assert v4 is not v3 and follows(v4) and get() is v4                  # (e) replaced Parameter objects, no clear call
    setattr(sub, pname, nn.Parameter(getattr(sub, pname).detach() * 2.0))
    v5 = get()
    assert v5 is not v4 and follows(v5) and get() is v5
    mod._apply(lambda t: t.clone())
    v6 = get()
    assert v6 is not v5 and follows(v6) and get() is v6                  # (f) moved storage


def test_one_clear_call_empties_a_tree_of_modules():
    from eprecon_amd import weight_cache as WC
    from eprecon_amd.backbone import _dw_taps
    from eprecon_amd.dense2d import packed_weight
    from eprecon_amd.modules import ConvGRU, Linear4xTrans, _linear_wt
    from eprecon_amd.sparse import clear_packed_weights, pack_mlp4x
    gru, mlp, dec = ConvGRU(hidden_dim=8, input_dim=8, pres=1, vres=0.04), Linear4xTrans(24, 1), _decoder()
    conv, dw = nn.Conv2d(4, 6, 3, padding=1), nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=False)
    tree = nn.ModuleList([gru, mlp, conv, dw, dec])
    lin = gru.convz.point_transforms[0]
    gru._merged_skip(), _linear_wt(lin), pack_mlp4x(mlp), packed_weight(conv), _dw_taps(dw), dec._query_side_pack(torch.device("cpu"))
    WC.derived(conv.weight, "test.on_a_parameter", (conv.weight,), lambda: conv.weight.detach().clone())
    kept = [(gru, "modules.merged_skip"), (lin, "modules.linear_wt"), (mlp, "sparse.pack_mlp4x"), (conv, "dense2d.packed_weight"),
            (dw, "backbone.dw_taps"), (dec, "mask3dformer.query_side_pack"), (dec, "weight_cache.parameter_slots"),
            (conv.weight, "test.on_a_parameter")]
    for owner, slot in kept:
        assert WC.peek(owner, slot) is not None, slot
    clear_packed_weights(tree)
    for owner in list(tree.modules()) + list(tree.parameters()):
        for _, slot in kept:
            assert WC.peek(owner, slot) is None, (type(owner).__name__, slot)
