"""Mask-transformer panoptic head on three voxel levels — mirror of models/mask3dformer.py
(MultiScaleMaskedTransformerDecoder :198-445, panoptic_post / panoptic_inference :462-581) and of the
Fourier positional encoding of models/voxel_position_encoding.py:123-152.

The decoder is dense attention over 80 queries and stays PyTorch-ROCm (rocBLAS / SDPA), as
BASELINE.json prescribes; parameter names follow the reference, so its state_dict loads as is.
The one quadratic piece, the `cdist` + `argmin` nearest finest-level voxel of every coarser voxel
(:361-367, [N2 x N0] and [N2 x N1] float distance matrices), is replaced by an exact integer
nearest-neighbour search over the hash grid of the finest level (csrc/nearest.hip): first-index
tie-break like argmin, no N2 x N matrix.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, weight_cache
from . import sparse as SP


class PositionEmbeddingCoordsSine(nn.Module):
    """Fourier features of normalised voxel coordinates (pos_type "fourier", normalize=True):
    sin / cos of 2*pi * x_norm @ gauss_B, gauss_B ~ N(0, gauss_scale) of shape [3, d_pos/2]."""

    def __init__(self, temperature=10000, normalize=False, scale=None, pos_type="fourier", d_pos=None, d_in=3,
                 gauss_scale=1.0):
        super().__init__()
        assert pos_type == "fourier" and d_pos is not None and d_pos % 2 == 0
        self.d_pos, self.normalize = d_pos, normalize
        self.register_buffer("gauss_B", torch.randn(d_in, d_pos // 2) * gauss_scale)

    def forward(self, xyz, num_channels=None, input_range=None):
        """xyz f32[B, N, 3] -> f32[B, d_pos, N]"""
        with torch.no_grad():
            x = xyz.clone()
            if self.normalize:
                lo, hi = input_range
                x = (x - lo[:, None, :]) * 1.0 / (hi[:, None, :] - lo[:, None, :]) + 0.0
            x = x * (2 * math.pi)
            b, n, _ = x.shape
            proj = torch.mm(x.view(-1, 3), self.gauss_B).view(b, n, -1)
            return torch.cat([proj.sin(), proj.cos()], dim=2).permute(0, 2, 1)


class _Attention(nn.Module):
    """post-norm residual attention block; `name` selects the reference's attribute name so that
    the state_dict keys match (self_attn / multihead_attn)"""

    def __init__(self, d_model, nhead, name):
        super().__init__()
        setattr(self, name, nn.MultiheadAttention(d_model, nhead, dropout=0.0))
        self._name = name
        self.norm = nn.LayerNorm(d_model)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, tgt, memory, attn_mask, pos, query_pos):
        attn = getattr(self, self._name)
        q = tgt + query_pos
        k = memory if pos is None else memory + pos
        upd = attn(query=q, key=k, value=memory, attn_mask=attn_mask)[0]
        return self.norm(tgt + upd)

    def project_kv(self, key_in, value_in):
        """in-projection of the keys / values of one level ([N, 1, C] each) -> per-head [1, H, N, C/H] tensors"""
        attn = getattr(self, self._name)
        c, h = attn.embed_dim, attn.num_heads
        w, b = attn.in_proj_weight, attn.in_proj_bias
        k = F.linear(key_in.squeeze(1), w[c:2 * c], b[c:2 * c])
        v = F.linear(value_in.squeeze(1), w[2 * c:], b[2 * c:])
        split = lambda t: t.view(t.shape[0], h, c // h).transpose(0, 1).unsqueeze(0)
        return split(k), split(v)

    def attend(self, tgt, query_pos, kv, blocked=None):
        """the same block on pre-projected keys / values with ONE [Q, N] mask shared by all heads (the reference
        repeats it per head, models/mask3dformer.py:441-443): nn.MultiheadAttention's arithmetic
        (scaled q . k, blocked logits = -inf, softmax, weighted values, out-projection) through SDPA, without the
        head-averaged attention weights the module would also return.  blocked: bool[Q, N], True = masked."""
        attn = getattr(self, self._name)
        c, h = attn.embed_dim, attn.num_heads
        w, b = attn.in_proj_weight, attn.in_proj_bias
        q = F.linear((tgt + query_pos).squeeze(1), w[:c], b[:c])
        q = q.view(q.shape[0], h, c // h).transpose(0, 1).unsqueeze(0)
        allowed = None if blocked is None else ~blocked
        o = F.scaled_dot_product_attention(q, kv[0], kv[1], attn_mask=allowed)
        o = o.squeeze(0).transpose(0, 1).reshape(-1, c)
        upd = F.linear(o, attn.out_proj.weight, attn.out_proj.bias).unsqueeze(1)
        return self.norm(tgt + upd)


class SelfAttentionLayer(_Attention):
    def __init__(self, d_model, nhead, dropout=0.0, activation="relu", normalize_before=False):
        assert not normalize_before and dropout == 0.0
        super().__init__(d_model, nhead, "self_attn")

    def forward(self, tgt, tgt_mask=None, tgt_key_padding_mask=None, query_pos=None):
        q = tgt + query_pos
        upd = self.self_attn(q, q, value=tgt, attn_mask=tgt_mask, need_weights=False)[0]
        return self.norm(tgt + upd)


class CrossAttentionLayer(_Attention):
    def __init__(self, d_model, nhead, dropout=0.0, activation="relu", normalize_before=False):
        assert not normalize_before and dropout == 0.0
        super().__init__(d_model, nhead, "multihead_attn")

    def forward(self, tgt, memory, memory_mask=None, memory_key_padding_mask=None, pos=None, query_pos=None):
        return super().forward(tgt, memory, memory_mask, pos, query_pos)


class FFNLayer(nn.Module):
    def __init__(self, d_model, dim_feedforward=2048, dropout=0.0, activation="relu", normalize_before=False):
        super().__init__()
        assert not normalize_before and dropout == 0.0
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm = nn.LayerNorm(d_model)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, tgt):
        return self.norm(tgt + self.linear2(F.relu(self.linear1(tgt))))


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        dims = [input_dim] + [hidden_dim] * (num_layers - 1) + [output_dim]
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = layer(x)
            if i + 1 < len(self.layers):
                x = F.relu(x)
        return x


def decoder_level_inputs(coords_xyz, feats_rows, level_embed, gauss_b, spitial_shape):
    """(src, keys) of one level as voxel rows f32[N, C]: src = feats + level_embed, keys = src + Fourier position encoding
    (models/mask3dformer.py:346-357, models/voxel_position_encoding.py:123-152) in ONE launch (csrc/decoder.hip).
    coords_xyz int32[N,3] (any row pitch), feats_rows f32[N, C] (row-major, any pitch)"""
    import ctypes
    lib = _lib.load()
    n, c = feats_rows.shape
    assert coords_xyz.dtype == torch.int32 and coords_xyz.stride(1) == 1 and feats_rows.stride(1) == 1
    src = torch.empty((n, c), dtype=torch.float32, device=feats_rows.device)
    keys = torch.empty_like(src)
    ext = (ctypes.c_float * 3)(*[float(v) for v in spitial_shape])
    _lib.check(lib.eprecon_decoder_keys_async(_lib.ptr(coords_xyz), coords_xyz.stride(0), _lib.ptr(feats_rows), feats_rows.stride(0),
                                              _lib.ptr(level_embed), _lib.ptr(gauss_b), ctypes.cast(ext, ctypes.c_void_p), n, c,
                                              _lib.ptr(src), _lib.ptr(keys), _lib.current_stream()), "eprecon_decoder_keys_async")
    return src, keys


def masked_attention(q, k, v, mask_logits_t, mask_rows, out, scale):
    """out[1, H, Q, D] = the scaled-dot-product attention of nn.MultiheadAttention over the voxel rows k / v f32[N, H * D]
    with the attention mask `sigmoid(mask_logits_t[mask_rows[n], i]) < 0.5 -> key n blocked for query i` (a query with every
    key blocked attends to all; models/mask3dformer.py:383-397,441-443) — without the [Q, N] mask, the [H, Q, N] scores or
    the index_select of the mask logits (csrc/decoder.hip: split-K flash attention, deterministic).
    q f32[1, H, Q, D] (any head / query strides: the head-split view of the in-projection is taken as is);
    mask_logits_t f32[N_fine, Q]; mask_rows int32[N] or None (identity)."""
    lib = _lib.load()
    _, h, nq, d = q.shape
    n = k.shape[0]
    assert q.stride(3) == 1 and out.is_contiguous() and out.shape == q.shape and k.stride(1) == 1 and v.stride(1) == 1
    ws = _lib.workspace(lib.eprecon_masked_attention_workspace_bytes(n, nq, h, d), q.device)
    _lib.check(lib.eprecon_masked_attention_async(
        _lib.ptr(q), q.stride(1), q.stride(2), _lib.ptr(k), k.stride(0), _lib.ptr(v), v.stride(0), n, _lib.ptr(mask_logits_t),
        mask_logits_t.stride(0) if mask_logits_t is not None else 0, _lib.ptr(mask_rows),
        mask_logits_t.shape[0] if mask_logits_t is not None else 0, nq, h, d, float(scale), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
        _lib.current_stream()), "eprecon_masked_attention_async")
    return out


def nearest_fine_index(coarse_xyz, fine_xyz, quantum, as_int32=False):
    """for every coarse voxel (multiple of `quantum`) the row of the nearest fine voxel (Euclidean on
    integer coordinates, smallest row on ties) — what argmin(cdist(fine, coarse), dim=0) returns when
    distances are exact.  coarse int[M,3], fine int[N,3] -> int64[M] (int32 on request)"""
    lib = _lib.load()
    dev = fine_xyz.device

    def with_batch(c):
        return torch.cat([torch.zeros_like(c[:, :1]), c], dim=1).to(torch.int32).contiguous()

    fine, coarse = with_batch(fine_xyz), with_batch(coarse_xyz)
    grid = SP.HashGrid(fine.shape[0], dev).build(fine)
    out = torch.empty(coarse.shape[0], dtype=torch.int32, device=dev)
    _lib.check(lib.eprecon_nearest_voxel_async(_lib.ptr(grid.mem), grid.capacity, _lib.ptr(fine), fine.shape[0],
                                               _lib.ptr(coarse), coarse.shape[0], int(quantum), _lib.ptr(out),
                                               _lib.current_stream()), "eprecon_nearest_voxel_async")
    return out if as_int32 else out.long()


class MultiScaleMaskedTransformerDecoder(nn.Module):
    def __init__(self, mask_classification=True, *, num_classes, hidden_dim, num_queries, nheads, dim_feedforward,
                 dec_layers, pre_norm, mask_dim):
        super().__init__()
        assert mask_classification and not pre_norm
        self.num_queries, self.num_heads, self.num_layers = num_queries, nheads, dec_layers
        self.query_feat = nn.Embedding(num_queries, hidden_dim)
        self.query_embed = nn.Embedding(num_queries, hidden_dim)
        self.pos_enc = PositionEmbeddingCoordsSine(pos_type="fourier", d_pos=mask_dim, gauss_scale=1.0, normalize=True)
        self.transformer_self_attention_layers = nn.ModuleList(
            SelfAttentionLayer(hidden_dim, nheads) for _ in range(dec_layers))
        self.transformer_cross_attention_layers = nn.ModuleList(
            CrossAttentionLayer(hidden_dim, nheads) for _ in range(dec_layers))
        self.transformer_ffn_layers = nn.ModuleList(
            FFNLayer(hidden_dim, dim_feedforward) for _ in range(dec_layers))
        self.decoder_norm = nn.LayerNorm(hidden_dim)
        self.num_feature_levels = 3
        self.level_embed = nn.Embedding(self.num_feature_levels, hidden_dim)
        self.class_embed = nn.Linear(hidden_dim, num_classes + 1)
        self.mask_embed = MLP(hidden_dim, hidden_dim * 4, mask_dim, 3)
        # the static-shape query side of every layer replayed from HIP graphs on the GPU inference path
        self.use_hip_graph = __import__("os").environ.get("EPRECON_NO_GRAPH", "0") != "1"
        # EPRECON_DECODER_FUSED=0: the decoder on PyTorch ops (key / value projections, SDPA over a dense [Q, N] mask, the query
        # side replayed from HIP graphs) instead of the HIP kernels of csrc/decoder.hip
        self.use_fused_voxel_side = __import__("os").environ.get("EPRECON_DECODER_FUSED", "1") == "1"

    def get_pos_encs(self, coords, spitial_shape):
        out = []
        for level in coords:
            for c in level:  # batch dimension (always 1 here)
                lo = torch.zeros((1, 3), dtype=torch.float32, device=c.device)
                hi = torch.tensor([list(spitial_shape)], dtype=torch.float32, device=c.device)
                out.append(self.pos_enc(c[None].float(), input_range=[lo, hi]))
        return out

    def forward_prediction_heads(self, output, mask_features, attn_mask_target_size, mask_indices):
        """models/mask3dformer.py:429-445; the attention mask is returned as ONE bool[Q, N_level] (True = blocked):
        the reference's per-head copies are identical"""
        dec = self.decoder_norm(output).transpose(0, 1)
        outputs_class = self.class_embed(dec)
        outputs_mask = torch.einsum("bqc,bcl->bql", self.mask_embed(dec), mask_features)
        attn = outputs_mask[0] if mask_indices is None else outputs_mask[0].index_select(1, mask_indices)
        return outputs_class, outputs_mask, (attn.sigmoid() < 0.5).detach()

    # ---- query side of a layer: everything between two cross-attentions has the STATIC shape [Q, C] ----------------
    def _project_q(self, j, output, query_embed):
        """in-projected, head-split queries of layer j's cross-attention: [1, H, Q, C/H]"""
        attn = self.transformer_cross_attention_layers[j].multihead_attn
        c, h = attn.embed_dim, attn.num_heads
        q = F.linear((output + query_embed).squeeze(1), attn.in_proj_weight[:c], attn.in_proj_bias[:c])
        return q.view(q.shape[0], h, c // h).transpose(0, 1).unsqueeze(0)

    def _head_static(self, output):
        dec = self.decoder_norm(output).transpose(0, 1)
        return self.class_embed(dec), self.mask_embed(dec)

    def _query_side(self, j, o_attn, output, query_embed):
        """after the scaled-dot-product of layer j's cross-attention (o_attn [1, H, Q, C/H]): out-projection +
        residual + LayerNorm, self-attention, FFN, the prediction head's class / mask embeddings and the next
        layer's projected queries"""
        cross = self.transformer_cross_attention_layers[j]
        attn = cross.multihead_attn
        o = o_attn.squeeze(0).transpose(0, 1).reshape(-1, attn.embed_dim)
        output = cross.norm(output + F.linear(o, attn.out_proj.weight, attn.out_proj.bias).unsqueeze(1))
        output = self.transformer_self_attention_layers[j](output, query_pos=query_embed)
        output = self.transformer_ffn_layers[j](output)
        cls, me = self._head_static(output)
        q_next = self._project_q(j + 1, output, query_embed) if j + 1 < self.num_layers else None
        return output, cls, me, q_next

    def _static_plan(self, device):
        """Inference on the GPU: the query side of every layer captured once into a HIP graph (7 small GEMMs, two
        LayerNorms, an 80 x 80 attention, ... per layer -> one replay), chained through static tensors; re-captured
        when a parameter changes (cached: weight_cache).  Returns None when graphs cannot be used (CPU, autograd)."""
        if device.type != "cuda" or torch.is_grad_enabled() or not self.use_hip_graph:
            return None
        return weight_cache.derived(self, "mask3dformer.static_plan", weight_cache.parameter_sources(self),
                                    lambda: self._capture_plan(device))

    def _capture_plan(self, device):
        qe = self.query_embed.weight.unsqueeze(1)
        attn0 = self.transformer_cross_attention_layers[0].multihead_attn
        h, c = attn0.num_heads, attn0.embed_dim
        state = self.query_feat.weight.unsqueeze(1)
        side = _lib.side_stream(device, _lib.SIDE_SETUP)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            cls0, me0 = self._head_static(state)
            q0 = self._project_q(0, state, qe)
            o_in = [torch.zeros((1, h, self.num_queries, c // h), device=device) for _ in range(self.num_layers)]
            for j in range(self.num_layers):     # warm-up outside the capture (first-use work of the libraries)
                self._query_side(j, o_in[j], state, qe)
        torch.cuda.current_stream(device).wait_stream(side)
        layers = []
        for j in range(self.num_layers):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                state, cls, me, q_next = self._query_side(j, o_in[j], state, qe)
            layers.append({"graph": g, "o_in": o_in[j], "cls": cls, "me": me, "q_next": q_next})
        return {"cls0": cls0, "me0": me0, "q0": q0, "layers": layers}

    def _mask_and_block(self, me, mask_features, mask_indices):
        """mask logits [1, Q, N2] of a prediction head and the attention mask bool[Q, N_level] (True = blocked)"""
        outputs_mask = torch.einsum("bqc,bcl->bql", me, mask_features)
        attn = outputs_mask[0] if mask_indices is None else outputs_mask[0].index_select(1, mask_indices)
        return outputs_mask, (attn.sigmoid() < 0.5).detach()

    def _query_side_pack(self, device):
        """Everything the HIP query side needs (cached: weight_cache): every weight matrix transposed to [in][out]
        (contiguous), the prediction head of the UNTOUCHED queries (static: models/mask3dformer.py:376-381 runs it before the
        first layer) and the first layer's projected queries."""
        return weight_cache.derived(self, "mask3dformer.query_side_pack", weight_cache.parameter_sources(self),
                                    self._build_query_side_pack, (device,))

    def _build_query_side_pack(self):
        t = lambda w: w.detach().t().contiguous()
        v = lambda x: x.detach().contiguous()
        layers = []
        for j in range(self.num_layers):
            ca = self.transformer_cross_attention_layers[j]
            sa = self.transformer_self_attention_layers[j]
            ff = self.transformer_ffn_layers[j]
            c = ca.multihead_attn.embed_dim
            w = {"cross_out_wt": t(ca.multihead_attn.out_proj.weight), "cross_out_b": v(ca.multihead_attn.out_proj.bias),
                 "cross_ln_g": v(ca.norm.weight), "cross_ln_b": v(ca.norm.bias),
                 "self_in_wt": t(sa.self_attn.in_proj_weight), "self_in_b": v(sa.self_attn.in_proj_bias),
                 "self_out_wt": t(sa.self_attn.out_proj.weight), "self_out_b": v(sa.self_attn.out_proj.bias),
                 "self_ln_g": v(sa.norm.weight), "self_ln_b": v(sa.norm.bias),
                 "ffn1_wt": t(ff.linear1.weight), "ffn1_b": v(ff.linear1.bias), "ffn2_wt": t(ff.linear2.weight), "ffn2_b": v(ff.linear2.bias),
                 "ffn_ln_g": v(ff.norm.weight), "ffn_ln_b": v(ff.norm.bias),
                 "dec_ln_g": v(self.decoder_norm.weight), "dec_ln_b": v(self.decoder_norm.bias),
                 "cls_wt": t(self.class_embed.weight), "cls_b": v(self.class_embed.bias)}
            for i, lin in enumerate(self.mask_embed.layers):
                w[f"m{i + 1}_wt"], w[f"m{i + 1}_b"] = t(lin.weight), v(lin.bias)
            if j + 1 < self.num_layers:
                nxt = self.transformer_cross_attention_layers[j + 1].multihead_attn
                w["next_q_wt"], w["next_q_b"] = t(nxt.in_proj_weight[:c]), v(nxt.in_proj_bias[:c])
            layers.append(w)
        # key / value in-projections of the layers that attend to the same level, side by side: [C][n_layers_of_level * C]
        kv_levels = []
        for lvl in range(self.num_feature_levels):
            js = [j for j in range(self.num_layers) if j % self.num_feature_levels == lvl]
            mh = [self.transformer_cross_attention_layers[j].multihead_attn for j in js]
            c = mh[0].embed_dim
            kv_levels.append({"layers": js,
                              "wk": torch.cat([t(m.in_proj_weight[c:2 * c]) for m in mh], 1).contiguous(),
                              "bk": torch.cat([v(m.in_proj_bias[c:2 * c]) for m in mh]).contiguous(),
                              "wv": torch.cat([t(m.in_proj_weight[2 * c:]) for m in mh], 1).contiguous(),
                              "bv": torch.cat([v(m.in_proj_bias[2 * c:]) for m in mh]).contiguous()})
        state0 = self.query_feat.weight.detach().unsqueeze(1)
        qe = self.query_embed.weight.detach().unsqueeze(1)
        with torch.no_grad():
            cls0, me0 = self._head_static(state0)
            q0 = self._project_q(0, state0, qe)
        # the kernel evaluates every LayerNorm of the query side with ONE eps (1e-5): all four kinds must carry it
        ok = (len(self.mask_embed.layers) == 3 and self.decoder_norm.eps == 1e-5 and
              all(l.norm.eps == 1e-5 for l in self.transformer_ffn_layers) and
              all(l.norm.eps == 1e-5 for l in self.transformer_cross_attention_layers) and
              all(l.norm.eps == 1e-5 for l in self.transformer_self_attention_layers))
        return {"layers": layers, "kv_levels": kv_levels, "cls0": cls0.contiguous(), "me0": me0.contiguous(), "q0": q0, "ok": ok,
                "state0": self.query_feat.weight.detach().contiguous(), "qpos": self.query_embed.weight.detach().contiguous(),
                "ffn_dim": self.transformer_ffn_layers[0].linear1.out_features, "n_cls": self.class_embed.out_features,
                "mask_hidden": self.mask_embed.layers[0].out_features}

    def _query_side_hip(self, pack, j, o_attn, state, outs, cls_out, ws):
        """one layer's query side on csrc/decoder.hip (two launches): -> (state, class logits [1, Q, K+1], mask embedding
        [1, Q, C], next layer's head-split queries | None)"""
        import ctypes
        lib = _lib.load()
        w = pack["layers"][j]
        q_n, c = state.shape
        d = _lib.DecoderLayerDesc()
        d.n_queries, d.channels, d.n_heads = q_n, c, self.num_heads
        d.ffn_dim, d.n_class_logits, d.mask_hidden = pack["ffn_dim"], pack["n_cls"], pack["mask_hidden"]
        d.o_attn, d.state_in, d.query_pos = o_attn.data_ptr(), state.data_ptr(), pack["qpos"].data_ptr()
        for name, tensor in w.items():
            setattr(d, name, tensor.data_ptr())
        d.ln_eps = 1e-5
        d.state_out, d.mask_embed_out, d.cls_out = outs[0].data_ptr(), outs[1].data_ptr(), cls_out.data_ptr()
        last = "next_q_wt" not in w
        d.next_q_out = None if last else outs[2].data_ptr()
        d.workspace = ws.data_ptr()
        _lib.check(lib.eprecon_decoder_query_side_async(ctypes.byref(d), _lib.current_stream()), "eprecon_decoder_query_side_async")
        h = self.num_heads
        q_next = None if last else outs[2].view(q_n, h, c // h).transpose(0, 1).unsqueeze(0)
        return outs[0], cls_out.unsqueeze(0), outs[1].unsqueeze(0), q_next

    def _forward_fused(self, pack, panoptic_features, panoptic_coords, mask_features, spitial_shape):
        """GPU inference, every step on csrc/decoder.hip + three GEMMs per layer: the mask logits (voxel-major: [N_2, Q]), the
        key / value projections, the masked attention as ONE split-K flash-attention pass over the level's voxels, and the
        query side (static shape) as two launches.  pred_masks of the auxiliary heads are [1, Q, N_2] VIEWS of the voxel-major
        logit matrices (same values and shape as the reference's, other strides); the final head's are contiguous.
        pack: _query_side_pack's (its tag reads every parameter: once per pass)"""
        c = self.query_feat.weight.shape[1]
        heads = self.num_heads
        n_q = self.num_queries
        dev = mask_features.device
        scale = 1.0 / math.sqrt(c // heads)
        outs = torch.empty((self.num_layers, 3, n_q, c), dtype=torch.float32, device=dev)
        cls_all = torch.empty((self.num_layers, n_q, pack["n_cls"]), dtype=torch.float32, device=dev)
        ws = torch.empty((4, n_q, c), dtype=torch.float32, device=dev)
        o_attn = torch.empty((1, heads, n_q, c // heads), dtype=torch.float32, device=dev)
        rows = lambda t: t[0].t()                                        # [1, C, N] view of voxel rows -> the rows [N, C]
        # per level: the projected keys / values of EVERY layer that attends to it in two products (columns [a C, (a + 1) C) =
        # the a-th of those layers): 6 launches for the 6 layers' 12 projections
        k_of, v_of = [None] * self.num_layers, [None] * self.num_layers
        for i in range(self.num_feature_levels):
            xyz = panoptic_coords[i][0]
            xyz = xyz if xyz.dtype == torch.int32 else xyz.to(torch.int32)
            f = rows(panoptic_features[i])
            f = f if f.stride(1) == 1 else f.contiguous()
            s_i, k_i = decoder_level_inputs(xyz, f, self.level_embed.weight[i], self.pos_enc.gauss_B, spitial_shape)
            kv = pack["kv_levels"][i]
            k_all = SP.sparse_conv(k_i, kv["wk"], None, kv["bk"])
            v_all = SP.sparse_conv(s_i, kv["wv"], None, kv["bv"])
            for a, j in enumerate(kv["layers"]):
                k_of[j], v_of[j] = k_all[:, a * c:(a + 1) * c], v_all[:, a * c:(a + 1) * c]
        fine = panoptic_coords[2].squeeze(0)
        mask_rows = [nearest_fine_index(panoptic_coords[0].squeeze(0), fine, 4, as_int32=True),
                     nearest_fine_index(panoptic_coords[1].squeeze(0), fine, 2, as_int32=True), None]
        mf = rows(mask_features)
        mf = mf if mf.is_contiguous() else mf.contiguous()
        classes, masks = [pack["cls0"].clone()], []
        me, q, state = pack["me0"], pack["q0"], pack["state0"]
        for j in range(self.num_layers):
            lvl = j % self.num_feature_levels
            logits_t = torch.mm(mf, me[0].t())                           # [N_2, Q]: this head's mask logits, voxel-major
            masks.append(logits_t.t().unsqueeze(0))
            masked_attention(q, k_of[j], v_of[j], logits_t, mask_rows[lvl], o_attn, scale)
            state, cls, me, q = self._query_side_hip(pack, j, o_attn, state, outs[j], cls_all[j], ws)
            classes.append(cls)
        # the final head's masks in the reference's own layout ([1, Q, N_2] contiguous): panoptic_post reduces over them
        # row-wise, which crawls on the transposed view (8 ms against 0.2 ms at 56k voxels)
        masks.append(torch.mm(me[0], mf.t()).unsqueeze(0))
        return {"pred_logits": classes[-1], "pred_masks": masks[-1],
                "aux_outputs": [{"pred_logits": a, "pred_masks": b} for a, b in zip(classes[:-1], masks[:-1])]}

    def forward(self, panoptic_features, panoptic_coords, mask_features, spitial_shape):
        """panoptic_features 3 x [1, C, N_l]; panoptic_coords 3 x [1, N_l, 3]; mask_features [1, C, N_2]"""
        if self.use_fused_voxel_side and mask_features.is_cuda and not torch.is_grad_enabled() and mask_features.shape[0] == 1:
            c = self.query_feat.weight.shape[1]
            ffn = self.transformer_ffn_layers[0].linear1.out_features
            if (c // self.num_heads == 6 and self.num_heads % 2 == 0 and self.num_heads <= 8 and c <= 64 and self.num_queries <= 128
                    and ffn <= 256 and self.mask_embed.layers[0].out_features <= 256):
                pack = self._query_side_pack(mask_features.device)
                if pack["ok"]:
                    return self._forward_fused(pack, panoptic_features, panoptic_coords, mask_features, spitial_shape)
        pos = self.get_pos_encs(panoptic_coords, spitial_shape)
        src, sizes = [], []
        for i in range(self.num_feature_levels):
            sizes.append(panoptic_coords[i].shape[1])
            src.append((panoptic_features[i] + self.level_embed.weight[i][None, :, None]).permute(2, 0, 1))
            pos[i] = pos[i].permute(2, 0, 1)
        fine = panoptic_coords[2].squeeze(0)
        # level 2 attends over the finest voxels themselves: identity (the reference indexes with an all-True mask)
        mask_indices = [nearest_fine_index(panoptic_coords[0].squeeze(0), fine, 4),
                        nearest_fine_index(panoptic_coords[1].squeeze(0), fine, 2), None]
        keys_in = [s_ + p_ for s_, p_ in zip(src, pos)]      # each level serves two layers
        query_embed = self.query_embed.weight.unsqueeze(1)
        classes, masks = [], []
        plan = self._static_plan(mask_features.device)
        if plan is not None:
            # ---- GPU inference: per layer only the voxel-count dependent work is issued eagerly (key / value
            # projections, the masked scaled-dot-product, the mask logits); the query side is one graph replay ----
            cls, me, q = plan["cls0"], plan["me0"], plan["q0"]
            msk, blocked = self._mask_and_block(me, mask_features, mask_indices[0])
            classes.append(cls.clone())
            masks.append(msk)
            for j in range(self.num_layers):
                lvl = j % self.num_feature_levels
                blocked = blocked & ~blocked.all(dim=-1, keepdim=True)        # :388 without the host round trip
                kv = self.transformer_cross_attention_layers[j].project_kv(keys_in[lvl], src[lvl])
                step = plan["layers"][j]
                step["o_in"].copy_(F.scaled_dot_product_attention(q, kv[0], kv[1], attn_mask=~blocked))
                step["graph"].replay()
                nxt = (j + 1) % self.num_feature_levels
                msk, blocked = self._mask_and_block(step["me"], mask_features, mask_indices[nxt])
                classes.append(step["cls"].clone())
                masks.append(msk)
                q = step["q_next"]
            return {"pred_logits": classes[-1], "pred_masks": masks[-1],
                    "aux_outputs": [{"pred_logits": a, "pred_masks": b} for a, b in zip(classes[:-1], masks[:-1])]}
        output = self.query_feat.weight.unsqueeze(1)
        cls, msk, blocked = self.forward_prediction_heads(output, mask_features, sizes[0], mask_indices[0])
        classes.append(cls)
        masks.append(msk)
        for j in range(self.num_layers):
            lvl = j % self.num_feature_levels
            # a query whose mask blocks every voxel attends to all of them (:388), without the host round trip
            # of the reference's torch.where
            blocked = blocked & ~blocked.all(dim=-1, keepdim=True)
            cross = self.transformer_cross_attention_layers[j]
            output = cross.attend(output, query_embed, cross.project_kv(keys_in[lvl], src[lvl]), blocked)
            output = self.transformer_self_attention_layers[j](output, query_pos=query_embed)
            output = self.transformer_ffn_layers[j](output)
            nxt = (j + 1) % self.num_feature_levels
            cls, msk, blocked = self.forward_prediction_heads(output, mask_features, sizes[nxt], mask_indices[nxt])
            classes.append(cls)
            masks.append(msk)
        return {"pred_logits": classes[-1], "pred_masks": masks[-1],
                "aux_outputs": [{"pred_logits": a, "pred_masks": b} for a, b in zip(classes[:-1], masks[:-1])]}


# ---------------------------------------------------------------------------------------------
# post-processing (models/mask3dformer.py:462-581)
# ---------------------------------------------------------------------------------------------
THING_IDS = tuple(range(3, 21))  # classes 1 (wall) and 2 (floor) are stuff


def panoptic_inference(mask_cls, mask_pred, object_mask_threshold=0.3, thing_id=THING_IDS, overlap_threshold=0.5):
    """mask_cls f32[Q, K+1], mask_pred f32[Q, N] (logits) -> [panoptic_seg int32[N], segments_info]"""
    scores, labels = F.softmax(mask_cls, dim=-1).max(-1)
    keep = labels.ne(0) & (scores > object_mask_threshold)
    q, n = mask_pred.shape
    dev = mask_pred.device
    seg = torch.zeros(n, dtype=torch.int32, device=dev)
    info = []
    hip = mask_pred.is_cuda and not torch.is_grad_enabled() and mask_pred.dtype == torch.float32 and mask_pred.stride(1) == 1 \
        and q <= 256
    if hip:
        # one pass over the [Q, N] logits (csrc/decoder.hip, panoptic_stats_kernel): owner of every voxel, its confidence, the
        # three per-query counts; ONE host read (counts + keep flags + classes); ids written by a second launch below
        lib = _lib.load()
        owner = torch.empty(n, dtype=torch.int32, device=dev)
        conf = torch.empty(n, dtype=torch.uint8, device=dev)
        meta = torch.empty((5, q), dtype=torch.int32, device=dev)
        meta[3], meta[4] = keep, labels
        sc = scores.contiguous()
        _lib.check(lib.eprecon_panoptic_stats_async(_lib.ptr(mask_pred), mask_pred.stride(0), _lib.ptr(sc), _lib.ptr(meta[3]), q, n,
                                                    _lib.ptr(owner), _lib.ptr(conf), _lib.ptr(meta), _lib.current_stream()),
                   "eprecon_panoptic_stats_async")
        _lib.count_host_read()
        host = meta.cpu()
    else:
        # The reference compacts the kept queries first (boolean indexing: a host read) and reads two more tensors back; here
        # the dropped queries stay in place with a score below every kept one, and the per-query counts, the keep flags and
        # the classes come back in ONE read.  Kept queries keep their relative order, so the ids come out the same.
        prob = mask_pred.sigmoid()
        weighted = torch.where(keep.view(-1, 1), scores.view(-1, 1) * prob, prob.new_full((), -1.0))
        owner = weighted.argmax(0)
        confident = (prob >= 0.5) & keep.view(-1, 1)
        onehot = (owner.unsqueeze(0) == torch.arange(q, device=owner.device).unsqueeze(1)) & keep.view(-1, 1)
        _lib.count_host_read()
        host = torch.stack([onehot.sum(1), confident.sum(1), (onehot & confident).sum(1), keep.long(), labels.long()]).cpu()
    stats, kept, classes = host[:3], host[3].tolist(), host[4].tolist()
    if not any(kept):
        return [seg, info]
    idmap = [0] * q
    seg_id, stuff_ids = 0, {}
    for k in range(q):
        if not kept[k]:
            continue
        mask_area, original_area, joint = (int(v) for v in stats[:, k])
        if mask_area > 0 and original_area > 0 and joint > 0:
            if mask_area / original_area < overlap_threshold:
                continue
            cls = int(classes[k])
            isthing = cls in thing_id
            region = None if hip else onehot[k] & confident[k]
            if not isthing:
                if cls in stuff_ids:
                    idmap[k] = stuff_ids[cls]
                    if not hip:
                        seg[region] = stuff_ids[cls]
                    continue
                stuff_ids[cls] = seg_id + 1
            seg_id += 1
            idmap[k] = seg_id
            if not hip:
                seg[region] = seg_id
            info.append({"id": seg_id, "isthing": bool(isthing), "category_id": cls})
    if hip and any(idmap):
        ids = torch.tensor(idmap, dtype=torch.int32).to(dev, non_blocking=True)
        _lib.check(_lib.load().eprecon_panoptic_assign_async(_lib.ptr(owner), _lib.ptr(conf), _lib.ptr(ids), n, _lib.ptr(seg),
                                                             _lib.current_stream()), "eprecon_panoptic_assign_async")
    return [seg, info]


def panoptic_post(outputs, semantic_on=False, panoptic_on=True, instance_on=False, occupied=None):
    assert panoptic_on and not semantic_on and not instance_on
    cls_all = outputs["pred_logits"]
    msk_all = outputs["pred_masks"] if occupied is None else outputs["pred_masks"][..., occupied]
    result = {}
    for mask_cls, mask_pred in zip(cls_all, msk_all):
        result["panoptic_seg"] = panoptic_inference(mask_cls, mask_pred)
    return result
