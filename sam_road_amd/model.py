"""`SAMRoad` — drop-in inference surface of the reference's LightningModule (reference
model.py:190-508) backed by the gfx950 HIP library (C ABI in include/samroad_hip.h).

Same constructor (`SAMRoad(config)`), same `state_dict` key names and shapes, same
three entry points with the same argument meaning:

    infer_masks_and_img_features(rgb)                       model.py:459-495
    infer_toponet(image_embeddings, graph_points, pairs, valid)   model.py:498-508
    forward(rgb, graph_points, pairs, valid)                model.py:414-457

The module tree below only HOLDS parameters (so `load_state_dict(strict=True)`, `.eval()`,
`.to(device)` behave as in the reference); no arithmetic runs in PyTorch.  There is no CPU path: a
call without the built library or without an MI355X raises.  Training (`training_step`, losses,
optimizers: model.py:349-363,511-685) is out of scope.
"""
import ctypes as C
import os
import warnings

import torch
from torch import nn

from . import _lib

ARCH = {  # model.py:197-218
    "vit_b": dict(embed_dim=768, depth=12, num_heads=12, global_attn_indexes=[2, 5, 8, 11]),
    "vit_l": dict(embed_dim=1024, depth=24, num_heads=16, global_attn_indexes=[5, 11, 17, 23]),
    "vit_h": dict(embed_dim=1280, depth=32, num_heads=16, global_attn_indexes=[7, 15, 23, 31]),
}


class _LayerNorm2dParams(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))


class _LoRAQkvParams(nn.Module):
    """Key layout of the reference's `_LoRA_qkv` (model.py:152-186): weight/bias keep their names and
    four rank-r adapters are added.  Folded into qkv.weight at pack time."""

    def __init__(self, dim, r):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(3 * dim, dim))
        self.bias = nn.Parameter(torch.zeros(3 * dim))
        self.linear_a_q = nn.Linear(dim, r, bias=False)
        self.linear_b_q = nn.Linear(r, dim, bias=False)
        self.linear_a_v = nn.Linear(dim, r, bias=False)
        self.linear_b_v = nn.Linear(r, dim, bias=False)
        nn.init.zeros_(self.linear_b_q.weight)
        nn.init.zeros_(self.linear_b_v.weight)


class _AttnParams(nn.Module):
    def __init__(self, dim, heads, grid, lora_rank):
        super().__init__()
        self.qkv = _LoRAQkvParams(dim, lora_rank) if lora_rank else nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        self.rel_pos_h = nn.Parameter(torch.zeros(2 * grid - 1, dim // heads))
        self.rel_pos_w = nn.Parameter(torch.zeros(2 * grid - 1, dim // heads))


class _MlpParams(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.lin1 = nn.Linear(dim, 4 * dim)
        self.lin2 = nn.Linear(4 * dim, dim)


class _BlockParams(nn.Module):
    def __init__(self, dim, heads, grid, lora_rank):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _AttnParams(dim, heads, grid, lora_rank)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _MlpParams(dim)


class _PatchEmbedParams(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=16, stride=16)


class _ImageEncoderParams(nn.Module):
    """Parameter layout of the fork's ImageEncoderViT as constructed at model.py:245-258."""

    def __init__(self, img_size, embed_dim, depth, num_heads, global_attn_indexes, lora_rank=0):
        super().__init__()
        self.img_size = img_size  # read at model.py:439
        grid = img_size // 16
        self.patch_embed = _PatchEmbedParams(embed_dim)
        self.pos_embed = nn.Parameter(torch.zeros(1, grid, grid, embed_dim))
        self.blocks = nn.ModuleList([
            _BlockParams(embed_dim, num_heads, grid if i in global_attn_indexes else 14, lora_rank)
            for i in range(depth)])
        self.neck = nn.Sequential(nn.Conv2d(embed_dim, 256, 1, bias=False), _LayerNorm2dParams(256),
                                  nn.Conv2d(256, 256, 3, padding=1, bias=False), _LayerNorm2dParams(256))


class _SamAttnParams(nn.Module):
    def __init__(self, dim, downsample):
        super().__init__()
        inner = dim // downsample
        self.q_proj, self.k_proj, self.v_proj = nn.Linear(dim, inner), nn.Linear(dim, inner), nn.Linear(dim, inner)
        self.out_proj = nn.Linear(inner, dim)


class _SamTwoWayBlockParams(nn.Module):
    def __init__(self):
        super().__init__()
        self.self_attn = _SamAttnParams(256, 1)
        self.norm1 = nn.LayerNorm(256)
        self.cross_attn_token_to_image = _SamAttnParams(256, 2)
        self.norm2 = nn.LayerNorm(256)
        self.mlp = nn.Module()
        self.mlp.lin1, self.mlp.lin2 = nn.Linear(256, 2048), nn.Linear(2048, 256)
        self.norm3 = nn.LayerNorm(256)
        self.norm4 = nn.LayerNorm(256)
        self.cross_attn_image_to_token = _SamAttnParams(256, 2)


class _SamMlpParams(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))


class _SamPromptEncoderParams(nn.Module):
    """Parameter layout of the fork's PromptEncoder as constructed at model.py:263-268 (embed 256, mask_in_chans 16).  Only
    no_mask_embed and the positional-encoding matrix are read by the no-prompt path the reference runs (model.py:427-429)."""

    def __init__(self):
        super().__init__()
        self.pe_layer = nn.Module()
        self.pe_layer.register_buffer("positional_encoding_gaussian_matrix", torch.randn((2, 128)))
        self.point_embeddings = nn.ModuleList([nn.Embedding(1, 256) for _ in range(4)])
        self.not_a_point_embed = nn.Embedding(1, 256)
        self.mask_downscaling = nn.Sequential(nn.Conv2d(1, 4, 2, stride=2), _LayerNorm2dParams(4), nn.GELU(),
                                              nn.Conv2d(4, 16, 2, stride=2), _LayerNorm2dParams(16), nn.GELU(),
                                              nn.Conv2d(16, 256, 1))
        self.no_mask_embed = nn.Embedding(1, 256)
        for p in self.parameters():
            p.requires_grad = False          # model.py:269-270


class _SamMaskDecoderParams(nn.Module):
    """Parameter layout of the fork's MaskDecoder + TwoWayTransformer as constructed at model.py:271-282."""

    def __init__(self):
        super().__init__()
        self.transformer = nn.Module()
        self.transformer.layers = nn.ModuleList([_SamTwoWayBlockParams() for _ in range(2)])
        self.transformer.final_attn_token_to_image = _SamAttnParams(256, 2)
        self.transformer.norm_final_attn = nn.LayerNorm(256)
        self.iou_token = nn.Embedding(1, 256)
        self.mask_tokens = nn.Embedding(3, 256)
        self.output_upscaling = nn.Sequential(nn.ConvTranspose2d(256, 64, 2, stride=2), _LayerNorm2dParams(64), nn.GELU(),
                                              nn.ConvTranspose2d(64, 32, 2, stride=2), nn.GELU())
        self.output_hypernetworks_mlps = nn.ModuleList([_SamMlpParams([256, 256, 256, 32]) for _ in range(3)])
        self.iou_prediction_head = _SamMlpParams([256, 256, 256, 3])


class _TopoNetParams(nn.Module):
    def __init__(self, version):
        super().__init__()
        self.feature_proj = nn.Linear(256, 128)
        self.pair_proj = nn.Linear(258, 128)
        if version != "no_transformer":
            layer = nn.TransformerEncoderLayer(d_model=128, nhead=4, dim_feedforward=128, dropout=0.1,
                                               activation="relu", batch_first=True)
            self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=3)
        self.output_proj = nn.Linear(128, 1)


class GraphRasterOps:
    """The road graph as a raster on the device (GRAPH_RASTER; the rule in sam_road_amd/graph_raster.py): the three entries
    srh_graph_raster / srh_graph_composite / srh_graph_compare on the device of `_graph_device()`, on torch's current stream.  They use
    the library context for its device and its error text only — no weights, no workspace — so they may run on a stream of their own."""

    def _graph_device(self):
        raise NotImplementedError

    def _graph_ctx(self):
        dev = self._graph_device()
        if dev.type != "cuda":
            raise _lib.SrhError("the graph rasteriser runs on an MI355X only (device %s); there is no CPU fallback" % dev)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        return _lib.Context.get(idx), torch.device("cuda", idx)

    @staticmethod
    def _graph_u8(name, t, shape, dev, optional=False):
        if t is None and optional:
            return None
        if not torch.is_tensor(t) or t.device != dev or t.dtype not in (torch.uint8, torch.bool) or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous uint8 tensor of shape {tuple(shape)} on {dev}, got "
                             f"{(t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t)}")
        return t

    @torch.no_grad()
    def graph_raster(self, shape, nodes, edges, width, mark="none", radius=0, values=(1, 2), out=None):
        """The class map of a graph over an image of shape (H, W) (srh_graph_raster): nodes int [N, 2] (row, col) and edges int [E, 2] on
        the HOST, checked by graph_raster.check_graph -> a NEW uint8 [H, W] tensor on the device (or `out`, a contiguous uint8 tensor of
        H W bytes there): values[1] on a node mark, else values[0] on an edge of `width`, else 0.  Three launches at most, no workspace of
        the library context, nothing read back."""
        from . import graph_raster as _gr
        ctx, dev = self._graph_ctx()
        H, W = int(shape[0]), int(shape[1])
        if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
            raise ValueError(f"the image must have at least 1 x 1 and at most 2^31 - 1 pixels, got {H} x {W}")
        n, e = _gr.check_graph(nodes, edges)
        _gr.check_style(width, mark, radius)
        if len(values) != 2 or not all(isinstance(v, int) and 1 <= v <= 255 for v in values):
            raise ValueError(f"values must be two ints 1 .. 255 (edge, node), got {values!r}")
        n_h, e_h = torch.from_numpy(n), torch.from_numpy(e)
        n_d, e_d = n_h.to(dev), e_h.to(dev)
        if out is None:
            out = torch.empty((H, W), dtype=torch.uint8, device=dev)
        elif out.device != dev or out.dtype != torch.uint8 or out.numel() != H * W or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of {H * W} pixels on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        N, E = int(n.shape[0]), int(e.shape[0])
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_graph_raster(ctx.handle, n_h.data_ptr() if N else None, n_d.data_ptr() if N else None, N,
                                               e_h.data_ptr() if E else None, e_d.data_ptr() if E else None, E, H, W, int(width),
                                               _lib.SRH_GRAPH_MARKS[mark], int(radius), values[0], values[1], out.data_ptr(),
                                               SAMRoad._stream(dev)), "srh_graph_raster")
        return out                                # the device tables were made on this stream and are read on it

    @torch.no_grad()
    def graph_composite(self, cls, img=None, edge_color=(253, 160, 15), node_color=(255, 255, 0), background=(0, 0, 0), out=None):
        """The scene with the classes in colour (srh_graph_composite): cls uint8 [H, W] and img uint8 [H, W, 3] (or None: the background
        colour) on the device -> a NEW uint8 [H, W, 3] tensor there (or `out`): node_color where cls >= 2, edge_color where cls == 1."""
        import numpy as np
        ctx, dev = self._graph_ctx()
        if not torch.is_tensor(cls) or cls.dim() != 2:
            raise ValueError("cls must be a uint8 [H, W] tensor")
        H, W = cls.shape
        cls = self._graph_u8("cls", cls, (H, W), dev)
        img = self._graph_u8("img", img, (H, W, 3), dev, optional=True)
        if img is not None and img.dtype != torch.uint8:
            raise ValueError("img must be uint8")
        cols = []
        for name, c in (("background", background), ("edge_color", edge_color), ("node_color", node_color)):
            if len(c) != 3 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v <= 255 for v in c):
                raise ValueError(f"{name} must be three ints 0 .. 255, got {c!r}")
            cols.append((C.c_int32 * 3)(*[int(v) for v in c]))
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if out is None else self._graph_u8("out", out, (H, W, 3), dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_graph_composite(ctx.handle, cls.data_ptr(), None if img is None else img.data_ptr(), H, W,
                                                  C.addressof(cols[0]), C.addressof(cols[1]), C.addressof(cols[2]), out.data_ptr(),
                                                  SAMRoad._stream(dev)), "srh_graph_composite")
        return out

    @torch.no_grad()
    def graph_compare(self, pred_thin, pred_wide, gt_thin, gt_wide, valid=None, img=None, diff=False):
        """Four class maps uint8 [H, W] on the device against each other (srh_graph_compare) -> (counts, diff image or None): counts an
        int64 [4] tensor ON THE DEVICE, {n_pred, n_fp, n_gt, n_missed} over the pixels with valid != 0 (valid uint8 / bool [H, W] or
        None); with diff=True the uint8 [H, W, 3] image, img (or black) with missed pixels red and false positives blue, from the same pass."""
        ctx, dev = self._graph_ctx()
        if not torch.is_tensor(pred_thin) or pred_thin.dim() != 2:
            raise ValueError("the class maps must be uint8 [H, W] tensors")
        H, W = pred_thin.shape
        maps = [self._graph_u8(n, t, (H, W), dev) for n, t in (("pred_thin", pred_thin), ("pred_wide", pred_wide), ("gt_thin", gt_thin), ("gt_wide", gt_wide))]
        valid = self._graph_u8("valid", valid, (H, W), dev, optional=True)
        img = self._graph_u8("img", img, (H, W, 3), dev, optional=True)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if diff else None
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_graph_compare(ctx.handle, *[m.data_ptr() for m in maps], None if valid is None else valid.data_ptr(),
                                                None if img is None else img.data_ptr(), H, W, counts.data_ptr(),
                                                None if out is None else out.data_ptr(), SAMRoad._stream(dev)), "srh_graph_compare")
        return counts, out

    @torch.no_grad()
    def graph_edge_stats(self, nodes, edges, mask, width=1, on_level=127, valid=None):
        """The mask under every edge (srh_graph_edge_stats; EDGE_SUPPORT, DESIGN.md §6p, the rule in sam_road_amd/edge_support.py): nodes
        int [N, 2] (row, col) and edges int [E, 2] on the HOST, checked by graph_raster.check_graph; mask uint8 [H, W] and valid uint8 /
        bool [H, W] or None, numpy arrays or tensors on the device -> a NEW int32 [E, 4] tensor on the device, rows {n, s, n_on,
        n_invalid} over the pixels GRAPH_RASTER's rule covers for the edge at `width`.  One launch (none for E = 0), no workspace of the
        library context, nothing read back."""
        import numpy as np
        from . import edge_support as _es
        from . import graph_raster as _gr
        ctx, dev = self._graph_ctx()
        t, level = _es.check_width(width), _es.check_on_level(on_level)
        n, e = _gr.check_graph(nodes, edges)
        if not torch.is_tensor(mask):
            mask = np.asarray(mask)
            if mask.dtype != np.uint8 or mask.ndim != 2:
                raise ValueError(f"mask must be uint8 [H, W], got {mask.dtype} {mask.shape}")
            mask = torch.from_numpy(np.ascontiguousarray(mask)).to(dev)
        if mask.dim() != 2 or mask.dtype != torch.uint8:
            raise ValueError(f"mask must be uint8 [H, W], got {mask.dtype} {tuple(mask.shape)}")
        H, W = mask.shape
        if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
            raise ValueError(f"the image must have at least 1 x 1 and at most 2^31 - 1 pixels, got {H} x {W}")
        mask = self._graph_u8("mask", mask, (H, W), dev)
        if valid is not None and not torch.is_tensor(valid):
            valid = np.asarray(valid)
            if valid.dtype not in (np.uint8, np.bool_) or valid.shape != (H, W):
                raise ValueError(f"valid must be uint8 / bool [{H}, {W}], got {valid.dtype} {valid.shape}")
            valid = torch.from_numpy(np.ascontiguousarray(valid)).to(dev)
        valid = self._graph_u8("valid", valid, (H, W), dev, optional=True)
        N, E = int(n.shape[0]), int(e.shape[0])
        out = torch.empty((E, 4), dtype=torch.int32, device=dev)
        if E == 0:
            return out
        n_h, e_h = torch.from_numpy(n), torch.from_numpy(e)
        n_d, e_d = n_h.to(dev), e_h.to(dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_graph_edge_stats(ctx.handle, n_h.data_ptr(), n_d.data_ptr(), N, e_h.data_ptr(), e_d.data_ptr(), E, H, W, t,
                                                   mask.data_ptr(), None if valid is None else valid.data_ptr(), level, out.data_ptr(),
                                                   SAMRoad._stream(dev)), "srh_graph_edge_stats")
        return out                                # the device tables were made on this stream and are read on it

    @torch.no_grad()
    def road_dist(self, mask, on_level=127, radius=32):
        """The capped squared distance map of a thresholded mask (srh_road_dist; ROAD_WIDTH, DESIGN.md §6q, the rule in
        sam_road_amd/road_width.py): mask uint8 [H, W], a numpy array or a tensor on the device -> a NEW uint16 [H, W] tensor on the
        device, 0 where mask <= on_level, else min(radius^2, the squared distance to the nearest such pixel of the image).  Two launches,
        H W bytes of the library context's workspace between them, nothing read back."""
        import numpy as np
        from . import edge_support as _es
        from . import road_width as _rw
        ctx, dev = self._graph_ctx()
        level, R = _es.check_on_level(on_level), _rw.check_radius(radius)
        if not torch.is_tensor(mask):
            mask = np.asarray(mask)
            if mask.dtype != np.uint8 or mask.ndim != 2:
                raise ValueError(f"mask must be uint8 [H, W], got {mask.dtype} {mask.shape}")
            mask = torch.from_numpy(np.ascontiguousarray(mask)).to(dev)
        if mask.dim() != 2 or mask.dtype != torch.uint8:
            raise ValueError(f"mask must be uint8 [H, W], got {mask.dtype} {tuple(mask.shape)}")
        H, W = mask.shape
        if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
            raise ValueError(f"the image must have at least 1 x 1 and at most 2^31 - 1 pixels, got {H} x {W}")
        mask = self._graph_u8("mask", mask, (H, W), dev)
        out = torch.empty((H, W), dtype=torch.uint16, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_road_dist(ctx.handle, mask.data_ptr(), H, W, level, R, out.data_ptr(), SAMRoad._stream(dev)), "srh_road_dist")
        return out

    @torch.no_grad()
    def graph_edge_widths(self, nodes, edges, d2, radius=32):
        """The width statistics of every edge (srh_graph_edge_widths; ROAD_WIDTH): nodes int [N, 2] (row, col) and edges
        int [E, 2] on the HOST, checked by graph_raster.check_graph; d2 the uint16 [H, W] tensor of road_dist at the same radius, on the
        device -> a NEW int32 [E, 8] tensor on the device, rows {n, n_in, s_q, n_cap, d2_min, d2_max, 0, 0} over the edge's centre line.
        One launch (none for E = 0), no workspace of the library context, nothing read back."""
        from . import graph_raster as _gr
        from . import road_width as _rw
        ctx, dev = self._graph_ctx()
        R = _rw.check_radius(radius)
        n, e = _gr.check_graph(nodes, edges)
        if not torch.is_tensor(d2) or d2.device != dev or d2.dtype != torch.uint16 or d2.dim() != 2 or not d2.is_contiguous():
            raise ValueError(f"d2 must be a contiguous uint16 [H, W] tensor on {dev}, got "
                             f"{(d2.dtype, tuple(d2.shape), d2.device) if torch.is_tensor(d2) else type(d2)}")
        H, W = d2.shape
        if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
            raise ValueError(f"the image must have at least 1 x 1 and at most 2^31 - 1 pixels, got {H} x {W}")
        N, E = int(n.shape[0]), int(e.shape[0])
        out = torch.empty((E, 8), dtype=torch.int32, device=dev)
        if E == 0:
            return out
        n_h, e_h = torch.from_numpy(n), torch.from_numpy(e)
        n_d, e_d = n_h.to(dev), e_h.to(dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_graph_edge_widths(ctx.handle, n_h.data_ptr(), n_d.data_ptr(), N, e_h.data_ptr(), e_d.data_ptr(), E, H, W,
                                                    d2.data_ptr(), R, out.data_ptr(), SAMRoad._stream(dev)), "srh_graph_edge_widths")
        return out                                # the device tables were made on this stream and are read on it

    @torch.no_grad()
    def graph_clean(self, nodes, edges, spur_q=0, comp_q=0, rounds=1, state=None, out=None):
        """Spur and small-component pruning with chain and component ids (srh_graph_clean; GRAPH_CLEAN, DESIGN.md §6s, the rule in
        sam_road_amd/graph_clean.py): nodes int [N, 2] (row, col) and edges int [E, 2] on the HOST, checked by graph_raster.check_graph;
        spur_q / comp_q the integer thresholds ceil(16 s) / ceil(16 c), 0 = not stated -> NEW tensors on the device (or `state` / `out`),
        state uint8 [E] and out int32 [E, 4], equal to graph_clean_ref.  5 (rounds + 1) launches (none for E = 0) over a workspace of the
        library context, nothing read back."""
        from . import graph_clean as _gc
        from . import graph_raster as _gr
        ctx, dev = self._graph_ctx()
        n, e = _gr.check_graph(nodes, edges)
        rounds = _gc.check_rounds(rounds)
        for name, q in (("spur_q", spur_q), ("comp_q", comp_q)):
            if not _gc._is_int(q) or not 0 <= q < 2 ** 63:
                raise ValueError(f"GRAPH_CLEAN: {name} must be an int >= 0, got {q!r}")
        N, E = int(n.shape[0]), int(e.shape[0])
        if N > _gc.MAX_ITEMS or E > _gc.MAX_ITEMS:
            raise ValueError(f"GRAPH_CLEAN: at most 2^26 nodes and edges, got {N}, {E}")
        if state is None:
            state = torch.empty(E, dtype=torch.uint8, device=dev)
        elif state.device != dev or state.dtype != torch.uint8 or state.numel() != E or not state.is_contiguous():
            raise ValueError(f"state must be a contiguous uint8 tensor of {E} elements on {dev}")
        if out is None:
            out = torch.empty((E, 4), dtype=torch.int32, device=dev)
        elif out.device != dev or out.dtype != torch.int32 or out.numel() != 4 * E or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int32 tensor of {4 * E} elements on {dev}")
        if E == 0:
            return state, out
        n_h, e_h = torch.from_numpy(n), torch.from_numpy(e)
        n_d, e_d = n_h.to(dev), e_h.to(dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_graph_clean(ctx.handle, n_h.data_ptr(), n_d.data_ptr(), N, e_h.data_ptr(), e_d.data_ptr(), E, int(spur_q), int(comp_q),
                                              rounds, state.data_ptr(), out.data_ptr(), SAMRoad._stream(dev)), "srh_graph_clean")
        return state, out                         # the device tables were made on this stream and are read on it


class DeviceGraphOps(GraphRasterOps):
    """GraphRasterOps without a model: the entries need a device, not weights."""

    def __init__(self, device):
        self.device = torch.device(device)

    def _graph_device(self):
        return self.device


class SAMRoad(nn.Module, GraphRasterOps):
    def __init__(self, config):
        super().__init__()
        self.config = config
        assert config.SAM_VERSION in {"vit_b", "vit_l", "vit_h"}  # model.py:197
        if config.NO_SAM:
            raise NotImplementedError("NO_SAM ablation is not part of the release (reference model.py:232-242)")
        arch = dict(ARCH[config.SAM_VERSION])
        if config.ENCODER_DEPTH:  # test hook, not a reference key (absent => falsy => ignored)
            arch["depth"] = int(config.ENCODER_DEPTH)
            arch["global_attn_indexes"] = [int(i) for i in (config.ENCODER_GLOBAL_ATTN_INDEXES or [])]
        self.arch = arch
        self.image_size = config.PATCH_SIZE
        self.register_buffer("pixel_mean", torch.Tensor([123.675, 116.28, 103.53]).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.Tensor([58.395, 57.12, 57.375]).view(-1, 1, 1), False)
        lora_rank = int(config.LORA_RANK) if config.ENCODER_LORA else 0
        self.image_encoder = _ImageEncoderParams(config.PATCH_SIZE, lora_rank=lora_rank, **arch)
        if config.USE_SAM_DECODER:  # model.py:260-282 (archived configs): SAM PromptEncoder (no prompts) + MaskDecoder
            self.prompt_encoder = _SamPromptEncoderParams()
            self.mask_decoder = _SamMaskDecoderParams()
        else:
            self.map_decoder = nn.Sequential(  # model.py:286-295 (indices 0,1,3,5,7 carry parameters)
                nn.ConvTranspose2d(256, 128, kernel_size=2, stride=2), _LayerNorm2dParams(128), nn.GELU(),
                nn.ConvTranspose2d(128, 64, kernel_size=2, stride=2), nn.GELU(),
                nn.ConvTranspose2d(64, 32, kernel_size=2, stride=2), nn.GELU(),
                nn.ConvTranspose2d(32, 2, kernel_size=2, stride=2))
        # a YAML without TOPONET_VERSION (toponet_vith_256 / vitl_256 / vitb_256 / vitb_1024) yields an empty Config here; the
        # reference then takes every `!=` / `==` string comparison's "normal" branch (model.py:84,111-116)
        v = config.TOPONET_VERSION
        self._topo_version = v if isinstance(v, str) else "normal"
        self.topo_net = _TopoNetParams(self._topo_version)
        self._packed = {}  # device index -> (Context, weights handle)
        self._packed_stamp = -1
        self._stamp_tensors = None
        self._imported = False                    # True: the packed weights came from another rank (import_packed)
        self._init_from_sam_checkpoint()

    # ---- init-time SAM checkpoint (model.py:365-411) ------------------------------------------------------
    def _init_from_sam_checkpoint(self):
        path = self.config.SAM_CKPT_PATH
        if not path or not os.path.exists(str(path)):
            warnings.warn(f"SAM checkpoint {path!r} not found: skipping the SAM initialisation that the "
                          "reference performs unconditionally (model.py:367); load a fine-tuned state_dict instead")
            return
        ckpt = torch.load(path, map_location="cpu")
        grid = self.image_size // 16
        if self.image_size != 1024 and ckpt["image_encoder.pos_embed"].shape[1] != grid:
            ckpt = dict(ckpt)
            pe = ckpt["image_encoder.pos_embed"].permute(0, 3, 1, 2)
            pe = nn.functional.interpolate(pe, (grid, grid), mode="bilinear", align_corners=False)
            ckpt["image_encoder.pos_embed"] = pe.permute(0, 2, 3, 1)
            # the reference selects "global" rel-pos keys by substring match on the block index
            # (model.py:403), which also catches e.g. block 17 for index 7 — reproduced as is.
            for k in [k for k in ckpt if "rel_pos" in k and any(str(i) in k for i in self.arch["global_attn_indexes"])]:
                t = ckpt[k][None, None]
                ckpt[k] = nn.functional.interpolate(t, (grid * 2 - 1, t.shape[-1]), mode="bilinear",
                                                    align_corners=False)[0, 0]
        own = dict(self.named_parameters())
        matched = {k: v for k, v in ckpt.items() if k in own and own[k].shape == v.shape}
        self.matched_param_names = set(matched)
        self.load_state_dict(matched, strict=False)

    # ---- packed weights life cycle ------------------------------------------------------------------------
    def _invalidate(self):
        for ctx, handle in self._packed.values():
            ctx.lib.srh_weights_free(handle)
        self._packed = {}
        self._stamp_tensors = None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._invalidate()
        self._imported = False
        return out

    def _apply(self, fn, *args, **kwargs):
        # a model that runs on an IMPORTED arena (share_packed_weights) keeps it across an _apply that moved nothing
        # (net.to(same_device), .cuda(), .float()): its Python parameters are not what it computes with, so dropping the
        # arena here would make the next call re-pack this rank's never-loaded parameters
        before = self._stamp() if self._imported else None
        out = super()._apply(fn, *args, **kwargs)
        if self._imported:
            self._stamp_tensors = None
            if self._stamp() == before:
                return out
        self._invalidate()
        return out

    def __del__(self):
        try:
            self._invalidate()
        except Exception:
            pass

    def _model_cfg(self):
        """The architecture record the library packs / lays out weights for (include/samroad_hip.h srh_model_cfg)."""
        cfg = _lib.ModelCfg()
        cfg.embed_dim, cfg.depth, cfg.num_heads = self.arch["embed_dim"], self.arch["depth"], self.arch["num_heads"]
        cfg.patch_size = int(self.config.PATCH_SIZE)
        gi = list(self.arch["global_attn_indexes"])
        cfg.n_global = len(gi)
        for i, g in enumerate(gi):
            cfg.global_attn_indexes[i] = g
        cfg.window_size = 14
        cfg.toponet_version = {"no_offset": 1, "no_transformer": 2}.get(self._topo_version, 0)
        cfg.use_sam_decoder = 1 if self.config.USE_SAM_DECODER else 0
        return cfg

    def _stamp(self):
        if self._stamp_tensors is None:           # the module-tree walk costs more than the stamp: cached until _apply / load_state_dict
            self._stamp_tensors = list(self.parameters()) + list(self.buffers())
        return hash(tuple((t._version, t.data_ptr()) for t in self._stamp_tensors))

    # ---- multi-GPU: the PACKED weights travel, not the state_dict (north_star: "RCCL broadcast of weights over xGMI") -------
    def export_packed(self, device):
        """The packed weight arena of this model on `device` (fp16 MFMA operands, f32 biases / LayerNorm / pos-embed, packed
        TopoNet fragments — what srh_weights_pack built) as a uint8 tensor on that device."""
        ctx, wh = self._weights(torch.device(device))
        n = C.c_size_t(0)
        ctx.check(ctx.lib.srh_weights_export(ctx.handle, wh, None, 0, C.byref(n)), "srh_weights_export")
        buf = torch.empty(n.value, dtype=torch.uint8, device=device)
        ctx.check(ctx.lib.srh_weights_export(ctx.handle, wh, buf.data_ptr(), n.value, C.byref(n)), "srh_weights_export")
        return buf

    def import_packed(self, buf):
        """Adopt packed weights produced by export_packed of a model with the SAME configuration (on another rank).  From here on
        this model's Python parameters are NOT what it computes with; editing them raises instead of silently re-packing."""
        dev = buf.device
        if dev.type != "cuda" or buf.dtype != torch.uint8:
            raise _lib.SrhError("import_packed expects a uint8 tensor on an MI355X")
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        ctx = _lib.Context.get(idx)
        self._invalidate()
        cfg = self._model_cfg()
        handle = C.c_void_p()
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_weights_import(ctx.handle, C.byref(cfg), buf.data_ptr(), buf.numel(), C.byref(handle)),
                      "srh_weights_import")
        self._packed[idx] = (ctx, handle)
        self._packed_stamp = self._stamp()
        self._imported = True

    def share_packed_weights(self, src=0):
        """torch.distributed (backend nccl = RCCL over xGMI): rank `src` packs its checkpoint once and broadcasts the packed
        arena device-to-device (one large collective: ~175 MB for ViT-B instead of 360 MB of f32 state_dict plus a host re-pack
        on every rank); the other ranks never read the checkpoint.  No-op without an initialised process group."""
        from . import distributed as D
        if not D.is_distributed():
            return
        dev = next(self.parameters()).device
        rank = torch.distributed.get_rank()
        buf = self.export_packed(dev) if rank == src else None
        buf = D.broadcast_bytes(buf, src=src, device=dev)
        if rank != src:
            self.import_packed(buf)

    def _weights(self, device):
        if device.type != "cuda":
            raise _lib.SrhError("SAMRoad runs on an MI355X only (tensor is on %s); there is no CPU fallback" % device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        # in-place parameter edits (p.data.copy_, an optimizer step, a manual LoRA merge, load_state_dict on a submodule) bump
        # the tensors' version counters: the packed fp16 copy is rebuilt instead of silently serving stale weights
        # (buffers too — the prompt encoder's Gaussian matrix is baked into the packed SAM-decoder weights — and each tensor's
        # storage address, so that `p.data = new_tensor` rebinding is seen as well)
        stamp = self._stamp()
        if stamp != self._packed_stamp:
            if self._imported:
                raise _lib.SrhError("this model computes with packed weights imported from another rank (share_packed_weights); "
                                    "its parameters were edited or moved afterwards — re-share the weights instead")
            self._invalidate()
            self._packed_stamp = stamp
        hit = self._packed.get(idx)
        if hit is not None:
            return hit
        if self._imported:      # whatever dropped the arena (or another device index asked for it): never re-pack local parameters
            raise _lib.SrhError("this model computes with packed weights imported from another rank (share_packed_weights) and has "
                                "none for cuda:%d — re-share the weights instead of re-packing this rank's parameters" % idx)
        ctx = _lib.Context.get(idx)
        sd = {k: v.detach().to(torch.float32).cpu().contiguous() for k, v in self.state_dict().items()}
        # fold LoRA adapters into the fused qkv weight (q rows [0:D], v rows [2D:3D]; model.py:179-185)
        for k in [k for k in sd if k.endswith("attn.qkv.linear_a_q.weight")]:
            base = k[: -len("linear_a_q.weight")]
            w = sd[base + "weight"].clone()
            d = w.shape[1]
            w[:d] += sd[base + "linear_b_q.weight"] @ sd[base + "linear_a_q.weight"]
            w[2 * d:] += sd[base + "linear_b_v.weight"] @ sd[base + "linear_a_v.weight"]
            sd[base + "weight"] = w
        cfg = self._model_cfg()
        names = [k for k in sd if ".linear_" not in k]
        arr = (_lib.NamedTensor * len(names))()
        keep = []
        for i, k in enumerate(names):
            t = sd[k]
            keep.append(k.encode())
            arr[i].name = keep[-1]
            arr[i].data = t.data_ptr()
            arr[i].on_device = 0
            arr[i].ndim = t.dim()
            for j, s in enumerate(t.shape):
                arr[i].shape[j] = s
        handle = C.c_void_p()
        ctx.check(ctx.lib.srh_weights_pack(ctx.handle, C.byref(cfg), arr, len(names), C.byref(handle)),
                  "srh_weights_pack")
        self._packed[idx] = (ctx, handle)
        return self._packed[idx]

    def _graph_device(self):                      # GraphRasterOps: the renders run where the model is
        return next(self.parameters()).device

    # ---- entry points -------------------------------------------------------------------------------------------
    @staticmethod
    def _stream(device):
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def _encode(self, rgb, want_logits, want_scores):
        if rgb.dim() != 4 or rgb.shape[-1] != 3 or rgb.shape[1] != self.image_size or rgb.shape[2] != self.image_size:
            raise ValueError(f"rgb must be [B,{self.image_size},{self.image_size},3], got {tuple(rgb.shape)}")
        ctx, wh = self._weights(rgb.device)
        if rgb.dtype == torch.uint8:
            dt = _lib.SRH_U8
        else:
            rgb = rgb.to(torch.float32)
            dt = _lib.SRH_F32
        rgb = rgb.contiguous()
        B, P = rgb.shape[0], self.image_size
        h = P // 16
        emb = torch.empty((B, h, h, 256), dtype=torch.float32, device=rgb.device)
        logits = torch.empty((B, P, P, 2), dtype=torch.float32, device=rgb.device) if want_logits else None
        scores = torch.empty((B, P, P, 2), dtype=torch.float32, device=rgb.device) if want_scores else None
        with torch.cuda.device(rgb.device):
            ctx.check(ctx.lib.srh_encode_decode(
                ctx.handle, wh, rgb.data_ptr(), dt, B,
                logits.data_ptr() if want_logits else None, scores.data_ptr() if want_scores else None,
                emb.data_ptr(), self._stream(rgb.device)), "srh_encode_decode")
        # reference shape [B,256,h,w]; memory stays channels-last (a permuted view, no copy)
        return logits, scores, emb.permute(0, 3, 1, 2)

    def _topo(self, image_embeddings, graph_points, pairs, valid, want_logits):
        dev = image_embeddings.device
        ctx, wh = self._weights(dev)
        emb = image_embeddings.permute(0, 2, 3, 1)
        if emb.dtype != torch.float32 or not emb.is_contiguous():
            emb = emb.to(torch.float32).contiguous()
        B, Ns, K = pairs.shape[0], pairs.shape[1], pairs.shape[2]
        N = graph_points.shape[1]
        if graph_points.dtype == torch.int64:
            pts, pdt = graph_points.contiguous(), _lib.SRH_I64
        else:
            pts, pdt = graph_points.to(torch.float32).contiguous(), _lib.SRH_F32
        if pairs.dtype == torch.int64:
            prs, qdt = pairs.contiguous(), _lib.SRH_I64
        else:
            prs, qdt = pairs.to(torch.int32).contiguous(), _lib.SRH_I32
        vld = valid.to(torch.uint8).contiguous()
        scores = torch.empty((B, Ns, K, 1), dtype=torch.float32, device=dev)
        logits = torch.empty((B, Ns, K, 1), dtype=torch.float32, device=dev) if want_logits else None
        if B * Ns * K > 0:
            with torch.cuda.device(dev):
                ctx.check(ctx.lib.srh_toponet(
                    ctx.handle, wh, emb.data_ptr(), pts.data_ptr(), pdt, prs.data_ptr(), qdt, vld.data_ptr(),
                    B, N, Ns, K, logits.data_ptr() if want_logits else None, scores.data_ptr(),
                    self._stream(dev)), "srh_toponet")
        return logits, scores

    @torch.no_grad()
    def forward(self, rgb, graph_points, pairs, valid):
        mask_logits, mask_scores, emb = self._encode(rgb, True, True)
        topo_logits, topo_scores = self._topo(emb, graph_points, pairs, valid, True)
        return mask_logits, mask_scores, topo_logits, topo_scores

    @torch.no_grad()
    def infer_masks_and_img_features(self, rgb):
        _, mask_scores, emb = self._encode(rgb, False, True)
        return mask_scores, emb

    @torch.no_grad()
    def infer_toponet(self, image_embeddings, graph_points, pairs, valid):
        """model.py:498-508: pairs [B,N,K,2], valid [B,N,K] for any K = MAX_NEIGHBOR_QUERIES from 1 to 64 (ABI 10) -> scores [B,N,K,1]."""
        return self._topo(image_embeddings, graph_points, pairs, valid, False)[1]

    @torch.no_grad()
    def infer_toponet_ragged(self, image_embeddings, points, point_tile, pairs, valid, tile_offsets=None):
        """infer_toponet over the UNPADDED query rows of many tiles at once (pass 2 of infer_one_img, reference inferencer.py:179-207,
        which pads every batch to its longest tile): image_embeddings [n,256,h,w] (the NCHW view of the library's channels-last
        buffer), points f32 [R,2] tile-local (x, y), point_tile i32 [R] (index into image_embeddings), pairs i32 [R,K,2] (rows of
        the flat list), valid u8 [R,K]  ->  scores f32 [R,K] (srh_toponet_ragged; rows as built by srh_pass2_pack_ragged).
        tile_offsets (host int64 [n + 1], rows of tile t = offsets[t] .. offsets[t+1], from 0 to R): the library then scores the scene in
        chunks of whole tiles (<= 16 k x 16 pairs = rows x K each, same bits) so that its workspace does not grow with the scene; without
        them at most 65 536 x 16 pairs per call.  K (MAX_NEIGHBOR_QUERIES) may be 1 to 64 (ABI 10).  Both rows of every pair must be rows of the same tile (ABI 9): a pair that is not makes check_finite()
        (or the next infer_* / scene_pass1 call) raise SrhError instead of the scores silently depending on the chunking."""
        dev = image_embeddings.device
        ctx, wh = self._weights(dev)
        emb = image_embeddings.permute(0, 2, 3, 1)
        if emb.dtype != torch.float32 or not emb.is_contiguous():
            emb = emb.to(torch.float32).contiguous()
        R, K = int(pairs.shape[0]), int(pairs.shape[1])
        pts = points.to(device=dev, dtype=torch.float32).contiguous()
        pt = point_tile.to(device=dev, dtype=torch.int32).contiguous()
        prs = pairs.to(device=dev, dtype=torch.int32).contiguous()
        vld = valid.to(device=dev, dtype=torch.uint8).contiguous()
        scores = torch.empty((R, K), dtype=torch.float32, device=dev)
        off = None
        if tile_offsets is not None:
            import numpy as np
            off = np.ascontiguousarray(tile_offsets, dtype=np.int64)
            if off.shape != (emb.shape[0] + 1,):
                raise ValueError(f"tile_offsets must have {emb.shape[0] + 1} entries (one per tile of image_embeddings + 1), got {off.shape}")
        if R * K > 0:
            with torch.cuda.device(dev):
                ctx.check(ctx.lib.srh_toponet_ragged(ctx.handle, wh, emb.data_ptr(), int(emb.shape[0]), pts.data_ptr(), pt.data_ptr(),
                                                     prs.data_ptr(), vld.data_ptr(), R, K, off.ctypes.data if off is not None else None,
                                                     scores.data_ptr(), self._stream(dev)), "srh_toponet_ragged")
        return scores

    def set_lanes(self, mode, device=None):
        """How this device's context runs the encoder of a batch (srh_ctx_set_lanes): 0 auto, 1 one lane, 2 two half-batch lanes on two
        streams whenever the batch is even.  Same outputs bit for bit.  last_lanes() tells what the last call ran."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        _lib.Context.get(dev.index if dev.index is not None else torch.cuda.current_device()).set_lanes(mode)

    def last_lanes(self, device=None):
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        return _lib.Context.get(dev.index if dev.index is not None else torch.cuda.current_device()).last_lanes()

    def check_finite(self, device=None, synchronize=True):
        """Raise SrhError if a LayerNorm pass of any earlier call on this device's context saw an Inf / NaN (an fp16 overflow in the
        encoder: srh_ctx_check, SRH_ERR_NONFINITE) — the masks / embeddings of that call are invalid.  synchronize=True waits for the
        current stream first; False only looks at what has already completed (the scene loop polls right after a scene's masks reached
        the host).  The same condition is raised lazily by the next infer_* / scene_pass1 call.  The reference's own guards
        (inferencer.py:206,219) only see TopoNet's scores.  An infer_toponet_ragged pair outside its own tile is reported here too."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        ctx = _lib.Context.get(idx)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_ctx_check(ctx.handle, self._stream(dev), 1 if synchronize else 0), "srh_ctx_check")

    # ---- scene level (pass 1 of infer_one_img: tile batcher + model + mask fusion) -------------------------
    @torch.no_grad()
    def scene_pass1(self, scene_u8, tile_xy, batch_size, canvas_kp=None, canvas_road=None, window=None, tta=None):
        """scene_u8 [H,W,3] uint8 on the GPU (H and W independent, each >= PATCH_SIZE), tile_xy int32 [n,2] (x0,y0) on the
        GPU, every tile inside the scene.  Runs the tiles in batches through the encoder + decoder and accumulates the two
        mask canvases [H,W] in the reference's sequential order (inferencer.py:87-104).  Returns (canvas_kp, canvas_road,
        embeddings[n,256,h,w]).  window (f32 [PATCH_SIZE] on the GPU, inferencer.fuse_window): every tile's scores enter the canvases
        weighted by window[lx] * window[ly] (srh_scene_pass1_window_hw); None: the call and the kernels of a scene
        without a window.  tta (orientation codes 0..7, the first one 0 = id, inferencer.tta_plan): the whole tile list is run once per
        orientation and the canvases hold the sum over (orientation, tile) — to be normalised with the tile list repeated len(tta)
        times; the embeddings are those of id (srh_scene_pass1_tta_hw, with or without window); None: the calls of a
        scene without TTA."""
        dev = scene_u8.device
        ctx, wh = self._weights(dev)
        assert scene_u8.dtype == torch.uint8 and scene_u8.dim() == 3 and scene_u8.shape[2] == 3
        scene_u8 = scene_u8.contiguous()
        tile_xy = tile_xy.to(device=dev, dtype=torch.int32).contiguous()
        H, W = int(scene_u8.shape[0]), int(scene_u8.shape[1])
        n, h = tile_xy.shape[0], self.image_size // 16
        if H < self.image_size or W < self.image_size:
            raise ValueError(f"scene {H} x {W} is smaller than a {self.image_size}-px tile")
        if canvas_kp is None:
            canvas_kp = torch.zeros((H, W), dtype=torch.float32, device=dev)
            canvas_road = torch.zeros((H, W), dtype=torch.float32, device=dev)
        elif tuple(canvas_kp.shape) != (H, W) or tuple(canvas_road.shape) != (H, W):
            raise ValueError(f"canvases must be [{H}, {W}] like the scene, got {tuple(canvas_kp.shape)} / {tuple(canvas_road.shape)}")
        emb = torch.empty((n, h, h, 256), dtype=torch.float32, device=dev)
        if n == 0:                                   # a rank without tiles (world_size > tile count): nothing to add
            return canvas_kp, canvas_road, emb.permute(0, 3, 1, 2)
        codes = self._tta_codes(tta) if tta is not None else None
        if window is not None:
            window = self._window_f32(window, dev)
        if codes is not None:
            entry, extra = "srh_scene_pass1_tta_hw", (codes, len(codes), window.data_ptr() if window is not None else None)
        elif window is not None:
            entry, extra = "srh_scene_pass1_window_hw", (window.data_ptr(),)
        else:
            entry, extra = "srh_scene_pass1_hw", ()
        with torch.cuda.device(dev):
            ctx.check(getattr(ctx.lib, entry)(ctx.handle, wh, scene_u8.data_ptr(), H, W, tile_xy.data_ptr(), n, int(batch_size), *extra,
                                              canvas_kp.data_ptr(), canvas_road.data_ptr(), emb.data_ptr(), self._stream(dev)), entry)
        return canvas_kp, canvas_road, emb.permute(0, 3, 1, 2)

    @torch.no_grad()
    def scene_normalise(self, canvas_kp, canvas_road, tile_xy, valid=None, window=None):
        """(canvas / coverage count) * 255 -> uint8 masks [H,W] (inferencer.py:106-110); tile_xy = ALL tiles.  valid (u8 [H,W] on the
        GPU, non-zero = valid pixel): the masks are also 0 on every invalid pixel (srh_scene_normalise_valid_hw); None: the call and
        the kernels of a scene without a mask.  window (f32 [PATCH_SIZE] on the GPU, the one pass 1 ran with): the divisor is the
        sum of the tiles' weights instead of their count (srh_scene_normalise_window_hw, with or without valid); None: the calls above."""
        dev = canvas_kp.device
        ctx, _ = self._weights(dev)
        H, W = int(canvas_kp.shape[0]), int(canvas_kp.shape[1])
        tile_xy = tile_xy.to(device=dev, dtype=torch.int32).contiguous()
        kp = torch.empty((H, W), dtype=torch.uint8, device=dev)
        road = torch.empty((H, W), dtype=torch.uint8, device=dev)
        if window is not None:
            window = self._window_f32(window, dev)
        if valid is not None:
            valid = self._valid_u8(valid, H, W, dev)
        if window is not None:
            entry, extra = "srh_scene_normalise_window_hw", (window.data_ptr(), valid.data_ptr() if valid is not None else None)
        elif valid is not None:
            entry, extra = "srh_scene_normalise_valid_hw", (valid.data_ptr(),)
        else:
            entry, extra = "srh_scene_normalise_hw", ()
        with torch.cuda.device(dev):
            ctx.check(getattr(ctx.lib, entry)(ctx.handle, canvas_kp.data_ptr(), canvas_road.data_ptr(), H, W, tile_xy.data_ptr(),
                                              tile_xy.shape[0], self.image_size, *extra, kp.data_ptr(), road.data_ptr(),
                                              self._stream(dev)), entry)
        return kp, road

    @staticmethod
    def _tta_codes(tta):
        """Orientation codes as the host byte array srh_scene_pass1_tta_hw reads (the library checks the rules of DESIGN.md §6f)."""
        import ctypes
        codes = [int(c) for c in tta]
        if not codes or any(not 0 <= c <= 255 for c in codes):
            raise ValueError(f"tta must be a non-empty sequence of orientation codes 0..7, got {list(tta)!r}")
        return (ctypes.c_uint8 * len(codes))(*codes)

    @torch.no_grad()
    def op_patch_im2col(self, scene_u8, tile_xy, orient=0, patch_size=None):
        """Test-only (srh_op_patch_im2col): the f16 GEMM A matrix [n (P/16)^2, 768] of pass 1's crop + normalise + im2col for the tiles
        tile_xy int32 [n,2] (x0,y0) of a u8 [H,W,3] scene on the GPU, in orientation code `orient` (0: the launch of a scene without TTA)."""
        dev = scene_u8.device
        ctx, _ = self._weights(dev)
        P = int(patch_size or self.image_size)
        if scene_u8.dtype != torch.uint8 or scene_u8.dim() != 3 or scene_u8.shape[2] != 3 or not scene_u8.is_contiguous():
            raise ValueError("scene must be a contiguous uint8 [H,W,3] tensor")
        tile_xy = tile_xy.to(device=dev, dtype=torch.int32).contiguous()
        n, H, W = int(tile_xy.shape[0]), int(scene_u8.shape[0]), int(scene_u8.shape[1])
        if n and (int(tile_xy.min()) < 0 or int(tile_xy[:, 0].max()) + P > W or int(tile_xy[:, 1].max()) + P > H):
            raise ValueError("a tile lies outside the scene")
        out = torch.empty((n * (P // 16) ** 2, 768), dtype=torch.float16, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_op_patch_im2col(ctx.handle, scene_u8.data_ptr(), H, W, tile_xy.data_ptr(), n, P, int(orient),
                                                  out.data_ptr(), self._stream(dev)), "srh_op_patch_im2col")
        return out

    @torch.no_grad()
    def op_scores_unorient(self, scores, orient):
        """Test-only (srh_op_scores_unorient): scores f32 [n,P,P,2] of tiles oriented by code `orient` -> the scene frame, as a new tensor
        (a permutation of bit patterns)."""
        dev = scores.device
        ctx, _ = self._weights(dev)
        if scores.dtype != torch.float32 or scores.dim() != 4 or scores.shape[1] != scores.shape[2] or scores.shape[3] != 2 or not scores.is_contiguous():
            raise ValueError("scores must be a contiguous float32 [n,P,P,2] tensor")
        out = torch.empty_like(scores)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_op_scores_unorient(ctx.handle, scores.data_ptr(), int(scores.shape[0]), int(scores.shape[1]), int(orient),
                                                     out.data_ptr(), self._stream(dev)), "srh_op_scores_unorient")
        return out

    def _window_f32(self, window, dev):
        if window.device != dev or window.dtype != torch.float32 or tuple(window.shape) != (self.image_size,):
            raise ValueError(f"window must be a float32 [{self.image_size}] tensor on {dev}, got {window.dtype} {tuple(window.shape)} on {window.device}")
        return window.contiguous()

    @torch.no_grad()
    def op_scene_fuse_window(self, scores, tile_xy, window, canvas_kp, canvas_road):
        """Test-only (srh_op_scene_fuse_window): the weighted add of pass 1 on given scores f32 [n,P,P,2], IN PLACE on the f32 [H,W]
        canvases; tile_xy int32 [n,2] (x0,y0), every tile inside the scene."""
        dev = canvas_kp.device
        ctx, _ = self._weights(dev)
        P, n = self.image_size, int(tile_xy.shape[0])
        H, W = int(canvas_kp.shape[0]), int(canvas_kp.shape[1])
        window = self._window_f32(window, dev)
        tile_xy = tile_xy.to(device=dev, dtype=torch.int32).contiguous()
        ok = lambda t, shape: t.device == dev and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()
        if not (ok(scores, (n, P, P, 2)) and ok(canvas_kp, (H, W)) and ok(canvas_road, (H, W))):
            raise ValueError(f"scores must be contiguous float32 [{n},{P},{P},2] and the canvases contiguous float32 [{H},{W}] on {dev}")
        if n:
            with torch.cuda.device(dev):
                ctx.check(ctx.lib.srh_op_scene_fuse_window(ctx.handle, scores.data_ptr(), n, P, tile_xy.data_ptr(), window.data_ptr(),
                                                           canvas_kp.data_ptr(), canvas_road.data_ptr(), H, W, self._stream(dev)),
                          "srh_op_scene_fuse_window")
        return canvas_kp, canvas_road

    # ---- scene level, validity mask (nodata): which tiles hold data, nodata neutralised before the crop ------------------------
    @staticmethod
    def _valid_u8(valid, H, W, dev):
        if valid.device != dev or valid.dtype not in (torch.uint8, torch.bool) or tuple(valid.shape) != (H, W):
            raise ValueError(f"valid must be a uint8 / bool [{H}, {W}] tensor on {dev}, got {valid.dtype} {tuple(valid.shape)} on {valid.device}")
        valid = valid.contiguous()
        return valid.view(torch.uint8) if valid.dtype == torch.bool else valid

    @torch.no_grad()
    def scene_tile_valid(self, valid_u8, tile_xy):
        """Valid pixels per tile: valid_u8 [H,W] uint8 / bool on the GPU (non-zero = valid), tile_xy int32 [n,2] (x0,y0), every tile
        inside the scene -> int32 [n] on the GPU (srh_scene_tile_valid: exact integer counts).  The call uses no workspace of the
        library context, so it may run on a side stream beside a scene's pass 1."""
        dev = valid_u8.device
        ctx, _ = self._weights(dev)
        H, W = int(valid_u8.shape[0]), int(valid_u8.shape[1])
        valid_u8 = self._valid_u8(valid_u8, H, W, dev)
        tile_xy = tile_xy.to(device=dev, dtype=torch.int32).contiguous()
        counts = torch.empty((tile_xy.shape[0],), dtype=torch.int32, device=dev)
        if tile_xy.shape[0] == 0:                    # nothing to count (an empty tensor has no address to hand over)
            return counts
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_tile_valid(ctx.handle, valid_u8.data_ptr(), H, W, tile_xy.data_ptr(), tile_xy.shape[0],
                                                   self.image_size, counts.data_ptr(), self._stream(dev)), "srh_scene_tile_valid")
        return counts

    @torch.no_grad()
    def scene_fill_invalid(self, scene_u8, valid_u8, fill):
        """scene_u8 [H,W,3] uint8 on the GPU, IN PLACE: every pixel whose valid_u8 [H,W] is 0 becomes the colour `fill` (three ints
        0..255).  Returns scene_u8 (srh_scene_fill_invalid)."""
        dev = scene_u8.device
        ctx, _ = self._weights(dev)
        if scene_u8.dtype != torch.uint8 or scene_u8.dim() != 3 or scene_u8.shape[2] != 3 or not scene_u8.is_contiguous():
            raise ValueError(f"scene must be a contiguous uint8 [H,W,3] tensor, got {scene_u8.dtype} {tuple(scene_u8.shape)}")
        H, W = int(scene_u8.shape[0]), int(scene_u8.shape[1])
        valid_u8 = self._valid_u8(valid_u8, H, W, dev)
        r, g, b = (int(v) for v in fill)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_fill_invalid(ctx.handle, scene_u8.data_ptr(), valid_u8.data_ptr(), H, W, r, g, b,
                                                     self._stream(dev)), "srh_scene_fill_invalid")
        return scene_u8

    # ---- scene level, border padding (SCENE_PAD) --------------------------------------------------------------------
    @torch.no_grad()
    def scene_pad(self, t_u8, pads, mode="reflect", fill=(0, 0, 0)):
        """t_u8 [H,W,3] (a scene) or [H,W] (a validity mask; bool allowed) uint8 on the GPU -> a NEW tensor [H + top + bottom, W + left +
        right(, 3)] of the same dtype: pads = (top, bottom, left, right) >= 0, mode 'reflect' (numpy's pad mode of that name, any pad
        width), 'edge' or 'constant' (the colour `fill`, three ints 0..255; a mask takes the first).  The source is not written
        (srh_scene_pad); it may be any contiguous view, at any byte address."""
        import ctypes
        dev = t_u8.device
        ctx, _ = self._weights(dev)
        if t_u8.dtype not in (torch.uint8, torch.bool) or t_u8.dim() not in (2, 3) or (t_u8.dim() == 3 and t_u8.shape[2] != 3) or not t_u8.is_contiguous():
            raise ValueError(f"scene_pad takes a contiguous uint8 [H,W,3] or uint8 / bool [H,W] tensor, got {t_u8.dtype} {tuple(t_u8.shape)}")
        if mode not in _lib.SRH_PAD_MODES:
            raise ValueError(f"mode must be one of {tuple(_lib.SRH_PAD_MODES)}, got {mode!r}")
        top, bottom, left, right = (int(v) for v in pads)
        rgb = (ctypes.c_int32 * 3)(*(int(v) for v in fill))
        H, W, ch = int(t_u8.shape[0]), int(t_u8.shape[1]), 3 if t_u8.dim() == 3 else 1
        if min(top, bottom, left, right) < 0 or H < 1 or W < 1:
            raise ValueError(f"pads must be >= 0 and the tensor not empty, got pads {tuple(pads)} for {tuple(t_u8.shape)}")
        out = torch.empty((H + top + bottom, W + left + right) + tuple(t_u8.shape[2:]), dtype=t_u8.dtype, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_pad(ctx.handle, t_u8.data_ptr(), H, W, ch, top, bottom, left, right, _lib.SRH_PAD_MODES[mode], rgb,
                                            out.data_ptr(), self._stream(dev)), "srh_scene_pad")
        return out

    # ---- scene level, GeoTIFF scenes (GEOTIFF) ---------------------------------------------------------------------------
    @torch.no_grad()
    def tiff_assemble(self, scene, flat, table, table_dev=None):
        """The decompressed segments of a GeoTIFF -> its raster on the GPU (srh_tiff_assemble; the rule in sam_road_amd/geotiff.py): scene
        a geotiff.TiffScene, flat the uint8 tensor of scene.segments() ON THE GPU (16-byte aligned), table its int64 [n, 7] table on the
        HOST (a numpy array; checked again by the entry; table_dev: the same on the GPU where the caller has uploaded it) -> a NEW tensor [H, W, C] of the file's sample type, equal to
        tiff_read_ref bit for bit.  One launch, no workspace of the library context, nothing read back."""
        import numpy as np
        dev = flat.device
        ctx, _ = self._weights(dev)
        dtypes = {"uint8": (torch.uint8, _lib.SRH_U8), "uint16": (torch.uint16, _lib.SRH_U16), "float32": (torch.float32, _lib.SRH_F32)}
        if flat.dtype != torch.uint8 or flat.dim() != 1 or not flat.is_contiguous() or flat.numel() < 1:
            raise ValueError(f"flat must be a contiguous uint8 [n] tensor, got {flat.dtype} {tuple(flat.shape)}")
        if str(scene.dtype) not in dtypes:
            raise ValueError(f"a GeoTIFF scene is uint8, uint16 or float32, got {scene.dtype}")
        table = np.ascontiguousarray(table)
        if table.dtype != np.int64 or table.ndim != 2 or table.shape[1] != 7 or table.shape[0] < 1:
            raise ValueError(f"table must be int64 [n, 7], got {table.dtype} {table.shape}")
        t_h = torch.from_numpy(table)
        t_d = t_h.to(dev) if table_dev is None else table_dev
        H, W, Cb = (int(v) for v in scene.shape)
        t_dtype, code = dtypes[str(scene.dtype)]
        out = torch.empty((H, W, Cb), dtype=t_dtype, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_tiff_assemble(ctx.handle, flat.data_ptr(), flat.numel(), t_h.data_ptr(), t_d.data_ptr(), int(table.shape[0]),
                                                out.data_ptr(), H, W, Cb, code, int(scene.predictor), 0 if scene.little else 1, self._stream(dev)),
                      "srh_tiff_assemble")
        return out                                # the device table was made on this stream and is read on it

    # ---- scene level, 16-bit and multi-band scenes (SCENE_BANDS) ---------------------------------------------------------
    @staticmethod
    def _bands_src(src, select):
        """(dtype code, levels, pixels, C, select as a host int32[3]) of a raw scene [..., C] (uint8 / uint16, contiguous, 1 <= C <= 16)."""
        import ctypes
        codes = {torch.uint8: (_lib.SRH_U8, 256), torch.uint16: (_lib.SRH_U16, 65536)}
        if src.dtype not in codes or src.dim() < 2 or not src.is_contiguous() or not 1 <= src.shape[-1] <= 16 or src.numel() < 1:
            raise ValueError(f"a raw scene is a contiguous uint8 / uint16 [..., C] tensor with 1 <= C <= 16, got {src.dtype} {tuple(src.shape)}")
        C = int(src.shape[-1])
        select = [int(b) for b in select]
        if len(select) != 3 or not all(0 <= b < C for b in select):
            raise ValueError(f"select must be three band indices in 0..{C - 1}, got {select!r}")
        n = src.numel() // C
        if n > 2 ** 31 - 1:
            raise ValueError(f"a raw scene has at most 2^31 - 1 pixels, got {n}")
        return (*codes[src.dtype], n, C, (ctypes.c_int32 * 3)(*select))

    @torch.no_grad()
    def scene_bands_hist(self, src, select, valid=None):
        """The exact histogram of the three selected bands (srh_scene_bands_hist): src uint8 / uint16 [..., C] on the GPU (any element-
        aligned address), select three band indices, valid uint8 / bool with one entry per pixel (non-zero = counted) or None -> uint32
        [3, levels] on the GPU, levels 256 / 65536 by dtype.  The call uses no workspace of the library context."""
        dev = src.device
        ctx, _ = self._weights(dev)
        code, levels, n, C, sel = self._bands_src(src, select)
        if valid is not None:
            if valid.device != dev or valid.dtype not in (torch.uint8, torch.bool) or valid.numel() != n or not valid.is_contiguous():
                raise ValueError(f"valid must be a contiguous uint8 / bool tensor of {n} pixels on {dev}, got {valid.dtype} {tuple(valid.shape)} on {valid.device}")
        hist = torch.empty((3, levels), dtype=torch.uint32, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_bands_hist(ctx.handle, src.data_ptr(), code, n, C, sel, None if valid is None else valid.data_ptr(),
                                                   hist.data_ptr(), self._stream(dev)), "srh_scene_bands_hist")
        return hist

    @torch.no_grad()
    def scene_bands_apply(self, src, select, lut):
        """src uint8 / uint16 [..., C] on the GPU -> a NEW uint8 tensor [..., 3]: channel b = lut[b][src[..., select[b]]], lut uint8
        [3, levels] on the GPU (srh_scene_bands_apply).  The source is not written; it may be any contiguous view."""
        dev = src.device
        ctx, _ = self._weights(dev)
        code, levels, n, C, sel = self._bands_src(src, select)
        if lut.device != dev or lut.dtype != torch.uint8 or tuple(lut.shape) != (3, levels) or not lut.is_contiguous():
            raise ValueError(f"lut must be a contiguous uint8 [3, {levels}] tensor on {dev}, got {lut.dtype} {tuple(lut.shape)} on {lut.device}")
        out = torch.empty(tuple(src.shape[:-1]) + (3,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_bands_apply(ctx.handle, src.data_ptr(), code, n, C, sel, lut.data_ptr(), out.data_ptr(),
                                                    self._stream(dev)), "srh_scene_bands_apply")
        return out

    # ---- scene level, float32 scenes (SCENE_FLOAT) ---------------------------------------------------------------------------
    @staticmethod
    def _float_src(src, select, dev):
        """(pixels, C, select as a host int32[3]) of a raw float32 scene [..., C] (contiguous, 1 <= C <= 16)."""
        import ctypes
        if src.dtype != torch.float32 or src.dim() < 2 or not src.is_contiguous() or not 1 <= src.shape[-1] <= 16 or src.numel() < 1:
            raise ValueError(f"a raw float scene is a contiguous float32 [..., C] tensor with 1 <= C <= 16, got {src.dtype} {tuple(src.shape)}")
        C = int(src.shape[-1])
        select = [int(b) for b in select]
        if len(select) != 3 or not all(0 <= b < C for b in select):
            raise ValueError(f"select must be three band indices in 0..{C - 1}, got {select!r}")
        n = src.numel() // C
        if n > 2 ** 31 - 1:
            raise ValueError(f"a raw scene has at most 2^31 - 1 pixels, got {n}")
        return n, C, (ctypes.c_int32 * 3)(*select)

    @staticmethod
    def _float_mask(valid, n, dev, what="valid"):
        if valid.device != dev or valid.dtype not in (torch.uint8, torch.bool) or valid.numel() != n or not valid.is_contiguous():
            raise ValueError(f"{what} must be a contiguous uint8 / bool tensor of {n} pixels on {dev}, got {valid.dtype} {tuple(valid.shape)} on {valid.device}")
        return valid

    @torch.no_grad()
    def scene_float_valid(self, src, select, nodata_keys=(), log=False, valid=None):
        """The validity mask of a float32 scene by rule 1 of float_scene.py (srh_scene_float_valid): src float32 [..., C] on the GPU,
        select three band indices, nodata_keys up to 4 ordered keys (float_scene.nodata_keys), log: every selected band must be > 0,
        valid: the caller's mask, uint8 / bool with one entry per pixel, or None -> a NEW uint8 tensor src.shape[:-1] of 0 / 1."""
        import ctypes
        dev = src.device
        ctx, _ = self._weights(dev)
        n, C, sel = self._float_src(src, select, dev)
        keys = [int(k) for k in nodata_keys]
        if len(keys) > 4 or not all(0 <= k <= 0xffffffff for k in keys):
            raise ValueError(f"nodata_keys are up to 4 uint32 keys, got {nodata_keys!r}")
        if valid is not None:
            self._float_mask(valid, n, dev)
        out = torch.empty(tuple(src.shape[:-1]), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_float_valid(ctx.handle, src.data_ptr(), n, C, sel, (ctypes.c_uint32 * len(keys))(*keys) if keys else None, len(keys),
                                                    1 if log else 0, None if valid is None else valid.data_ptr(), out.data_ptr(), self._stream(dev)),
                      "srh_scene_float_valid")
        return out

    @torch.no_grad()
    def scene_float_hist(self, src, select, valid, targets=None):
        """Exact counts of the ordered keys of a float32 scene over the pixels where valid is non-zero (srh_scene_float_hist).  targets
        None: pass 1, uint32 [3, 65536] over key >> 16 of the three selected bands.  targets, 1 to 6 (band, prefix) pairs: pass 2, uint32
        [len(targets), 65536] over key & 0xffff of the values of `band` whose key >> 16 is `prefix`.  The call uses no workspace."""
        import ctypes
        dev = src.device
        ctx, _ = self._weights(dev)
        n, C, sel = self._float_src(src, select, dev)
        self._float_mask(valid, n, dev)
        tg = None
        if targets is not None:
            flat = [int(v) for t in targets for v in t]
            if not 1 <= len(targets) <= 6 or len(flat) != 2 * len(targets) or not all(0 <= b < C and 0 <= pre <= 0xffff for b, pre in zip(flat[::2], flat[1::2])):
                raise ValueError(f"targets are 1 to 6 (band in 0..{C - 1}, prefix in 0..65535) pairs, got {targets!r}")
            tg = (ctypes.c_uint32 * len(flat))(*flat)
        hist = torch.empty((3 if tg is None else len(targets), 65536), dtype=torch.uint32, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_float_hist(ctx.handle, src.data_ptr(), n, C, sel, valid.data_ptr(), tg, 0 if tg is None else len(targets),
                                                   hist.data_ptr(), self._stream(dev)), "srh_scene_float_hist")
        return hist

    @torch.no_grad()
    def scene_float_apply(self, src, select, valid, thresholds):
        """src float32 [..., C] on the GPU -> a NEW uint8 tensor [..., 3]: channel b of a pixel with a non-zero valid byte = the number of
        thresholds[b][:255] <= the ordered key of src[..., select[b]], of any other pixel 0 (srh_scene_float_apply).  thresholds: uint32
        [3, 256] on the GPU (float_scene.threshold_keys).  The source is not written; it may be any contiguous 4-byte-aligned view."""
        dev = src.device
        ctx, _ = self._weights(dev)
        n, C, sel = self._float_src(src, select, dev)
        self._float_mask(valid, n, dev)
        if thresholds.device != dev or thresholds.dtype != torch.uint32 or tuple(thresholds.shape) != (3, 256) or not thresholds.is_contiguous():
            raise ValueError(f"thresholds must be a contiguous uint32 [3, 256] tensor on {dev}, got {thresholds.dtype} {tuple(thresholds.shape)} on {thresholds.device}")
        out = torch.empty(tuple(src.shape[:-1]) + (3,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_float_apply(ctx.handle, src.data_ptr(), n, C, sel, valid.data_ptr(), thresholds.data_ptr(), out.data_ptr(),
                                                    self._stream(dev)), "srh_scene_float_apply")
        return out

    # ---- scene level, another ground resolution (SCENE_SCALE) -----------------------------------------------------------
    @staticmethod
    def _resample_tables(ctx, dev, n_in, n_out, p, q):
        """One axis' tables on the device, (start int32 [n_out], weights uint8 [n_out, T], T, D): built by resample.axis_tables and
        cached on the library context by (n_in, n_out, p, q)."""
        from . import resample
        cache = ctx.resample_tables
        key = (n_in, n_out, p, q)
        if key not in cache:
            if len(cache) >= 64:                       # a stream of scenes of ever new sizes: start over
                cache.clear()
            s, w, T, D = resample.axis_tables(n_in, p, q, n_out)
            cache[key] = (torch.from_numpy(s).to(dev), torch.from_numpy(w).to(dev), T, D)
        return cache[key]

    @torch.no_grad()
    def scene_resample(self, t, p, q, out_shape=None, valid_rule=False, zero_where=None, direct=False):
        """t [H,W,3] (a scene) or [H,W] (a mask; bool allowed) uint8 on the GPU -> a NEW tensor [Ho, Wo(, 3)] of the same dtype, resampled
        by the fraction p/q (two ints >= 1, p != q) exactly as resample.resample_ref does (srh_scene_resample): area averaging for p < q,
        bilinear at pixel centres for p > q, one rounding.  out_shape: (Ho, Wo), default (ceil(H p / q), ceil(W p / q)).  valid_rule: t is
        a validity mask and an output pixel is 1 iff every tap with a non-zero weight is non-zero.  zero_where: uint8 / bool [Ho, Wo] on
        the GPU; the result is 0 where it is 0.  direct: every output gathers its own taps instead of the separable form through LDS (the
        same bytes; for measurements).  The source is not written; it may be any contiguous view, at any byte address."""
        from . import resample
        dev = t.device
        ctx, _ = self._weights(dev)
        if t.dtype not in (torch.uint8, torch.bool) or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3) or not t.is_contiguous():
            raise ValueError(f"scene_resample takes a contiguous uint8 [H,W,3] or uint8 / bool [H,W] tensor, got {t.dtype} {tuple(t.shape)}")
        for v in (p, q):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"p and q must be ints >= 1, got {p!r} and {q!r}")
        H, W, ch = int(t.shape[0]), int(t.shape[1]), 3 if t.dim() == 3 else 1
        Ho, Wo = (resample.out_size(H, p, q), resample.out_size(W, p, q)) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
        if p == q or H < 1 or W < 1 or Ho < 1 or Wo < 1 or H * W > 2 ** 31 - 1 or Ho * Wo > 2 ** 31 - 1:
            raise ValueError(f"scene_resample: p != q and 1 to 2^31 - 1 pixels on both sides, got {p}/{q} for {tuple(t.shape)} -> {(Ho, Wo)}")
        if zero_where is not None:
            zero_where = self._valid_u8(zero_where, Ho, Wo, dev)
        sy, wy, Ty, Dy = self._resample_tables(ctx, dev, H, Ho, p, q)
        sx, wx, Tx, Dx = self._resample_tables(ctx, dev, W, Wo, p, q)
        bh, bw, win_h, win_w = resample.block_plan(Ty, Tx, p, q, ch)
        if direct or valid_rule:
            win_h = win_w = 0
        out = torch.empty((Ho, Wo) + tuple(t.shape[2:]), dtype=t.dtype, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_resample(ctx.handle, t.data_ptr(), H, W, ch, out.data_ptr(), Ho, Wo, sy.data_ptr(), wy.data_ptr(), Ty, Dy,
                                                 sx.data_ptr(), wx.data_ptr(), Tx, Dx, 1 if valid_rule else 0,
                                                 None if zero_where is None else zero_where.data_ptr(), bh, bw, win_h, win_w, self._stream(dev)),
                      "srh_scene_resample")
        return out

    # ---- scene level, groups of small scenes (SCENE_GROUP) -------------------------------------------------------------
    @staticmethod
    def _group_table(table, table_dev, dev):
        """(table on the host as a contiguous int64 [n,8] CPU tensor, the same on the device): the library validates the host copy and
        the kernel reads the device copy (include/samroad_hip.h); without table_dev the table is uploaded here."""
        t = torch.as_tensor(table)
        if t.device.type != "cpu" or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 8 or t.shape[0] < 1:
            raise ValueError(f"a scene-group table is an int64 [n, 8] array on the host with n >= 1, got {t.dtype} {tuple(t.shape)} on {t.device}")
        t = t.contiguous()
        if table_dev is None:
            table_dev = t.to(dev)
        if table_dev.device != dev or table_dev.dtype != torch.int64 or tuple(table_dev.shape) != tuple(t.shape) or not table_dev.is_contiguous():
            raise ValueError(f"table_dev must be the table as a contiguous int64 {tuple(t.shape)} tensor on {dev}")
        return t, table_dev

    @torch.no_grad()
    def scene_group_pack(self, ragged_u8, table, C, Ha, Wa, mode="reflect", fill=(0, 0, 0), table_dev=None):
        """The stack of a group's scenes (srh_scene_group_pack): ragged_u8, a flat uint8 / bool tensor on the GPU that holds the real scenes
        back to back (any byte address), table int64 [n,8] on the HOST with one row {byte offset in ragged_u8, H, W, top, left, H', W', row0}
        per scene -> a NEW tensor [Ha, Wa, 3] (C = 3) or [Ha, Wa] (C = 1) of ragged_u8's dtype: rows row0 .. row0 + H' hold the scene padded
        as scene_pad pads it, with its own pads, in columns 0 .. W', and 0 beyond.  table_dev: the table on the GPU if the caller has
        uploaded it already."""
        import ctypes
        dev = ragged_u8.device
        ctx, _ = self._weights(dev)
        if ragged_u8.dtype not in (torch.uint8, torch.bool) or ragged_u8.dim() != 1 or not ragged_u8.is_contiguous() or ragged_u8.numel() < 1:
            raise ValueError(f"scene_group_pack takes a flat contiguous uint8 / bool tensor, got {ragged_u8.dtype} {tuple(ragged_u8.shape)}")
        if mode not in _lib.SRH_PAD_MODES:
            raise ValueError(f"mode must be one of {tuple(_lib.SRH_PAD_MODES)}, got {mode!r}")
        if C not in (1, 3):
            raise ValueError(f"C must be 1 or 3, got {C!r}")
        t, t_dev = self._group_table(table, table_dev, dev)
        Ha, Wa = int(Ha), int(Wa)
        if Ha < 1 or Wa < 1 or Ha * Wa > 2 ** 31 - 1:
            raise ValueError(f"a stack has 1 to 2^31 - 1 pixels, got {Ha} x {Wa}")
        rgb = (ctypes.c_int32 * 3)(*(int(v) for v in fill))
        out = torch.empty((Ha, Wa, 3) if C == 3 else (Ha, Wa), dtype=ragged_u8.dtype, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_group_pack(ctx.handle, ragged_u8.data_ptr(), ragged_u8.numel(), t.data_ptr(), t_dev.data_ptr(), int(t.shape[0]),
                                                   int(C), Ha, Wa, _lib.SRH_PAD_MODES[mode], rgb, out.data_ptr(), self._stream(dev)),
                      "srh_scene_group_pack")
        return out

    @torch.no_grad()
    def scene_group_crop(self, kp_u8, road_u8, table, table_dev=None):
        """Every scene's window of the stack's two uint8 [Ha,Wa] masks, in ONE allocation (srh_scene_group_crop): table int64 [n,8] on the
        HOST as for scene_group_pack, column 0 being the byte offset of the scene's H x W block in each output (0, H0 W0, H0 W0 + H1 W1, ...).
        Returns a uint8 [2, sum H W] tensor: row 0 the keypoint masks, row 1 the road masks, the scenes back to back."""
        dev = kp_u8.device
        ctx, _ = self._weights(dev)
        for m in (kp_u8, road_u8):
            if m.device != dev or m.dtype != torch.uint8 or m.dim() != 2 or tuple(m.shape) != tuple(kp_u8.shape) or not m.is_contiguous():
                raise ValueError(f"scene_group_crop takes two contiguous uint8 [Ha,Wa] masks on one GPU, got {m.dtype} {tuple(m.shape)} on {m.device}")
        t, t_dev = self._group_table(table, table_dev, dev)
        total = int((t[:, 1] * t[:, 2]).sum())
        if total < 1:
            raise ValueError("scene_group_crop: the table describes no pixel")
        out = torch.empty((2, total), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_group_crop(ctx.handle, kp_u8.data_ptr(), road_u8.data_ptr(), int(kp_u8.shape[0]), int(kp_u8.shape[1]),
                                                   t.data_ptr(), t_dev.data_ptr(), int(t.shape[0]), out[0].data_ptr(), out[1].data_ptr(), total,
                                                   self._stream(dev)), "srh_scene_group_crop")
        return out

    # ---- scene level, small mask components dropped (MASK_CLEAN) ---------------------------------------------------------
    @torch.no_grad()
    def mask_clean(self, buf_u8, table, table_dev=None, connectivity=8):
        """The connected-component filter of mask_clean.mask_clean_ref, IN PLACE, on every image that `table` describes inside buf_u8, a
        flat contiguous uint8 tensor on the GPU (srh_mask_clean): table int64 [n,8] on the HOST (mask_clean.mask_clean_table), one row
        {byte offset in buf_u8, H, W, t_on, min_area, t_peak, BASE, SEG0} per image.  Nothing connects two images.  table_dev: the table on
        the GPU if the caller has uploaded it already.  The workspaces — an int32 parent / label per pixel plus an area and a peak per
        label — are allocated here for the call; the five launches are queued on the current stream and nothing is read back.  Returns
        buf_u8."""
        dev = buf_u8.device
        ctx, _ = self._weights(dev)
        if buf_u8.dtype != torch.uint8 or buf_u8.dim() != 1 or not buf_u8.is_contiguous() or buf_u8.numel() < 1:
            raise ValueError(f"mask_clean takes a flat contiguous uint8 tensor, got {buf_u8.dtype} {tuple(buf_u8.shape)}")
        if connectivity not in (4, 8):
            raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
        t, t_dev = self._group_table(table, table_dev, dev)
        total = int((t[:, 1] * t[:, 2]).sum())
        if total < 1 or total > 2 ** 31 - 1:
            raise ValueError(f"mask_clean: the table describes {total} pixels; 1 to 2^31 - 1 are supported")
        ws = torch.empty((3, total), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_mask_clean(ctx.handle, buf_u8.data_ptr(), buf_u8.numel(), t.data_ptr(), t_dev.data_ptr(), int(t.shape[0]),
                                             int(connectivity), ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr(), total, self._stream(dev)),
                      "srh_mask_clean")
        return buf_u8

    def mask_clean_pair(self, kp_u8, road_u8, plan):
        """mask_clean for the two [H,W] masks of one scene under a mask_clean.MaskCleanPlan, in place: one call when both are rows of one
        contiguous [2,H,W] tensor, else one call per mask; a mask whose rule drops nothing is left out.  Returns (kp_u8, road_u8)."""
        from . import mask_clean as mc
        for m in (kp_u8, road_u8):
            if m.dtype != torch.uint8 or m.dim() != 2 or not m.is_contiguous() or tuple(m.shape) != tuple(kp_u8.shape):
                raise ValueError(f"mask_clean_pair takes two contiguous uint8 [H,W] masks of one shape, got {m.dtype} {tuple(m.shape)}")
        H, W = int(kp_u8.shape[0]), int(kp_u8.shape[1])
        live = [(m, rule) for m, rule in ((kp_u8, plan.keypoint), (road_u8, plan.road)) if not mc.idle(rule)]
        if len(live) == 2 and road_u8.data_ptr() == kp_u8.data_ptr() + H * W and kp_u8.untyped_storage().data_ptr() == road_u8.untyped_storage().data_ptr():
            both = torch.as_strided(kp_u8, (2 * H * W,), (1,))
            self.mask_clean(both, mc.mask_clean_table([(0, H, W, plan.keypoint), (H * W, H, W, plan.road)]), connectivity=plan.connectivity)
        else:
            for m, rule in live:
                self.mask_clean(m.view(-1), mc.mask_clean_table([(0, H, W, rule)]), connectivity=plan.connectivity)
        return kp_u8, road_u8

    # ---- scene level, the validity mask from a nodata value (SCENE_NODATA) ------------------------------------------------
    @staticmethod
    def _nodata_and(and_with, n, dev):
        if and_with is None:
            return None
        if and_with.device != dev or and_with.dtype not in (torch.uint8, torch.bool) or and_with.numel() != n or not and_with.is_contiguous():
            raise ValueError(f"and_with must be a contiguous uint8 / bool tensor of {n} pixels on {dev}, got {and_with.dtype} {tuple(and_with.shape)} on {and_with.device}")
        return and_with

    @torch.no_grad()
    def scene_nodata_match(self, src, lo, hi, match="all", and_with=None, invert=False, out=None):
        """Which pixels of a raw scene hold the nodata value (srh_scene_nodata_match): src uint8 / uint16 [..., C] on the GPU (any element-
        aligned address, 1 <= C <= 16), lo / hi C ints each, the inclusive range of every band; match 'all' (every band inside its range)
        or 'any' -> a NEW uint8 tensor [...] of 0 / 1 (or `out`, a flat contiguous uint8 view of one byte per pixel): (not hit if invert
        else hit) & (and_with != 0), and_with a uint8 / bool tensor of one entry per pixel or None.  One launch, no workspace of the
        library context; the source is not written."""
        import ctypes
        dev = src.device
        ctx, _ = self._weights(dev)
        codes = {torch.uint8: _lib.SRH_U8, torch.uint16: _lib.SRH_U16}
        if src.dtype not in codes or src.dim() < 2 or not src.is_contiguous() or not 1 <= src.shape[-1] <= 16 or src.numel() < 1:
            raise ValueError(f"a raw scene is a contiguous uint8 / uint16 [..., C] tensor with 1 <= C <= 16, got {src.dtype} {tuple(src.shape)}")
        C = int(src.shape[-1])
        n = src.numel() // C
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if len(lo) != C or len(hi) != C or not all(0 <= v <= 65535 for v in lo + hi):
            raise ValueError(f"lo and hi must hold {C} ints in 0..65535 each, got {lo!r}, {hi!r}")
        if match not in _lib.SRH_NODATA_MATCH:
            raise ValueError(f"match must be one of {tuple(_lib.SRH_NODATA_MATCH)}, got {match!r}")
        if n > 2 ** 31 - 1:
            raise ValueError(f"a raw scene has at most 2^31 - 1 pixels, got {n}")
        and_with = self._nodata_and(and_with, n, dev)
        if out is None:
            out = torch.empty(tuple(src.shape[:-1]), dtype=torch.uint8, device=dev)
        elif out.device != dev or out.dtype != torch.uint8 or out.numel() != n or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of {n} pixels on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_nodata_match(ctx.handle, src.data_ptr(), codes[src.dtype], n, C, (ctypes.c_int32 * C)(*lo), (ctypes.c_int32 * C)(*hi),
                                                     _lib.SRH_NODATA_MATCH[match], None if and_with is None else and_with.data_ptr(), 1 if invert else 0,
                                                     out.data_ptr(), self._stream(dev)), "srh_scene_nodata_match")
        return out

    @torch.no_grad()
    def scene_nodata_grow(self, src_u8, table, r, and_with=None, invert=False, table_dev=None, out=None):
        """The Chebyshev dilation by r (1..16) of every image that `table` describes inside src_u8, a flat contiguous uint8 tensor on the GPU
        (srh_scene_nodata_grow): table int64 [n,8] on the HOST, one row {byte offset, H, W, ...} per image — columns 3..7 are not read, a
        mask_clean table serves as it is.  Returns a NEW flat uint8 tensor of src_u8's size (or `out`, which must not overlap src_u8) whose
        blocks hold (not g if invert else g) & (and_with != 0), g = 1 iff a pixel of the image within distance r is non-zero; and_with is
        laid out like src_u8, or None.  Bytes outside the blocks are not written.  table_dev: the table on the GPU if the caller has uploaded
        it already.  One launch, no workspace of the library context."""
        dev = src_u8.device
        ctx, _ = self._weights(dev)
        if src_u8.dtype != torch.uint8 or src_u8.dim() != 1 or not src_u8.is_contiguous() or src_u8.numel() < 1:
            raise ValueError(f"scene_nodata_grow takes a flat contiguous uint8 tensor, got {src_u8.dtype} {tuple(src_u8.shape)}")
        r = int(r)
        if not 1 <= r <= 16:
            raise ValueError(f"r must be 1 to 16, got {r!r}")
        t, t_dev = self._group_table(table, table_dev, dev)
        n = src_u8.numel()
        and_with = self._nodata_and(and_with, n, dev)
        if out is None:
            out = torch.empty((n,), dtype=torch.uint8, device=dev)
        elif out.device != dev or out.dtype != torch.uint8 or out.numel() != n or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of {n} bytes on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_nodata_grow(ctx.handle, src_u8.data_ptr(), out.data_ptr(), n, t.data_ptr(), t_dev.data_ptr(), int(t.shape[0]), r,
                                                    None if and_with is None else and_with.data_ptr(), 1 if invert else 0, self._stream(dev)),
                      "srh_scene_nodata_grow")
        return out

    # ---- scene level, the validity mask from the polygons of an area of interest (SCENE_AOI) -------------------------------
    @torch.no_grad()
    def scene_aoi_fill(self, shape, edges, polys, n_include, n_exclude, and_with=None, invert=False, table_dev=None, out=None):
        """The even-odd fill of include / exclude polygons over a scene of shape (H, W) (srh_scene_aoi_fill): edges int32 [E, 4] and polys
        int32 [n_include + n_exclude + 1] on the HOST, the tables of aoi.aoi_edges -> a NEW uint8 [H, W] tensor of 0 / 1 on the model's
        device (or `out`, a contiguous uint8 tensor of H W bytes there): (not aoi if invert else aoi) & (and_with != 0), and_with a uint8 /
        bool tensor of one entry per pixel or None.  table_dev: aoi.aoi_pack(edges, polys) on the GPU (a flat int32 tensor at a 16-byte
        aligned address) if the caller has uploaded it already.  One launch, no workspace of the library context, nothing read back."""
        import numpy as np
        from . import aoi as _aoi
        dev = next(self.parameters()).device
        ctx, _ = self._weights(dev)
        H, W = int(shape[0]), int(shape[1])
        if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
            raise ValueError(f"a scene has at least 1 x 1 and at most 2^31 - 1 pixels, got {(H, W)}")
        e = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 4))
        o = torch.from_numpy(np.ascontiguousarray(polys, dtype=np.int32).reshape(-1))
        n_include, n_exclude = int(n_include), int(n_exclude)
        if n_include < 0 or n_exclude < 0 or o.numel() != n_include + n_exclude + 1 or int(o[-1]) != e.shape[0]:
            raise ValueError(f"polys holds n_include + n_exclude + 1 offsets that end at the number of edges, got {o.numel()} offsets for "
                             f"{n_include} + {n_exclude} polygons and {e.shape[0]} edges")
        packed = torch.from_numpy(_aoi.aoi_pack(e.numpy(), o.numpy()))
        if table_dev is None:
            table_dev = packed.to(dev)
        if table_dev.device != dev or table_dev.dtype != torch.int32 or tuple(table_dev.shape) != tuple(packed.shape) or not table_dev.is_contiguous():
            raise ValueError(f"table_dev must be aoi_pack(edges, polys) as a contiguous int32 {tuple(packed.shape)} tensor on {dev}")
        n = H * W
        and_with = self._nodata_and(and_with, n, dev)
        if out is None:
            out = torch.empty((H, W), dtype=torch.uint8, device=dev)
        elif out.device != dev or out.dtype != torch.uint8 or out.numel() != n or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of {n} pixels on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        n_rows = max(int(e.shape[0]), 1)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.srh_scene_aoi_fill(ctx.handle, packed.data_ptr(), table_dev.data_ptr(), packed.data_ptr() + 16 * n_rows,
                                                 table_dev.data_ptr() + 16 * n_rows, n_include, n_exclude, H, W,
                                                 None if and_with is None else and_with.data_ptr(), 1 if invert else 0, out.data_ptr(),
                                                 self._stream(dev)), "srh_scene_aoi_fill")
        return out
