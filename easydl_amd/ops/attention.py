"""Flash attention (csrc/kernels/attention.hip): causal or full, GQA, head_dim 64 or 128, bf16.

Inputs are the ``[B, H, S, D]``-shaped views of token-major ``[B, S, H, D]``
memory that the fused RoPE+QKV kernel produces; the output is returned the
same way, so ``o.transpose(1, 2).reshape(B*S, H*D)`` feeding the output
projection is free.  The forward saves only O and the log-sum-exp (fp32
[B,H,S]); the backward recomputes P tile by tile (dK/dV kernel + dQ kernel,
no float atomics).  ``EDL_ATTN=sdpa`` falls back to PyTorch SDPA (used for
A/B comparisons); other head dims also use SDPA.  Head dim 64 (BERT-large,
Llama-3.2-1B/3B) runs the same kernels instantiated for 128-byte rows.

Packed sequences: ``bounds = segment_bounds(segment_ids)`` restricts every query
to the keys of its own document (``flash_attention(..., bounds=bounds)``).  The
document-masked kernels skip the key / query tiles outside a block's documents,
so a row of eight 1024-token documents costs about an eighth of a full causal row.
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F

from easydl_amd import _native

# EDL_ATTN_QKV_SPLIT=1: split packed qkv into three tensors before the forward (A/B)
_QKV_SPLIT = os.environ.get("EDL_ATTN_QKV_SPLIT", "0") == "1"


def _bshd(t: torch.Tensor) -> torch.Tensor:
    """[B,H,S,D]-shaped tensor -> contiguous [B,S,H,D] memory (no copy if already laid out so)."""
    return t.transpose(1, 2).contiguous()


def _bound_ptrs(bounds):
    return (None, None) if bounds is None else (bounds[0].data_ptr(), bounds[1].data_ptr())


def _attn_fwd(qp, kp, vp, o, KV, causal, scale, qis, kvs, bounds=None):
    """The forward kernel into ``o`` (contiguous [B,S,H,D]); returns the log-sum-exp.  ``qp`` / ``kp`` /
    ``vp`` are device pointers to token-major rows ``qis`` / ``kvs`` elements apart."""
    B, S, H, D = o.shape
    lse = torch.empty(B, H, S, dtype=torch.float32, device=o.device)
    _native.kernels().check("edl_attn_fwd", qp, kp, vp, o.data_ptr(), lse.data_ptr(), B, S, H, KV, D,
                            1 if causal else 0, scale, qis, kvs, *_bound_ptrs(bounds), _native.stream_of(o))
    return lse


def _attn_bwd(qm, kp, vp, o, dom, lse, dqp, dkp, dvp, KV, causal, scale, dqs, dkvs, kvs, bounds=None):
    """The backward kernels: ``qm`` / ``o`` / ``dom`` contiguous [B,S,H,D]; k / v pointers with rows ``kvs``
    apart; dq / dk / dv pointers with rows ``dqs`` / ``dkvs`` apart."""
    kn = _native.kernels()
    B, S, H, D = qm.shape
    delta = torch.empty(2, B, H, S, dtype=torch.float32, device=qm.device)  # (delta, -lse*log2e)
    causal = 1 if causal else 0
    # fp32 partials when the GQA group is split over workgroups (csrc/kernels/attention.hip dkdv64_plan)
    nws = kn.raw("edl_attn_bwd_ws_bytes")(B, S, H, KV, D, causal, 0 if bounds is None else 1)
    ws = torch.empty(nws // 4, dtype=torch.float32, device=qm.device) if nws else None
    kn.check("edl_attn_bwd", qm.data_ptr(), kp, vp, o.data_ptr(), dom.data_ptr(), lse.data_ptr(), delta.data_ptr(),
             dqp, dkp, dvp, _native.ptr(ws), B, S, H, KV, D, causal, scale, dqs, dkvs, kvs, *_bound_ptrs(bounds),
             _native.stream_of(qm))


class _FlashAttnFn(torch.autograd.Function):
    """``bounds``: int32 [2, B, S] = (dstart, dend) of every token (document mask), or None."""

    @staticmethod
    def forward(ctx, q, k, v, bounds, causal, scale):
        B, H, S, D = q.shape
        KV = k.shape[1]
        qm, km, vm = _bshd(q), _bshd(k), _bshd(v)
        o = torch.empty_like(qm)
        lse = _attn_fwd(qm.data_ptr(), km.data_ptr(), vm.data_ptr(), o, KV, causal, scale, H * D, KV * D, bounds)
        ctx.save_for_backward(qm, km, vm, o, lse, bounds)
        ctx.causal, ctx.scale = causal, scale
        return o.transpose(1, 2)

    @staticmethod
    def backward(ctx, do):
        qm, km, vm, o, lse, bounds = ctx.saved_tensors
        _, _, H, D = qm.shape
        KV = km.shape[2]
        dq, dk, dv = torch.empty_like(qm), torch.empty_like(km), torch.empty_like(vm)
        _attn_bwd(qm, km.data_ptr(), vm.data_ptr(), o, _bshd(do), lse, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                  KV, ctx.causal, ctx.scale, H * D, KV * D, KV * D, bounds)
        return dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2), None, None, None


class _PackedQKVAttnFn(torch.autograd.Function):
    """Attention over one packed ``[B*S, 3*H*D]`` q|k|v projection (BERT's fused qkv
    Linear).  The forward kernels read q, k and v as row-strided slices of the packed
    tensor (row stride 3*H*D, no split pass); the backward copies q out once (the dK/dV
    kernel stages q and dO tiles with one DMA plan) and reads k / v strided.  The backward
    kernels write dq / dk / dv straight into the slices of one packed gradient, so the qkv
    projection's backward gets its input gradient without the concatenation pass
    autograd's unbind would run.  ``EDL_ATTN_QKV_SPLIT=1`` restores the split of all three."""

    @staticmethod
    def forward(ctx, qkv, B, S, H, causal, scale):
        D = qkv.shape[-1] // (3 * H)
        row = H * D
        o = torch.empty(B, S, H, D, dtype=qkv.dtype, device=qkv.device)
        if _QKV_SPLIT:
            qm, km, vm = (torch.empty(B, S, H, D, dtype=qkv.dtype, device=qkv.device) for _ in range(3))
            _native.kernels().check("edl_qkv_split", qkv.data_ptr(), qm.data_ptr(), km.data_ptr(), vm.data_ptr(),
                                    B * S, row, _native.stream_of(qkv))
            lse = _attn_fwd(qm.data_ptr(), km.data_ptr(), vm.data_ptr(), o, H, causal, scale, row, row)
            ctx.save_for_backward(qm, km, vm, o, lse)
        else:
            base, es = qkv.data_ptr(), qkv.element_size()
            lse = _attn_fwd(base, base + row * es, base + 2 * row * es, o, H, causal, scale, 3 * row, 3 * row)
            ctx.save_for_backward(qkv, o, lse)
        ctx.causal, ctx.scale, ctx.shape = causal, scale, (B, S, H, D)
        return o.view(B * S, H * D)

    @staticmethod
    def backward(ctx, do):
        B, S, H, D = ctx.shape
        row = H * D
        saved = ctx.saved_tensors
        if len(saved) == 5:
            qm, km, vm, o, lse = saved
            kptr, vptr, kvs = km.data_ptr(), vm.data_ptr(), row
        else:
            qkv, o, lse = saved
            qm = torch.empty(B, S, H, D, dtype=qkv.dtype, device=qkv.device)
            _native.kernels().check("edl_qkv_split", qkv.data_ptr(), qm.data_ptr(), None, None, B * S, row,
                                    _native.stream_of(do))
            es = qkv.element_size()
            kptr, vptr, kvs = qkv.data_ptr() + row * es, qkv.data_ptr() + 2 * row * es, 3 * row
        dom = do.reshape(B, S, H, D).contiguous()
        dqkv = torch.empty(B * S, 3 * row, dtype=qm.dtype, device=qm.device)
        base, es = dqkv.data_ptr(), dqkv.element_size()
        _attn_bwd(qm, kptr, vptr, o, dom, lse, base, base + row * es, base + 2 * row * es, H, ctx.causal, ctx.scale,
                  3 * row, 3 * row, kvs)
        return dqkv, None, None, None, None, None


def packed_qkv_attention(qkv: torch.Tensor, B: int, S: int, H: int, causal: bool = False,
                         scale: float | None = None) -> torch.Tensor:
    """``qkv`` [B*S, 3*H*D] (q | k | v per token, multi-head) -> attention output [B*S, H*D]."""
    D = qkv.shape[-1] // (3 * H)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if (qkv.is_cuda and D in (64, 128) and qkv.dtype == torch.bfloat16 and qkv.is_contiguous()
            and os.environ.get("EDL_ATTN", "hip") != "sdpa" and os.environ.get("EDL_ATTN_PACKED", "1") != "0"):
        return _PackedQKVAttnFn.apply(qkv, B, S, H, causal, scale)
    q, k, v = (t.transpose(1, 2) for t in qkv.view(B, S, 3, H, D).unbind(2))
    return flash_attention(q, k, v, causal, scale).transpose(1, 2).reshape(B * S, H * D)


def segment_bounds(segment_ids: torch.Tensor) -> torch.Tensor:
    """Integer ``segment_ids`` [B, S] -> int32 [2, B, S]: ``dstart`` (first token of each token's
    document) and ``dend`` (one past its last token).  A document is a maximal run of equal ids."""
    B, S = segment_ids.shape
    pos = torch.arange(S, device=segment_ids.device).expand(B, S)
    first = torch.ones(B, S, dtype=torch.bool, device=segment_ids.device)
    first[:, 1:] = segment_ids[:, 1:] != segment_ids[:, :-1]
    dstart = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), dim=1).values
    # a run ends where the next one starts: reversed running minimum of the next run's start
    nxt = torch.full((B, S), S, dtype=pos.dtype, device=pos.device)
    nxt[:, :-1] = torch.where(first[:, 1:], pos[:, 1:], nxt[:, 1:])
    dend = torch.cummin(nxt.flip(1), dim=1).values.flip(1)
    return torch.stack((dstart, dend)).to(torch.int32).contiguous()


def _check_bounds(bounds: torch.Tensor, q: torch.Tensor) -> None:
    B, _, S, _ = q.shape
    if bounds.shape != (2, B, S) or bounds.dtype != torch.int32 or bounds.device != q.device:
        raise ValueError(f"bounds must be int32 [2, {B}, {S}] on {q.device} (segment_bounds(segment_ids)), got "
                         f"{bounds.dtype} {tuple(bounds.shape)} on {bounds.device}")


def doc_mask(bounds: torch.Tensor, causal: bool) -> torch.Tensor:
    """Boolean [B, 1, S, S] visibility mask of ``bounds``: key j is visible to query i iff
    dstart[i] <= j < dend[i] (and j <= i when causal)."""
    S = bounds.shape[-1]
    j = torch.arange(S, device=bounds.device)
    vis = (j >= bounds[0].unsqueeze(-1)) & (j < bounds[1].unsqueeze(-1))
    if causal:
        vis = vis & (j <= j.unsqueeze(-1))
    return vis.unsqueeze(1)


def attention_ref(q, k, v, causal=True, scale=None, bounds=None):
    """fp32 reference (GQA by head repetition); ``bounds`` adds the document mask."""
    H, KV = q.shape[1], k.shape[1]
    if H != KV:
        k = k.repeat_interleave(H // KV, dim=1)
        v = v.repeat_interleave(H // KV, dim=1)
    if bounds is not None:
        _check_bounds(bounds, q)
        return F.scaled_dot_product_attention(q.float(), k.float(), v.float(), attn_mask=doc_mask(bounds, causal),
                                              scale=scale).to(q.dtype)
    return F.scaled_dot_product_attention(q.float(), k.float(), v.float(), is_causal=causal,
                                          scale=scale).to(q.dtype)


def flash_attention(q, k, v, causal: bool = True, scale: float | None = None, bounds: torch.Tensor | None = None):
    """q [B,H,S,D], k/v [B,KV,S,D] -> [B,H,S,D].  ``bounds`` (``segment_bounds(segment_ids)``,
    int32 [2,B,S]) keeps attention inside each token's document; ``None`` is plain attention."""
    D = q.shape[-1]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if bounds is not None:
        _check_bounds(bounds, q)
        if not q.is_cuda:
            return attention_ref(q, k, v, causal, scale, bounds)
        if D in (64, 128) and q.dtype == torch.bfloat16 and os.environ.get("EDL_ATTN", "hip") != "sdpa":
            return _FlashAttnFn.apply(q, k, v, bounds.contiguous(), causal, scale)
        return F.scaled_dot_product_attention(q, k, v, attn_mask=doc_mask(bounds, causal), scale=scale,
                                              enable_gqa=q.shape[1] != k.shape[1])
    if q.is_cuda:
        if D in (64, 128) and q.dtype == torch.bfloat16 and os.environ.get("EDL_ATTN", "hip") != "sdpa":
            return _FlashAttnFn.apply(q, k, v, None, causal, scale)
        return F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=scale,
                                              enable_gqa=q.shape[1] != k.shape[1])
    return attention_ref(q, k, v, causal, scale)
