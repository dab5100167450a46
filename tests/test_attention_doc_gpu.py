"""Document-masked flash attention (packed sequences) vs the fp32 reference with the same bounds (GPU).

Error measure and limits as in test_attention_gpu.py: max-abs over max-abs, below 2e-2 for the
forward and 3e-2 for dq / dk / dv.  Document layouts are lengths per batch row."""

import pytest
import torch

from easydl_amd.ops.attention import attention_ref, flash_attention, segment_bounds

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 2e-2, 3e-2


def _mk(B, S, H, KV, dev, seed, D=128):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randn(B, S, H, D, device=dev, generator=g).to(torch.bfloat16).transpose(1, 2)
    k = torch.randn(B, S, KV, D, device=dev, generator=g).to(torch.bfloat16).transpose(1, 2)
    v = torch.randn(B, S, KV, D, device=dev, generator=g).to(torch.bfloat16).transpose(1, 2)
    return q, k, v


def _err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def _segments(rows, dev):
    """Lengths per batch row -> segment ids [B, S]."""
    return torch.stack([torch.repeat_interleave(torch.arange(len(r)), torch.tensor(r)) for r in rows]).to(dev)


def _run(q, k, v, do, causal, bounds):
    """flash_attention forward + backward -> (o, dq, dk, dv)."""
    q1, k1, v1 = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = flash_attention(q1, k1, v1, causal=causal, bounds=bounds)
    o.backward(do)
    return o.detach(), q1.grad, k1.grad, v1.grad


def _check_against_ref(cuda, B, S, H, KV, D, causal, rows, seed):
    assert all(sum(r) == S for r in rows) and len(rows) == B
    q, k, v = _mk(B, S, H, KV, cuda, seed, D)
    bounds = segment_bounds(_segments(rows, cuda))
    do = torch.randn(B, H, S, D, device=cuda).to(torch.bfloat16)
    o, dq, dk, dv = _run(q, k, v, do, causal, bounds)
    assert o.shape == (B, H, S, D)
    q2, k2, v2 = (t.detach().float().requires_grad_() for t in (q, k, v))
    o2 = attention_ref(q2, k2, v2, causal=causal, bounds=bounds)
    o2.backward(do.float())
    errs = {"forward": _err(o, o2), "dq": _err(dq, q2.grad), "dk": _err(dk, k2.grad), "dv": _err(dv, v2.grad)}
    print(f"\n[attn-doc] S={S} D={D} causal={causal} rows={rows}: {errs}")
    assert errs["forward"] < FWD_TOL, errs
    for n in ("dq", "dk", "dv"):
        assert errs[n] < BWD_TOL, (n, errs)


@pytest.mark.parametrize("causal", [True, False])
def test_boundaries_off_tile_edges_one_token_document_and_tail(cuda, causal):
    """Starts 0, 70, 71, 128: 128 is a workgroup edge, 71 inside a wave, one 1-token document; S = 200 has a
    tail tile."""
    _check_against_ref(cuda, 1, 200, 4, 1, 128, causal, [[70, 1, 57, 72]], 11)


@pytest.mark.parametrize("rows", [[[512, 512], [100, 924]], [[192, 832], [192, 832]]])
def test_tile_skipping_with_odd_first_tile(cuda, rows):
    """Workgroups start at key tiles 8 and 1 (a layout per row) and at tile 3 (an odd first tile lands in
    LDS stage 1)."""
    _check_against_ref(cuda, 2, 1024, 8, 2, 128, True, rows, 12)


@pytest.mark.parametrize("causal", [True, False])
def test_xcd_decode_path(cuda, causal):
    """B*KV % 8 == 0: the XCD-aware work decode of the forward and dQ kernels."""
    _check_against_ref(cuda, 2, 384, 16, 4, 128, causal, [[128, 256], [128, 256]], 13)


@pytest.mark.parametrize("causal", [True, False])
def test_head_dim_64(cuda, causal):
    _check_against_ref(cuda, 2, 200, 4, 4, 64, causal, [[70, 1, 57, 72], [200]], 14)


@pytest.mark.parametrize("causal", [True, False])
def test_single_document_equals_plain_attention(cuda, causal):
    B, S, H, KV = 1, 384, 8, 2
    q, k, v = _mk(B, S, H, KV, cuda, 15)
    do = torch.randn(B, H, S, 128, device=cuda).to(torch.bfloat16)
    doc = _run(q, k, v, do, causal, segment_bounds(_segments([[S]], cuda)))
    plain = _run(q, k, v, do, causal, None)
    assert _err(doc[0], plain[0]) < FWD_TOL
    for n, a, b in zip(("dq", "dk", "dv"), doc[1:], plain[1:]):
        assert _err(a, b) < BWD_TOL, n


def test_no_leak_across_documents(cuda):
    """Document 1's outputs and gradients do not depend on document 0 (scaled by 8 and drawn anew), and
    equal the kernels run on document 1 alone."""
    B, S, H, KV, L = 1, 1024, 8, 2, 512
    q, k, v = _mk(B, S, H, KV, cuda, 16)
    do = torch.randn(B, H, S, 128, device=cuda).to(torch.bfloat16)
    bounds = segment_bounds(_segments([[L, L]], cuda))
    before = _run(q, k, v, do, True, bounds)
    q8, k8, v8 = _mk(B, S, H, KV, cuda, 17)
    mixed = []
    for fresh, old in ((q8, q), (k8, k), (v8, v)):
        t = old.clone()
        t[:, :, :L] = fresh[:, :, :L] * 8
        mixed.append(t)
    after = _run(*mixed, do, True, bounds)
    alone = _run(*(t[:, :, L:] for t in (q, k, v)), do[:, :, L:], True,
                 segment_bounds(_segments([[L]], cuda)))
    for n, tol, a, b, c in zip(("o", "dq", "dk", "dv"), (FWD_TOL, BWD_TOL, BWD_TOL, BWD_TOL), after, before, alone):
        assert torch.isfinite(a.float()).all(), n
        assert _err(a[:, :, L:], b[:, :, L:]) < tol, (n, "changed with document 0")
        assert _err(b[:, :, L:], c) < tol, (n, "differs from document 1 alone")


@pytest.mark.parametrize("recompute", [False, True])
def test_llama_with_segment_ids_matches_fp32_cpu_model(cuda, recompute):
    """The setup of test_llama_on_hip_kernels_matches_fp32_cpu_model with packed documents."""
    from easydl_amd.models.llama import Llama, get_config
    cfg = get_config("llama-tiny", dim=512, n_heads=4, n_kv_heads=2, ffn_dim=512, n_layers=2, vocab_size=512)
    torch.manual_seed(0)
    ref = Llama(cfg, device="cpu", dtype=torch.float32)
    cfg_gpu = get_config("llama-tiny", dim=512, n_heads=4, n_kv_heads=2, ffn_dim=512, n_layers=2, vocab_size=512,
                         recompute=recompute)
    m = Llama(cfg_gpu, device=cuda, dtype=torch.bfloat16)
    with torch.no_grad():
        for (n, p), (n2, p2) in zip(ref.named_parameters(), m.named_parameters()):
            assert n == n2
            p.copy_(p.to(torch.bfloat16).float())       # identical (bf16-representable) weights
            p2.copy_(p)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, cfg.vocab_size, (2, 257), generator=g)
    x, y = ids[:, :-1], ids[:, 1:].clone()
    seg = _segments([[100, 156], [256]], "cpu")
    last = torch.ones_like(seg, dtype=torch.bool)
    last[:, :-1] = seg[:, 1:] != seg[:, :-1]
    y[last] = -100
    loss_ref = ref(x, y, seg)
    loss_ref.backward()
    loss = m(x.to(cuda), y.to(cuda), seg.to(cuda))
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) / loss_ref.item() < 1e-2
    for (n, p), (_, p2) in zip(ref.named_parameters(), m.named_parameters()):
        err = ((p2.grad.float().cpu() - p.grad).norm() / p.grad.norm().clamp_min(1e-12)).item()
        assert err < 5e-2, (n, err)


class _Entries:
    """The two launch entries on zeroed buffers at B 1, S 128: every pointer is the same bf16 buffer, lse and
    delta one fp32 buffer, so a rejected call must leave both all zero."""

    def __init__(self, cuda, H, KV, D):
        from easydl_amd import _native
        self.kn = _native.kernels()
        self.B, self.S, self.H, self.KV, self.D = 1, 128, H, KV, D
        self.buf = torch.zeros(self.B * self.S * H * 128, dtype=torch.bfloat16, device=cuda)
        self.f32 = torch.zeros(2 * self.B * H * self.S, dtype=torch.float32, device=cuda)
        self.bounds = segment_bounds(_segments([[self.S]], cuda))
        self.st = _native.stream_of(self.buf)

    def fwd(self, dstart, dend):
        p, (B, S, H, KV, D) = self.buf.data_ptr(), (self.B, self.S, self.H, self.KV, self.D)
        return self.kn.raw("edl_attn_fwd")(p, p, p, p, self.f32.data_ptr(), B, S, H, KV, D, 1, 0.1, H * D, KV * D,
                                           dstart, dend, self.st)

    def bwd(self, ws, dstart, dend):
        p, f, (B, S, H, KV, D) = self.buf.data_ptr(), self.f32.data_ptr(), (self.B, self.S, self.H, self.KV, self.D)
        return self.kn.raw("edl_attn_bwd")(p, p, p, p, p, f, f, p, p, p, ws, B, S, H, KV, D, 1, 0.1, H * D, KV * D,
                                           KV * D, dstart, dend, self.st)

    def untouched(self):
        torch.cuda.synchronize()
        return not self.buf.any() and not self.f32.any()


@pytest.mark.parametrize("H,KV,D", [(4, 2, 96), (5, 2, 128)])
def test_doc_entries_reject_bad_arguments(cuda, H, KV, D):
    """Head dim 96 and H % KV != 0 are errors of both entries, with bounds and with null bounds, before any
    launch (no buffer is touched)."""
    e = _Entries(cuda, H, KV, D)
    for dstart, dend in ((e.bounds[0].data_ptr(), e.bounds[1].data_ptr()), (None, None)):
        assert e.fwd(dstart, dend) != 0
        assert e.bwd(None, dstart, dend) != 0
    assert e.untouched()


def test_entries_reject_one_null_bound(cuda):
    """dstart and dend come as a pair: exactly one of them null is an error of both entries before any launch."""
    e = _Entries(cuda, 4, 2, 128)
    for dstart, dend in ((e.bounds[0].data_ptr(), None), (None, e.bounds[1].data_ptr())):
        assert e.fwd(dstart, dend) != 0
        assert e.bwd(None, dstart, dend) != 0
    assert e.untouched()


def test_backward_rejects_null_workspace_when_the_query_is_positive(cuda):
    """B 1, S 128, H 4, KV 2, D 128, causal, no bounds: the 64-key dK/dV kernel splits the GQA group and needs
    its workspace; a null ws is an error before any launch."""
    e = _Entries(cuda, 4, 2, 128)
    assert e.bwd(None, None, None) != 0
    assert e.untouched()


def test_workspace_query_follows_the_dkdv_kernel(cuda):
    """The query is positive only where the 64-key dK/dV kernel runs: not at head dim 64, not with bounds."""
    from easydl_amd import _native
    query = _native.kernels().raw("edl_attn_bwd_ws_bytes")
    assert query(1, 128, 4, 2, 128, 1, 0) > 0
    assert query(1, 128, 4, 2, 64, 1, 0) == 0
    assert query(1, 128, 4, 2, 128, 1, 1) == 0
