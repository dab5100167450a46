"""Document masking for packed sequences on the CPU reference path: segment_bounds, flash_attention /
attention_ref with bounds, Llama with segment_ids, and the PackedTokens source."""

import pytest
import torch

from easydl_amd.ops.attention import attention_ref, flash_attention, segment_bounds


def test_segment_bounds_of_runs():
    seg = torch.tensor([[5, 5, 5, 2, 2, 9], [1, 1, 1, 1, 1, 1]])
    b = segment_bounds(seg)
    assert b.shape == (2, 2, 6) and b.dtype == torch.int32 and b.is_contiguous()
    assert b[0].tolist() == [[0, 0, 0, 3, 3, 5], [0] * 6]
    assert b[1].tolist() == [[3, 3, 3, 5, 5, 6], [6] * 6]


def test_segment_bounds_repeated_id_is_a_new_document():
    """A document is a maximal run: the same id after another document starts a new one."""
    b = segment_bounds(torch.tensor([[0, 0, 1, 0]], dtype=torch.int32))
    assert b[0].tolist() == [[0, 0, 2, 3]] and b[1].tolist() == [[2, 2, 3, 4]]


@pytest.mark.parametrize("causal", [True, False])
def test_cpu_flash_attention_with_bounds_is_per_document_attention(causal):
    B, S, H, KV, D = 2, 48, 4, 2, 16
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, H, S, D, generator=g)
    k, v = torch.randn(B, KV, S, D, generator=g), torch.randn(B, KV, S, D, generator=g)
    rows = [[17, 1, 30], [48]]
    seg = torch.stack([torch.repeat_interleave(torch.arange(len(r)), torch.tensor(r)) for r in rows])
    o = flash_attention(q, k, v, causal=causal, bounds=segment_bounds(seg))
    for b, lens in enumerate(rows):
        s0 = 0
        for n in lens:
            sl = slice(s0, s0 + n)
            piece = attention_ref(q[b:b + 1, :, sl], k[b:b + 1, :, sl], v[b:b + 1, :, sl], causal=causal)
            assert (o[b:b + 1, :, sl] - piece).abs().max().item() < 1e-5
            s0 += n


def test_bounds_are_validated():
    q = torch.randn(1, 2, 8, 16)
    with pytest.raises(ValueError):
        flash_attention(q, q, q, bounds=torch.zeros(2, 1, 8, dtype=torch.int64))
    with pytest.raises(ValueError):
        flash_attention(q, q, q, bounds=torch.zeros(2, 1, 7, dtype=torch.int32))


def test_llama_segment_ids_isolate_documents():
    from easydl_amd.models.llama import Llama, get_config
    cfg = get_config("llama-tiny", dim=64, n_heads=4, n_kv_heads=2, ffn_dim=128, n_layers=2, vocab_size=128)
    torch.manual_seed(0)
    m = Llama(cfg, device="cpu", dtype=torch.float32).eval()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, cfg.vocab_size, (2, 40), generator=g)
    other = ids.clone()
    other[:, :15] = (ids[:, :15] + 1) % cfg.vocab_size      # every token of document 0 changes
    seg = torch.repeat_interleave(torch.arange(2), torch.tensor([15, 25])).expand(2, 40)
    with torch.no_grad():
        a, b = m(ids, segment_ids=seg), m(other, segment_ids=seg)
        a0, b0 = m(ids), m(other)
    assert (a[:, 15:] - b[:, 15:]).abs().max().item() < 1e-5
    assert (a0[:, 15:] - b0[:, 15:]).abs().max().item() > 1e-3
    # a packed row gives each document the loss it has on its own: positions are relative under RoPE
    alone = m(ids[:, 15:])
    assert (a[:, 15:] - alone).abs().max().item() < 1e-4


def test_packed_tokens_source():
    from easydl_amd.models.llama import Llama, get_config
    from easydl_amd.trainer.data import PackedTokens
    src = PackedTokens(vocab=128, seq=96, mean_doc_len=12, num_samples=1000)
    assert len(src) == 1000
    ids, labels, seg = src.batch([3, 7, 3], "cpu")
    for t in (ids, labels, seg):
        assert t.shape == (3, 96) and t.dtype == torch.long
    assert torch.equal(ids[0], ids[2]) and torch.equal(labels[0], labels[2]) and torch.equal(seg[0], seg[2])
    assert not torch.equal(seg[0], seg[1])
    ids2, labels2, seg2 = src.batch([7], "cpu")
    assert torch.equal(ids2[0], ids[1]) and torch.equal(labels2[0], labels[1]) and torch.equal(seg2[0], seg[1])
    assert ids.min() >= 0 and ids.max() < 128
    for r in range(3):
        lens = src.doc_lengths([3, 7, 3][r])
        assert min(lens) >= 1 and sum(lens) == 96 and len(lens) > 1
        assert seg[r].tolist() == [d for d, n in enumerate(lens) for _ in range(n)]   # non-decreasing runs over seq
        ends = torch.tensor(lens).cumsum(0) - 1
        is_end = torch.zeros(96, dtype=torch.bool)
        is_end[ends] = True
        assert torch.equal(labels[r] == -100, is_end)
        assert torch.equal(labels[r][~is_end], ids[r][1:][~is_end[:-1]])
    cfg = get_config("llama-tiny", dim=64, n_heads=4, n_kv_heads=2, ffn_dim=128, n_layers=1, vocab_size=128)
    torch.manual_seed(0)
    m = Llama(cfg, device="cpu", dtype=torch.float32)
    loss = m(*src.batch([0, 1], "cpu"))
    assert loss.ndim == 0 and torch.isfinite(loss)
