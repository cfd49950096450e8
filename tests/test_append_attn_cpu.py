"""The append-attention planner (host only) and the model-level paths on the torch fallback."""
import pytest
import torch

from distributed_pytorch_cookbook_amd.models.gpt import TransformerDecoderLM
from distributed_pytorch_cookbook_amd.ops.attention import APPEND_MAX_SPLITS, append_attn_tiles, append_splits


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_append_splits_plan(cus):
    QB, KT = append_attn_tiles()
    assert append_splits(1, 1, cus * QB, 1 << 20, cus) == 1       # the query tiles cover the CUs
    assert append_splits(8, cus // 8, 8, 1 << 20, cus) == 1
    for Smax in (1, KT, 5 * KT, 4096, 16392, 1 << 20):
        for NH in (1, 12, 96, 4096):
            for n in (2, QB, 4 * QB):
                assert 1 <= append_splits(1, NH, n, Smax, cus) <= max(1, min(-(-Smax // KT), APPEND_MAX_SPLITS))
    assert append_splits(1, 1, 8, 1 << 20, 256) == APPEND_MAX_SPLITS


def test_model_blocks_cpu(monkeypatch):
    """Chunked prefill (shared and ragged) and ragged continuations (a block, then one token with
    lens) against full forwards; a prefill that fails in a later block leaves the cache empty."""
    torch.manual_seed(0)
    m = TransformerDecoderLM(32, 8, 2, 2, 64, 48).eval()
    ids = torch.randint(0, 64, (2, 40))
    pos = torch.arange(40).expand(2, 40)
    with torch.no_grad():
        def full(s, L):
            return m(ids[s:s + 1, :L], pos[:1, :L])[:, -1:]

        for lens in (None, [37, 12]):
            cache = m.new_kv_cache(2, 44, ragged=lens is not None)
            lg = m.decode(ids[:, :37], pos[:, :37], cache, lens=lens, prefill_chunk=8)
            for s in (0, 1):
                torch.testing.assert_close(lg[s:s + 1], full(s, (lens or [37, 37])[s]), rtol=1e-4, atol=1e-4)
        for blk, lens, want in [(torch.stack([ids[0, 37:39], ids[1, 12:14]]), [2, 1], [39, 13]),
                                (torch.stack([ids[0, 39:40], ids[1, 13:14]]), [1, 1], [40, 14])]:
            lg = m.decode(blk, None, cache, lens=lens)
            assert cache.lens == want and cache.len_t.tolist() == want
            for s in (0, 1):
                torch.testing.assert_close(lg[s:s + 1], full(s, want[s]), rtol=1e-4, atol=1e-4)
        with pytest.raises(ValueError):
            m.decode(torch.stack([ids[0, :2], ids[1, :2]]), None, cache)

        def fail(*args, **kw):
            raise RuntimeError("append failed")

        monkeypatch.setattr("distributed_pytorch_cookbook_amd.models.decode.append_attention", fail)
        cache = m.new_kv_cache(2, 44, ragged=True)
        with pytest.raises(RuntimeError):
            m.decode(ids[:, :37], pos[:, :37], cache, lens=[37, 12], prefill_chunk=8)
        assert (cache.len, cache.lens, cache.len_t.tolist()) == (0, [0, 0], [0, 0])
