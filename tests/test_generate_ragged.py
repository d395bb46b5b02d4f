"""Ragged generate() — what needs no GPU: the C surface of the per-row-position kernels (exported, validated before any launch),
the ``prompt_lengths`` keyword of both model classes and its argument checks (kosmosx.generation.resolve_prompt_lengths is the
device-free path: generate() itself refuses CPU tensors before it looks at anything else)."""
import ctypes as C
import inspect

import pytest
import torch

from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
RAGGED_SYMBOLS = ("kx_attention_decode_ragged", "kx_step_prepare", "kx_sample_logits_ragged", "kx_decoder_decode_step_ragged")


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from kosmosx import _hip
    return _hip.load()


def _good_args():
    from kosmosx import _hip
    a = _hip.SampleArgs()
    a.do_sample, a.logits, a.ld, a.B, a.V = 1, 256, 512, 2, 502
    a.temperature, a.top_k, a.top_p, a.repetition_penalty = 1.0, 0, 1.0, 1.0
    a.next_token = 256
    a.eos_id, a.pad_id = -1, 1
    return a


def test_the_library_exports_the_ragged_entry_points_within_abi_7(lib):
    from kosmosx import _hip
    for name in RAGGED_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _hip.SYMBOLS
    assert lib.kx_version() == 7
    assert (_hip.KX_RAGGED_ERR_TABLE, _hip.KX_RAGGED_ERR_CACHE) == (1, 2)


def test_ragged_entry_points_validate_without_a_launch(lib):
    from kosmosx import _hip
    a = _good_args()
    assert lib.kx_sample_logits_ragged(C.byref(a), None, 1, None) == 1 and "positions" in _hip.last_error()
    assert lib.kx_sample_logits_ragged(C.byref(a), 256, -1, None) == 1 and "advance" in _hip.last_error()
    a.position = -5                                                        # ignored by the ragged form, refused by the uniform one
    a.top_p = 0.0
    assert lib.kx_sample_logits_ragged(C.byref(a), 256, 1, None) == 1 and "top_p" in _hip.last_error()
    a = _good_args()
    a.position = -5
    assert lib.kx_sample_logits(C.byref(a), None) == 1 and "position" in _hip.last_error()
    # attention: positions and the error word are mandatory, the other checks are kx_attention_decode's
    assert lib.kx_attention_decode_ragged(256, 256, 256, 256, 0, None, 2, 4, None, 64, 1, 256, None) == 1
    assert "positions" in _hip.last_error()
    assert lib.kx_attention_decode_ragged(256, 256, 256, 256, 0, None, 2, 4, 256, 64, 1, None, None) == 1
    assert "error_word" in _hip.last_error()
    assert lib.kx_attention_decode_ragged(256, 256, 256, 256, 0, None, 2, 4, 256, 0, 1, 256, None) == 1
    assert lib.kx_attention_decode_ragged(256, 256, 256, 256, 0, None, 2, 4, 256, 64, 2, 256, None) == 1   # bf16x3: no cache kernels
    assert "precision" in _hip.last_error()
    # step prepare: tokens, embed, pos, positions, 4 tables, x, xpos_rows, B, d, vocab, max_pos, pos_shift, xpos_len, err, stream
    assert lib.kx_step_prepare(256, 256, 256, None, 256, 256, 256, 256, 256, 256, 2, 256, 502, 64, 0, 64, 256, None) == 1
    assert "null" in _hip.last_error()
    assert lib.kx_step_prepare(256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 2, 256, 502, 64, 0, 64, None, None) == 1
    assert "null" in _hip.last_error()
    assert lib.kx_step_prepare(256, 256, 256, 256, 256, 256, 256, None, 256, 256, 2, 256, 502, 64, 0, 64, 256, None) == 1
    assert "together" in _hip.last_error()                                 # three tables of four
    assert lib.kx_step_prepare(256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 2, 258, 502, 64, 0, 64, 256, None) == 1
    assert "shape" in _hip.last_error()                                    # d % 4
    # the ragged step refuses a stale binding before it reads a layer pointer, like every stage entry point
    w = _hip.DecoderWeights()
    w.layer_bytes -= 8
    rc = lib.kx_decoder_decode_step_ragged(C.byref(w), 256, 256, 256, 502, 64, 0, 256, 2, 256, 256, 256, 256, 256, 256, 256, 256,
                                           64, 256, 0, 256, 1 << 20, 1, 256, None)
    assert rc == 1 and "stale binding" in _hip.last_error()
    w = _hip.DecoderWeights()
    rc = lib.kx_decoder_decode_step_ragged(C.byref(w), 256, 256, 256, 502, 64, 0, 256, 2, None, 256, 256, 256, 256, 256, 256, 256,
                                           64, 256, 0, 256, 1 << 20, 1, 256, None)
    assert rc == 1 and "null" in _hip.last_error()


def test_both_generate_signatures_take_prompt_lengths():
    from kosmosx.model import Kosmos, KosmosLanguage
    for cls in (Kosmos, KosmosLanguage):
        p = inspect.signature(cls.generate).parameters["prompt_lengths"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_prompt_lengths_are_validated_on_the_host():
    from kosmosx import generation as G
    assert G.resolve_prompt_lengths([3, 9, 1, 6], 4, 9) == [3, 9, 1, 6]
    assert G.resolve_prompt_lengths((2, 10), 2, 10, min_len=2) == [2, 10]
    assert G.resolve_prompt_lengths(torch.tensor([3, 9, 1, 6], dtype=torch.int32), 4, 9) == [3, 9, 1, 6]
    import numpy as np
    assert G.resolve_prompt_lengths(np.array([4, 5]), 2, 5) == [4, 5]
    with pytest.raises(ValueError, match="4 entries"):
        G.resolve_prompt_lengths([3, 9, 1], 4, 9)
    with pytest.raises(ValueError, match="4 entries"):
        G.resolve_prompt_lengths(torch.tensor([3, 9, 1, 6, 2]), 4, 9)
    with pytest.raises(ValueError, match="entries"):
        G.resolve_prompt_lengths(torch.tensor([[3, 9], [1, 6]]), 4, 9)
    with pytest.raises(ValueError, match="at least 1 token"):
        G.resolve_prompt_lengths([3, 0, 1, 6], 4, 9)
    with pytest.raises(ValueError, match="at least 1 token"):
        G.resolve_prompt_lengths([3, -2, 1, 6], 4, 9)
    with pytest.raises(ValueError, match="at least 2 tokens.*spliced after two"):
        G.resolve_prompt_lengths([10, 1], 2, 10, min_len=2)                # Kosmos: the image goes after two text tokens
    with pytest.raises(ValueError, match="exceeds the padded width 9"):
        G.resolve_prompt_lengths([3, 10, 1, 6], 4, 9)
    with pytest.raises(ValueError, match="integers"):
        G.resolve_prompt_lengths([3.0, 9, 1, 6], 4, 9)
    with pytest.raises(ValueError, match="integers"):
        G.resolve_prompt_lengths(torch.tensor([3.0, 9.0, 1.0, 6.0]), 4, 9)
    with pytest.raises(ValueError, match="integers"):
        G.resolve_prompt_lengths(7, 4, 9)


def test_the_budget_counts_the_longest_row_and_keeps_its_wording():
    from kosmosx import generation as G
    from kosmosx.model import KosmosLanguage
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=64).eval()
    lens = G.resolve_prompt_lengths([3, 9, 1, 6], 4, 30)                   # a width of 30 with 21 columns nobody uses
    G.check_budget(lm.decoder, max(lens), 62 - 9)
    with pytest.raises(IndexError, match="index out of range in self: 9 prompt positions"):
        G.check_budget(lm.decoder, max(lens), 62 - 9 + 1)


def test_padding_is_replaced_by_the_rows_first_token():
    from kosmosx import generation as G
    tok = torch.arange(20).reshape(4, 5)
    got = G.mask_padding(tok, [5, 1, 3, 2])
    want = torch.tensor([[0, 1, 2, 3, 4], [5, 5, 5, 5, 5], [10, 11, 12, 10, 10], [15, 16, 15, 15, 15]])
    assert torch.equal(got, want)
