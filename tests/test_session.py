"""Sessions without a GPU: generate()'s refusals of the session arguments (before the device check), Session's own host-side
checks, the turn bookkeeping against a token-by-token restatement, and the library's two new entry points, which validate before
any launch."""
import ctypes as C
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from kosmosx import _hip
    return _hip.load()


def _models():
    """generate(**kw) of a KosmosLanguage and of a Kosmos, on CPU tensors."""
    from helpers import tiny_config
    from kosmosx.model import Kosmos, KosmosLanguage
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    tok = torch.zeros(2, 4, dtype=torch.long)
    img = torch.zeros(2, 3, m.cfg.vit.image, m.cfg.vit.image)
    return [(lambda **kw: lm.generate(tok, 4, **kw), lm), (lambda **kw: m.generate(tok, img, 4, **kw), m)]


@pytest.mark.parametrize("name,kw", [("return_session", dict(return_session=True, num_beams=2)),
                                     ("return_session", dict(return_session=True, prompt_lookup_num_tokens=2)),
                                     ("session_capacity", dict(return_session=True, session_capacity=0)),
                                     ("session_capacity", dict(return_session=True, session_capacity=True)),
                                     ("session_capacity", dict(return_session=True, session_capacity=2.5)),
                                     ("session_capacity", dict(return_session=True, session_capacity=1 << 20)),
                                     ("session_capacity", dict(session_capacity=16))])
def test_generate_refuses_with_a_value_error_that_names_the_argument(name, kw):
    """CPU tensors: the ValueError comes before the device check, hence before any launch."""
    for gen, _ in _models():
        with pytest.raises(ValueError, match=name):
            gen(**kw)


def test_what_generate_accepts_reaches_the_device_check():
    for gen, _ in _models():
        for kw in (dict(return_session=True), dict(return_session=True, session_capacity=20), dict(return_session=False)):
            with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
                gen(**kw)


def test_session_generate_and_append_check_the_turn_on_the_host():
    from kosmosx.generation import Session
    for _, model in _models():
        s = Session(model, {"batch": 2}, 20)
        assert s.capacity == 20 and s.lengths == [0, 0] and s.batch == 2
        x = torch.zeros(2, 4, dtype=torch.long)
        for call in (lambda x, **kw: s.generate(x, 3, **kw), s.append):
            with pytest.raises(ValueError, match="keeps its batch size"):
                call(torch.zeros(3, 4, dtype=torch.long))
            with pytest.raises(ValueError, match="prompt_lengths must have 2 entries"):
                call(x, prompt_lengths=[1, 2, 3])
            with pytest.raises(ValueError, match=r"prompt_lengths\[0\] = 0"):
                call(x, prompt_lengths=[0, 2])
            with pytest.raises(ValueError, match="exceeds the padded width"):
                call(x, prompt_lengths=[1, 5])
            with pytest.raises(ValueError, match="at least one token"):
                call(torch.zeros(2, 0, dtype=torch.long))
            with pytest.raises(TypeError):
                call([[1, 2], [3, 4]])
            with pytest.raises(ValueError, match="prefill_chunk"):
                call(x, prefill_chunk=0)
        with pytest.raises(ValueError, match="max_new_tokens"):
            s.generate(x, 0)
        with pytest.raises(ValueError, match="min_new_tokens = 2 needs an eos_token_id"):
            s.generate(x, 3, min_new_tokens=2)
        # the budget: cached rows + the padded block + the new tokens, before the device check
        s._cached = [9, 4]
        with pytest.raises(IndexError, match="exceed the session's 20-row cache"):
            s.generate(x, 8)                                                 # 9 + 4 + 8 = 21
        with pytest.raises(IndexError, match="exceed the session's 20-row cache"):
            s.append(torch.zeros(2, 12, dtype=torch.long))                   # 9 + 12 = 21
        assert s._cached == [9, 4] and s.lengths == [0, 0]
        with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):         # 9 + 4 + 7 = 20 fits: as far as the device check
            s.generate(x, 7)


def _replay_turn(seq, cache, pending, new_ids, generated):
    """One row, token by token.  ``seq``: the logical sequence; ``cache``: the positions whose k / v are valid; ``pending``: the
    token sampled but not fed.  The block (pending, new ids) is fed, then every generated token but the last."""
    for t in ([] if pending is None else [pending]) + list(new_ids):
        cache.append(len(cache))
    seq = seq + list(new_ids)
    for i, t in enumerate(generated):
        seq.append(t)
        if i + 1 < len(generated):
            cache.append(len(cache))
    return seq, cache, (generated[-1] if generated else None)


def test_the_turn_bookkeeping_matches_a_token_by_token_replay():
    from kosmosx.generation import session_after_turn
    g = torch.Generator().manual_seed(0)
    B = 4
    seqs = [list(range(100, 100 + n)) for n in (5, 9, 12, 1)]
    caches, pend = [list(range(len(s))) for s in seqs], [None] * B          # after a prefill every prompt row is cached
    cached = [len(c) for c in caches]
    for turn in range(6):
        new = [torch.randint(0, 90, (int(torch.randint(1, 7, (1,), generator=g)),), generator=g).tolist() for _ in range(B)]
        n_valid = [int(torch.randint(0 if turn == 3 else 1, 6, (1,), generator=g)) for _ in range(B)]   # turn 3: an append-like row
        gen = [torch.randint(0, 90, (n,), generator=g).tolist() for n in n_valid]
        block_lens = [len(x) + (p is not None) for x, p in zip(new, pend)]
        lengths, rows, idx = session_after_turn(cached, block_lens, n_valid)
        for b in range(B):
            seqs[b], caches[b], pend[b] = _replay_turn(seqs[b], caches[b], pend[b], new[b], gen[b])
            assert lengths[b] == len(seqs[b]) and rows[b] == len(caches[b]), (turn, b)
            assert (idx[b] == -1 and pend[b] is None) or gen[b][idx[b]] == pend[b]
            assert rows[b] == lengths[b] - (pend[b] is not None)            # the pending token is the one position not cached
        cached = rows


def test_the_header_and_the_binding_declare_both_entry_points_within_abi_7(lib):
    from kosmosx import _hip
    header = (ROOT / "include" / "kosmosx_hip.h").read_text()
    for name in ("kx_attention_extend_ragged", "kx_decoder_extend_ragged"):
        assert hasattr(lib, name) and name in _hip.SYMBOLS and f"int {name}(" in header, name
    assert "Ragged extend" in header
    assert lib.kx_version() == 7 and lib.kx_struct_bytes(13) == 0 and len(_hip.STRUCT_IDS) == 13
    assert "KX_STRUCT_COUNT = 13" in header and "#define KX_ABI_VERSION 7" in header


def test_the_entry_points_validate_before_any_launch(lib):
    from kosmosx import _hip
    att = lib.kx_attention_extend_ragged
    #           qkv  kc   vc   out  odt stats B  H  Tn positions Tmax prec err stream
    assert att(256, 256, 256, 256, 0, None, 3, 2, 4, None, 64, 1, 256, None) == 1 and "null positions" in _hip.last_error()
    assert att(256, 256, 256, 256, 0, None, 3, 2, 4, 256, 64, 1, None, None) == 1 and "error_word" in _hip.last_error()
    for k in range(4):
        ptrs = [256] * 4
        ptrs[k] = None
        assert att(*ptrs, 0, None, 3, 2, 4, 256, 64, 1, 256, None) == 1 and "null pointer" in _hip.last_error()
    assert att(256, 256, 256, 256, 0, None, 3, 2, 4, 256, 64, 99, 256, None) == 1 and "precision" in _hip.last_error()
    assert att(256, 256, 256, 256, 0, None, 3, 2, 0, 256, 64, 1, 256, None) == 1 and "outside the cache" in _hip.last_error()
    assert att(256, 256, 256, 256, 0, None, 3, 2, 65, 256, 64, 1, 256, None) == 1 and "outside the cache" in _hip.last_error()
    assert att(256, 256, 256, 256, 0, None, 0, 2, 4, 256, 64, 1, 256, None) == 1 and "B/H" in _hip.last_error()
    assert att(256, 256, 256, 256, _hip.KX_F16C, None, 3, 2, 4, 256, 64, _hip.KX_PREC_BF16, 256, None) == 1
    assert att(264, 256, 256, 256, 0, None, 3, 2, 4, 256, 64, 1, 256, None) == 1 and "aligned" in _hip.last_error()
    ext = lib.kx_decoder_extend_ragged
    w = _hip.DecoderWeights()
    w.dim, w.heads, w.ffn, w.layers, w.vocab = 128, 2, 128, 1, 102
    #       tokens embed pos vocab max_pos shift x   B  T  positions tables + rows  logits ldt kc   vc  Tmax ws   bytes   prec err stream
    args = [256, 256, 256, 102, 32, 0, 256, 3, 4, 256] + [None] * 5 + [256, 0, 256, 256, 30, 256, 1 << 20, 1, 256, None]
    assert ext(None, *args) == 1 and "null pointer" in _hip.last_error()
    for k, what in ((0, "null pointer"), (1, "null pointer"), (2, "null pointer"), (6, "null pointer"), (9, "null pointer"),
                    (17, "cache missing"), (18, "cache missing"), (20, "null pointer"), (23, "null pointer")):
        bad = list(args)
        bad[k] = None
        assert ext(C.byref(w), *bad) == 1 and what in _hip.last_error(), (k, _hip.last_error())
    for prec in (99, _hip.KX_PREC_BF16X3, _hip.KX_PREC_F16):
        bad = list(args)
        bad[22] = prec
        assert ext(C.byref(w), *bad) == 1 and "bf16, fp32 and f16c" in _hip.last_error(), prec
    for k, v in ((7, 0), (8, 0), (8, 31), (19, 0)):                          # B, T = 0, T > Tmax, Tmax = 0
        bad = list(args)
        bad[k] = v
        assert ext(C.byref(w), *bad) == 1, (k, v)
    stale = _hip.DecoderWeights()
    stale.layer_bytes -= 8
    assert ext(C.byref(stale), *args) == 1 and "stale binding" in _hip.last_error()
