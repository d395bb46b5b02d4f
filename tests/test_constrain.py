"""Constraints on generation, the parts that need no GPU: the NumPy restatement of the contract (tests/constrain_ref.py)
against the `transformers` logits processors; the C entry point's argument validation (no launch); the struct and ABI
bookkeeping; the refusals of ops.constrain_logits, check_constraint_args and both generate() methods."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import constrain_ref as CR

ROOT = Path(__file__).resolve().parent.parent


def _banned(scores):
    return set(np.nonzero(~np.isfinite(scores[0].numpy()))[0].tolist())


def test_reference_known_answers():
    row = np.zeros(12, dtype=np.float32)
    ban, fin = CR.constrain_row([5, 6, 7, 5, 6], row, ngram=3)
    assert set(np.nonzero(ban)[0]) == {7} and not fin
    ban, _ = CR.constrain_row([5, 6, 7, 5, 6], row, bad_words=[[5, 6, 2], [9], [6, 3]])
    assert set(np.nonzero(ban)[0]) == {2, 3, 9}
    ban, _ = CR.constrain_row([5, 6], row, new_tokens=1, min_new=2, eos_id=4)
    assert set(np.nonzero(ban)[0]) == {4}
    assert not CR.constrain_row([5, 6], row, new_tokens=2, min_new=2, eos_id=4)[0].any()
    # stop: a suffix after at least one new token; a stopped row gets no bans; ids outside [0, V) ban nothing
    ban, fin = CR.constrain_row([5, 6, 7], row, new_tokens=1, stop_sequences=[[6, 7]], ngram=1)
    assert fin and not ban.any()
    assert not CR.constrain_row([5, 6, 7], row, new_tokens=0, stop_sequences=[[6, 7]])[1]
    assert not CR.constrain_row([5, 6, 7], row, new_tokens=1, stop_sequences=[[5, 6]])[1]
    ban, _ = CR.constrain_row([-1, 17, 3], row, ngram=1)
    assert set(np.nonzero(ban)[0]) == {3}
    assert CR.logical([4, 8, 4, 4, 9, 2, 0], 6, prompt_width=4, prompt_len=2) == [4, 8, 9, 2]


def test_reference_equals_the_transformers_processors():
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(0)
    V, A = 12, 7                                                        # histories over 7 ids: matches are plentiful
    ngram_cases = ngram_banning = word_cases = planted = 0
    for N in (1, 2, 3, 5):
        for n in sorted({0, 1, N - 2, N - 1, N, 70} - {-1}):
            # 4 random draws, and where a ban is possible at all (n >= N) 8 more with a repeat planted: the tail's (N-1)-gram copied
            # to the front (a constant sequence where the two would overlap).  Random 4-grams over 7 ids rarely recur in 70 tokens.
            for rep in range(4 + (8 if n >= N else 0)):
                hist = rng.integers(0, A, n)
                if rep >= 4:
                    if n - N + 1 >= N - 1:
                        hist[:N - 1] = hist[n - N + 1:]
                    else:
                        hist[:] = hist[0]
                    planted += 1
                row = rng.standard_normal(V).astype(np.float32)
                ids, scores = torch.from_numpy(hist)[None], torch.from_numpy(row)[None]
                ban, fin = CR.constrain_row(hist, row, ngram=N)
                hf = lp.NoRepeatNGramLogitsProcessor(N)(ids, scores.clone())
                assert _banned(hf) == set(np.nonzero(ban)[0].tolist()) and not fin, (N, n, rep)
                ngram_cases += 1
                ngram_banning += bool(ban.any())
                # bad words: singles, and multi-token entries cut from the history's own tail so that some complete
                words = [[int(rng.integers(0, V))], [int(t) for t in rng.integers(0, A, 2)], [int(t) for t in rng.integers(0, A, 3)]]
                for m in (2, 3, 4):
                    if n >= m - 1:
                        words.append([int(t) for t in hist[n - (m - 1):]] + [int(rng.integers(0, V))])
                # The one corner where the contract and the processor part: a word of m = n + 1 ids whose first m - 1 ARE the whole
                # sequence.  The contract (n >= m - 1) bans its last id — the next token would complete it; the processor skips
                # every word longer than the context (m > n).  Such words are compared with the contract alone.
                whole = [w for w in words if len(w) == n + 1 and len(w) > 1]
                words = [w for w in words if w not in whole]
                ban, _ = CR.constrain_row(hist, row, bad_words=words)
                hf = lp.NoBadWordsLogitsProcessor(words, eos_token_id=None)(ids, scores.clone())
                assert _banned(hf) == set(np.nonzero(ban)[0].tolist()), (N, n, rep, words)
                for w in whole:
                    want = {w[-1]} if w[:-1] == [int(t) for t in hist] else set()
                    assert set(np.nonzero(CR.constrain_row(hist, row, bad_words=[w])[0])[0].tolist()) == want
                word_cases += 1
    assert ngram_cases == 4 * sum(len({0, 1, N - 2, N - 1, N, 70} - {-1}) for N in (1, 2, 3, 5)) + planted and word_cases == ngram_cases
    assert planted == 8 * 8                                             # (N, n) with n >= N: n = N and n = 70 for each N
    assert 2 * ngram_banning >= ngram_cases, (ngram_banning, ngram_cases)
    assert set(np.nonzero(CR.constrain_row([5, 6, 7, 5, 6], np.zeros(V, np.float32), ngram=3)[0])[0]) == {7}
    # minimum length: EOS is banned while fewer than min_new tokens follow the prompt
    P, eos, min_new = 4, 3, 3
    proc = lp.MinNewTokensLengthLogitsProcessor(P, min_new, eos)
    for g in range(6):
        hist = rng.integers(0, A, P + g)
        row = rng.standard_normal(V).astype(np.float32)
        hf = proc(torch.from_numpy(hist)[None], torch.from_numpy(row)[None].clone())
        ban, _ = CR.constrain_row(hist, row, new_tokens=g, min_new=min_new, eos_id=eos)
        assert _banned(hf) == set(np.nonzero(ban)[0].tolist()) == ({eos} if g < min_new else set())


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from kosmosx import _hip
    return _hip.load()


def _offsets(lengths):
    off = [0]
    for m in lengths:
        off.append(off[-1] + m)
    return (C.c_int32 * len(off))(*off)


def _good_args(keep):
    """Every pointer a fake non-null value: each call below must fail before anything is launched or read on the device."""
    from kosmosx import _hip
    a = _hip.ConstrainArgs()
    a.logits, a.ld, a.B, a.V = 256, 512, 2, 502
    a.history, a.hist_ld, a.hist_len = 256, 16, 8
    a.ngram, a.new_tokens, a.min_new, a.eos_id = 3, 2, 0, -1
    off = _offsets([1, 3])
    keep.append(off)
    a.bad_ids, a.bad_off, a.bad_off_host, a.n_bad = 256, 256, C.cast(off, C.c_void_p), 2
    return a


def test_entry_point_is_exported_and_validates_without_a_launch(lib):
    from kosmosx import _hip
    keep = []
    assert hasattr(lib, "kx_constrain_logits")
    assert lib.kx_constrain_logits(None, None) == 1 and "null" in _hip.last_error()
    for field, value, word in (("logits", 0, "logits"), ("V", 0, "V="), ("ld", 501, "ld="), ("B", 0, "B="), ("hist_len", -1, "hist_len"),
                               ("history", 0, "history"), ("new_tokens", -1, "new_tokens"), ("min_new", -1, "min_new"),
                               ("ngram", -1, "ngram"), ("bad_ids", 0, "bad_ids"), ("bad_off", 0, "bad_off"),
                               ("bad_off_host", 0, "bad_off_host"), ("n_bad", -1, "n_bad")):
        a = _good_args(keep)
        setattr(a, field, value)
        assert lib.kx_constrain_logits(C.byref(a), None) == 1, field
        assert word in _hip.last_error(), (field, _hip.last_error())
    a = _good_args(keep)
    a.hist_ld = a.hist_len                                                        # hist_ld <= hist_len: no room to append
    assert lib.kx_constrain_logits(C.byref(a), None) == 1 and "hist_ld" in _hip.last_error()
    a = _good_args(keep)
    a.prompt_lens, a.prompt_width = 256, 9                                        # the ragged form: prompt_width <= hist_len
    assert lib.kx_constrain_logits(C.byref(a), None) == 1 and "prompt_width" in _hip.last_error()
    a = _good_args(keep)
    a.struct_bytes -= 8
    assert lib.kx_constrain_logits(C.byref(a), None) == 1 and "stale binding" in _hip.last_error()
    # the limits: KX_ERR_UNSUPPORTED (4) with a message, before any launch
    a = _good_args(keep)
    a.ngram = 65
    assert lib.kx_constrain_logits(C.byref(a), None) == 4 and "ngram=65" in _hip.last_error()
    for table in ("bad", "stop"):
        for lengths, what in (([2, 65], "65 ids"), ([2, 0, 1], "0 ids")):
            a = _good_args(keep)
            off = _offsets(lengths)
            setattr(a, f"{table}_ids", 256)
            setattr(a, f"{table}_off", 256)
            setattr(a, f"{table}_off_host", C.cast(off, C.c_void_p))
            setattr(a, f"n_{table}", len(lengths))
            assert lib.kx_constrain_logits(C.byref(a), None) == 4, (table, lengths)
            assert what in _hip.last_error() and f"{table} sequence 1" in _hip.last_error(), _hip.last_error()
    a = _good_args(keep)
    off = (C.c_int32 * 3)(1, 2, 3)
    a.bad_off_host = C.cast(off, C.c_void_p)
    assert lib.kx_constrain_logits(C.byref(a), None) == 1 and "bad_off_host[0]" in _hip.last_error()


def test_struct_and_abi(lib):
    from kosmosx import _hip
    assert lib.kx_version() == 7 and _hip.ABI_VERSION == 7
    assert _hip.STRUCT_IDS.index(_hip.ConstrainArgs) == 12 and len(_hip.STRUCT_IDS) == 13
    assert lib.kx_struct_bytes(12) == C.sizeof(_hip.ConstrainArgs) > 0
    assert lib.kx_struct_bytes(13) == 0
    header = (ROOT / "include" / "kosmosx_hip.h").read_text()
    assert "KX_STRUCT_CONSTRAIN_ARGS = 12" in header and "KX_STRUCT_COUNT = 13" in header
    assert "#define KX_ABI_VERSION 7" in header
    assert _hip.SYMBOLS["kx_constrain_logits"][1][0]._type_ is _hip.ConstrainArgs


def _tiny_lm():
    from kosmosx.model import KosmosLanguage
    return KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=16).eval()


def test_ops_and_generate_refuse_cpu_tensors():
    from helpers import tiny_config
    from kosmosx import ops
    from kosmosx.model import Kosmos
    with pytest.raises(RuntimeError, match="not on a CUDA"):
        ops.constrain_logits(torch.zeros(2, 8), no_repeat_ngram_size=2)
    for name in ("bad_words", "stop_sequences"):                         # the CSR tables are ops.SequenceTable, not raw lists
        with pytest.raises(TypeError, match=f"constrain_logits: {name} must be an ops.SequenceTable"):
            ops.constrain_logits(torch.zeros(2, 8), **{name: [[1]]})
    kw = dict(no_repeat_ngram_size=2, bad_words_ids=[[3], [4, 5]], min_new_tokens=2, eos_token_id=7, stop_sequences=[[8, 9]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _tiny_lm().generate(torch.zeros(1, 4, dtype=torch.long), 4, **kw)
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate(torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, 3, m.cfg.vit.image, m.cfg.vit.image), 4, **kw)


BAD_ARGS = [
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=True), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=65), "no_repeat_ngram_size = 65 exceeds 64"),
    (dict(min_new_tokens=-2, eos_token_id=5), "min_new_tokens"),
    (dict(min_new_tokens=3), "min_new_tokens = 3 needs an eos_token_id"),
    (dict(bad_words_ids=5), "bad_words_ids must be a list"),
    (dict(bad_words_ids=[5]), r"bad_words_ids\[0\] must be a list"),
    (dict(bad_words_ids=[[5], []]), r"bad_words_ids\[1\] is empty"),
    (dict(bad_words_ids=[[5, 102]]), r"bad_words_ids\[0\] holds the id 102"),
    (dict(bad_words_ids=[[-1]]), r"bad_words_ids\[0\] holds the id -1"),
    (dict(bad_words_ids=[list(range(65))]), r"bad_words_ids\[0\] holds 65 ids"),
    (dict(stop_sequences="ab"), "stop_sequences must be a list"),
    (dict(stop_sequences=[[]]), r"stop_sequences\[0\] is empty"),
    (dict(stop_sequences=[[1.5]]), r"stop_sequences\[0\] must be a list of integer"),
    (dict(stop_sequences=[[3, 200]]), r"stop_sequences\[0\] holds the id 200"),
    (dict(stop_sequences=[[1] * 65]), r"stop_sequences\[0\] holds 65 ids"),
]
BEAM_ARGS = [
    (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size is not offered together with beam search"),
    (dict(bad_words_ids=[[3], [4, 5]]), "bad_words_ids with more than one id per entry is not offered together with beam search"),
    (dict(stop_sequences=[[4]]), "stop_sequences is not offered together with beam search"),
]


@pytest.mark.parametrize("kw,msg", BAD_ARGS)
def test_check_constraint_args_names_the_argument(kw, msg):
    from kosmosx import generation
    with pytest.raises(ValueError, match=msg):
        generation.check_constraint_args(102, **kw)
    with pytest.raises(ValueError, match=msg):                           # generate(): before the device check
        _tiny_lm().generate(torch.zeros(1, 4, dtype=torch.long), 4, **kw)


@pytest.mark.parametrize("kw,msg", BEAM_ARGS)
def test_beam_search_refuses_the_constraints_that_need_a_history(kw, msg):
    from helpers import tiny_config
    from kosmosx import generation
    from kosmosx.model import Kosmos
    with pytest.raises(ValueError, match=msg):
        generation.check_constraint_args(102, num_beams=3, **kw)
    generation.check_constraint_args(102, **kw)                          # fine without beams
    with pytest.raises(ValueError, match=msg):
        _tiny_lm().generate(torch.zeros(1, 4, dtype=torch.long), 4, num_beams=3, **kw)
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    with pytest.raises(ValueError, match=msg):
        m.generate(torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, 3, m.cfg.vit.image, m.cfg.vit.image), 4, num_beams=3, **kw)


def test_check_constraint_args_result():
    from kosmosx import generation
    assert generation.check_constraint_args(102) is None                 # the defaults: no launch
    assert generation.check_constraint_args(102, bad_words_ids=[], stop_sequences=[]) is None
    c = generation.check_constraint_args(102, min_new_tokens=2, eos_token_id=3, bad_words_ids=[[4]], num_beams=3)
    assert c["min_new"] == 2 and c["bad"] == [[4]] and not c["reads_history"] and c["every_step"]
    c = generation.check_constraint_args(102, min_new_tokens=2, eos_token_id=3)
    assert not c["reads_history"] and not c["every_step"]
    for kw in (dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[4, 5]]), dict(stop_sequences=[[6]])):
        assert generation.check_constraint_args(102, **kw)["reads_history"]
