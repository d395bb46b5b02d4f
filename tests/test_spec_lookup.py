"""Prompt-lookup speculative decoding without a GPU: the contract (tests/spec_ref.py) reproduces plain greedy decoding whatever the
drafts are; the lookup rule on hand-written sequences; generate()'s refusals, which come before the device check; and the
library's new entry points, which validate before any launch."""
import ctypes as C
import itertools
import random
from pathlib import Path

import pytest
import torch

import spec_ref as R

ROOT = Path(__file__).resolve().parent.parent
SPEC_SYMBOLS = ("kx_spec_accept", "kx_attention_decode_block", "kx_decoder_decode_step_block")


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from kosmosx import _hip
    return _hip.load()


def _random_model(seed, vocab=5, context=2):
    """A deterministic next-token function over a small vocabulary: the token depends on the last ``context`` ids, so n-grams
    recur and the roll-out becomes periodic — the lookup accepts some drafts and misses others."""
    rng = random.Random(seed)
    table = {}

    def f(seq):
        key = tuple(seq[-context:])
        if key not in table:
            table[key] = rng.randrange(vocab)
        return table[key]
    return f


@pytest.mark.parametrize("D", [1, 3, 7, 15])
@pytest.mark.parametrize("ngram", [1, 2, 3])
def test_the_loop_reproduces_plain_greedy_decoding(D, ngram):
    accepted_more_than_one = False
    for seed, n, eos in itertools.product(range(12), (1, 2, 13, 32, 33), (None, 3)):
        rng = random.Random(1000 + seed)
        prompt = [rng.randrange(5) for _ in range(rng.randrange(1, 9))]
        f = _random_model(seed, context=1 + seed % 3)
        want = R.greedy(f, prompt, n, eos)
        got, emitted = R.run(f, prompt, n, D, ngram, eos)
        assert got == want, (seed, n, eos)
        assert sum(emitted) == len(got) and emitted[0] == 1 and all(1 <= e <= D + 1 for e in emitted)
        accepted_more_than_one |= max(emitted) > 1
    assert accepted_more_than_one                           # the cases do exercise acceptance


@pytest.mark.parametrize("D", [1, 3, 7, 15])
def test_perfect_and_adversarial_drafts_change_the_steps_not_the_tokens(D):
    K = D + 1
    for seed, n, eos in itertools.product(range(6), (1, 5, 16, 17, 40), (None, 2)):
        prompt = [seed % 5, (seed + 2) % 5, 1]
        f = _random_model(50 + seed, context=3)
        want = R.greedy(f, prompt, n, eos)
        padded = want + [0] * (n - len(want))
        got, emitted = R.run(f, prompt, n, D, 2, eos, draft_from=padded)                  # every draft right
        assert got == want
        assert len(emitted) == 1 + -(-(len(want) - 1) // K) and all(e == K for e in emitted[1:-1])
        got, emitted = R.run(f, prompt, n, D, 2, eos, draft_from=[(t + 1) % 5 for t in padded])   # every draft wrong
        assert got == want and emitted == [1] * len(want)


def test_max_new_tokens_is_never_exceeded():
    f = lambda seq: 4                                       # noqa: E731  (every lookup draft is right from the second token on)
    for n in (1, 2, 3, 4, 5, 9):
        got, emitted = R.run(f, [4, 4, 4], n, 3, 2, None)
        assert got == [4] * n and sum(emitted) == n


def test_the_lookup_rule_on_hand_written_sequences():
    # the most recent match wins: "1 2" occurs at 0 and at 3; the continuation is taken after the later one
    assert R.lookup([1, 2, 7, 1, 2, 8, 9, 1, 2], 2, 2) == [8, 9]
    # longer n is preferred: the 2-gram "5 1" at 0 beats the more recent 1-gram "1" at 4
    assert R.lookup([5, 1, 6, 0, 1, 7, 5, 1], 2, 2) == [6, 0]
    assert R.lookup([5, 1, 6, 0, 1, 7, 5, 1], 2, 1) == [7, 5]
    # ... and a sequence with no 2-gram match falls back to the 1-gram
    assert R.lookup([3, 1, 4, 2, 1], 3, 2) == [4, 2, 1]
    # the suffix never matches itself: its only occurrence is the suffix
    assert R.lookup([1, 2, 3, 4], 3, 2) == [4, 4, 4]       # no match: the last token repeated
    assert R.lookup([7], 2, 2) == [7, 7]                    # a single id has no n with len > n
    # wrap-around: the match ends one before the end, the continuation has period 1 ... and period 3
    assert R.lookup([9, 9], 4, 2) == [9, 9, 9, 9]
    assert R.lookup([1, 2, 3, 1], 7, 2) == [2, 3, 1, 2, 3, 1, 2]
    # overlapping occurrences: "4 4" in "4 4 4" matches at 0 (i <= len - n - 1 = 0)
    assert R.lookup([4, 4, 4], 2, 2) == [4, 4]


def test_accept_emit_and_draft_of_one_step():
    st = R.new_state([5, 6, 5, 6], prefill_len=10)
    e, nxt = R.step(st, None, [5], K=4, max_new=20, step_index=0)
    assert e == 1 and st["base"] == 10 and nxt == [5, 6, 5, 6] and st["out_src"] == [0]
    # two of three drafts confirmed: the picks 6, 5 and the correction 9 are emitted
    e, nxt = R.step(st, nxt, [6, 5, 9, 0], K=4, max_new=20, step_index=1)
    assert e == 3 and st["out"] == [5, 6, 5, 9] and st["base"] == 13 and st["out_src"] == [0, 4, 5, 6] and nxt[0] == 9
    # EOS inside the accepted run cuts it, inclusive
    e, nxt = R.step(st, [9, 1, 2, 3], [1, 2, 3, 4], K=4, max_new=20, step_index=2, eos=2, pad=0)
    assert e == 2 and st["out"][-2:] == [1, 2] and st["finished"] and nxt == [0, 0, 0, 0] and st["base"] == 15
    assert R.step(st, nxt, [1, 1, 1, 1], K=4, max_new=20, step_index=3, pad=0) == (0, [0, 0, 0, 0]) and st["base"] == 15
    # the budget cut
    st = R.new_state([1], prefill_len=1)
    R.step(st, None, [1], K=4, max_new=3, step_index=0)
    e, nxt = R.step(st, [1, 1, 1, 1], [1, 1, 1, 1], K=4, max_new=3, step_index=1)
    assert e == 2 and st["out"] == [1, 1, 1] and st["finished"]


def _models(batch=2):
    from helpers import tiny_config
    from kosmosx.model import Kosmos, KosmosLanguage
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    tok = torch.zeros(batch, 4, dtype=torch.long)
    img = torch.zeros(batch, 3, m.cfg.vit.image, m.cfg.vit.image)
    return [lambda **kw: lm.generate(tok, 4, **kw), lambda **kw: m.generate(tok, img, 4, **kw)]


REFUSED = [("do_sample", dict(do_sample=True)), ("temperature", dict(temperature=0.7)), ("top_k", dict(top_k=5)),
           ("top_p", dict(top_p=0.9)), ("repetition_penalty", dict(repetition_penalty=1.2)), ("num_beams", dict(num_beams=2)),
           ("prompt_lengths", dict(prompt_lengths=[3, 4])), ("sequence_ids", dict(sequence_ids=torch.arange(2))),
           ("no_repeat_ngram_size", dict(no_repeat_ngram_size=2)), ("bad_words_ids", dict(bad_words_ids=[[5]])),
           ("min_new_tokens", dict(min_new_tokens=2, eos_token_id=3)), ("stop_sequences", dict(stop_sequences=[[5, 6]])),
           ("prompt_lookup_num_tokens", dict(prompt_lookup_num_tokens=-1)), ("prompt_lookup_num_tokens", dict(prompt_lookup_num_tokens=2.0)),
           ("prompt_lookup_num_tokens", dict(prompt_lookup_num_tokens=True)),
           ("prompt_lookup_num_tokens", dict(prompt_lookup_num_tokens=8)),               # 2 sequences x 9 rows > 16
           ("max_matching_ngram_size", dict(max_matching_ngram_size=0)), ("max_matching_ngram_size", dict(max_matching_ngram_size=65)),
           ("eos_poll", dict(eos_poll=0)), ("eos_poll", dict(eos_poll=-1))]


@pytest.mark.parametrize("name,kw", REFUSED, ids=[f"{n}-{i}" for i, (n, _) in enumerate(REFUSED)])
def test_generate_refuses_what_prompt_lookup_does_not_offer(name, kw):
    """CPU tensors: the ValueError comes before the device check, hence before any launch, and names the argument."""
    for gen in _models():
        with pytest.raises(ValueError, match=name):
            gen(**{"prompt_lookup_num_tokens": 3, **kw})
    # the same call without the offending argument gets as far as the device check
    for gen in _models():
        with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
            gen(prompt_lookup_num_tokens=3)


def test_generate_refuses_acceptance_without_drafts_and_offers_logits_with_them():
    for gen in _models():
        with pytest.raises(ValueError, match="output_acceptance"):
            gen(output_acceptance=True)
        with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
            gen(prompt_lookup_num_tokens=7, output_logits=True, output_acceptance=True, max_matching_ngram_size=64)   # 2 x 8 = 16 rows
        with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
            gen()                                                                        # the defaults: as before
    for gen in _models(batch=1):
        with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
            gen(prompt_lookup_num_tokens=15)
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            gen(prompt_lookup_num_tokens=16)


def test_the_budget_counts_the_draft_rows():
    from kosmosx.model import KosmosLanguage
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    from kosmosx import generation
    generation.check_budget(lm.decoder, 4, 26)                                           # 30 rows: exactly full
    generation.check_budget(lm.decoder, 4, 23, spare=3)
    with pytest.raises(IndexError, match="draft rows"):
        generation.check_budget(lm.decoder, 4, 24, spare=3)


def test_the_library_exports_the_lookup_entry_points_within_abi_7(lib):
    from kosmosx import _hip
    for name in SPEC_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _hip.SYMBOLS
    assert lib.kx_version() == 7
    # kx_spec_args has no kx_struct_id (the id list is pinned at 13 entries): the call checks struct_bytes itself, so a mirror of
    # the right size gets past that check to the next one, and any other size is a stale binding
    assert _hip.SpecArgs not in _hip.STRUCT_IDS and lib.kx_struct_bytes(13) == 0
    a = _good_args()
    a.K = 1
    assert a.struct_bytes == C.sizeof(_hip.SpecArgs) and lib.kx_spec_accept(C.byref(a), None) == 1 and "K=1 " in _hip.last_error()
    for off in (-8, 8):
        a.struct_bytes = C.sizeof(_hip.SpecArgs) + off
        assert lib.kx_spec_accept(C.byref(a), None) == 1 and "stale binding" in _hip.last_error()
    header = (ROOT / "include" / "kosmosx_hip.h").read_text()
    assert "} kx_spec_args;" in header and "KX_STRUCT_COUNT = 13" in header
    assert _hip.SYMBOLS["kx_spec_accept"][1][0]._type_ is _hip.SpecArgs


def _good_args():
    from kosmosx import _hip
    a = _hip.SpecArgs()
    a.ngram_max, a.B, a.K, a.Kin = 2, 2, 4, 4
    for f in ("fed", "picked", "positions", "history", "hist_len", "out_tokens", "n_out", "finished", "next_tokens"):
        setattr(a, f, 256)
    a.prefill_len, a.hist_ld, a.out_ld, a.max_new, a.eos_id, a.pad_id, a.step = 5, 64, 16, 16, -1, 1, 1
    return a


BAD_ARGS = [("K=1 ", dict(K=1, Kin=1)), ("K=17 ", dict(K=17, Kin=17)), ("Kin=2 ", dict(Kin=2)), ("B=0 ", dict(B=0)),
            ("ngram_max=0 ", dict(ngram_max=0)), ("ngram_max=65 ", dict(ngram_max=65)), ("null pointer", dict(picked=None)),
            ("null pointer", dict(next_tokens=None)), ("null pointer", dict(history=None)), ("null fed", dict(fed=None)),
            ("out_ld", dict(out_ld=15)), ("max_new", dict(max_new=0)), ("prefill_len", dict(Kin=1, prefill_len=0)),
            ("step", dict(step=-1)), ("emitted_ld", dict(emitted=256, emitted_ld=1)), ("stale binding", dict(struct_bytes=8))]


@pytest.mark.parametrize("what,kw", BAD_ARGS, ids=[f"{w.strip()}-{i}" for i, (w, _) in enumerate(BAD_ARGS)])
def test_spec_accept_validates_before_any_launch(lib, what, kw):
    from kosmosx import _hip
    a = _good_args()
    for k, v in kw.items():
        setattr(a, k, v)
    assert lib.kx_spec_accept(C.byref(a), None) == 1
    assert what in _hip.last_error(), _hip.last_error()
    assert lib.kx_spec_accept(None, None) == 1 and "null args" in _hip.last_error()


def test_the_block_entry_points_validate_before_any_launch(lib):
    from kosmosx import _hip
    blk = lib.kx_attention_decode_block
    #       qkv  kc   vc   out  odt stats B  K  H  positions Tmax prec err stream
    assert blk(256, 256, 256, 256, 0, None, 1, 4, 2, None, 64, 1, 256, None) == 1 and "null positions" in _hip.last_error()
    assert blk(256, 256, 256, 256, 0, None, 1, 4, 2, 256, 64, 1, None, None) == 1 and "error_word" in _hip.last_error()
    for K in (0, 1, 17):
        assert blk(256, 256, 256, 256, 0, None, 1, K, 2, 256, 64, 1, 256, None) == 1 and f"K={K} " in _hip.last_error()
    assert blk(None, 256, 256, 256, 0, None, 1, 4, 2, 256, 64, 1, 256, None) == 1 and "null pointer" in _hip.last_error()
    assert blk(256, 256, 256, 256, 0, None, 0, 4, 2, 256, 64, 1, 256, None) == 1 and "B=0 " in _hip.last_error()
    assert blk(256, 256, 256, 256, 0, None, 1, 4, 2, 256, 0, 1, 256, None) == 1 and "Tmax=0 " in _hip.last_error()
    step = lib.kx_decoder_decode_step_block
    w = _hip.DecoderWeights()
    args = [256, 256, 256, 102, 32, 0, 256, 1, 4, 256] + [None] * 5 + [256, 256, 30, 256, 0, 256, 1 << 20, 1, 256, None]
    assert step(None, *args) == 1 and "null pointer" in _hip.last_error()
    for K in (1, 17):
        bad = list(args)
        bad[8] = K
        assert step(C.byref(w), *bad) == 1 and f"K={K} " in _hip.last_error()
    stale = _hip.DecoderWeights()
    stale.layer_bytes -= 8
    assert step(C.byref(stale), *args) == 1 and "stale binding" in _hip.last_error()
