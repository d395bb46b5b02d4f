"""Token-automaton constrained decoding without a GPU: the host class kosmosx.automaton.TokenAutomaton against the NumPy
restatement of the device contract (tests/automaton_ref.py), its constructors and refusals, generate()'s refusals around
``token_automaton`` / ``automaton_start`` (which come before the device check), the public signatures, and the library's new entry
point, which validates before any launch."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import automaton_ref as AR
from kosmosx import generation as G
from kosmosx.automaton import TokenAutomaton

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kosmosx_hip.h").read_text()
KX_ERR_INVALID_ARG, KX_ERR_UNSUPPORTED = 1, 4              # include/kosmosx_hip.h, kx_status


def test_from_choices_merges_shared_prefixes():
    a = TokenAutomaton.from_choices([[5, 6, 7], [5, 6, 9, 2], [8, 3]])
    # root, 5, 56, 567, 569, 5692, 8, 83: the prefix 5 6 is stored once
    assert a.num_states == 8 and a.start == 0 and a.default == [-1] * 8
    assert sorted(a.edges[0]) == [5, 8] and sorted(a.edges[a.walk([5, 6])]) == [7, 9]
    for choice in ([5, 6, 7], [5, 6, 9, 2], [8, 3]):
        end = a.walk(choice)
        assert end >= 0 and not a.edges[end] and not a.allowed(end, 12).any()          # a choice's node has no way out
        assert a.walk(choice + [5]) == -1
    assert a.walk([5, 7]) == -1 and a.walk([6]) == -1 and a.walk([]) == 0
    assert a.allowed(0, 12).nonzero()[0].tolist() == [5, 8]
    assert TokenAutomaton.from_choices([[4, 4], [4, 4]]).num_states == 3                # duplicates merge


def test_from_choices_with_a_prefix_choice_needs_an_eos():
    with pytest.raises(ValueError, match="choices\\[0\\] is a proper prefix"):
        TokenAutomaton.from_choices([[5, 6], [5, 6, 7]])
    a = TokenAutomaton.from_choices([[5, 6], [5, 6, 7]], eos_token_id=2)
    mid, end = a.walk([5, 6]), a.walk([5, 6, 7])
    assert sorted(a.edges[mid]) == [2, 7] and sorted(a.edges[end]) == [2]
    assert a.accepts_eos(mid, 2) and a.accepts_eos(end, 2) and not a.accepts_eos(0, 2) and not a.accepts_eos(-1, 2)
    last = a.walk([5, 6, 2])
    assert last == a.walk([5, 6, 7, 2]) and last >= 0 and not a.edges[last]              # one shared state with no way out
    assert a.walk([5, 6, 2, 2]) == -1


@pytest.mark.parametrize("field,make", [
    ("choices", lambda: TokenAutomaton.from_choices([])),
    ("choices\\[1\\] is empty", lambda: TokenAutomaton.from_choices([[3], []])),
    ("choices\\[0\\]", lambda: TokenAutomaton.from_choices([[3, -1]])),
    ("choices\\[0\\]", lambda: TokenAutomaton.from_choices([[3, 2.5]])),
    ("choices\\[0\\]", lambda: TokenAutomaton.from_choices([7])),
    ("eos_token_id", lambda: TokenAutomaton.from_choices([[3, 2]], eos_token_id=2)),
    ("eos_token_id", lambda: TokenAutomaton.from_choices([[3]], eos_token_id=-2)),
    ("ids", lambda: TokenAutomaton.from_allowed([])),
    ("ids", lambda: TokenAutomaton.from_allowed([3, -4])),
    ("ids", lambda: TokenAutomaton.from_allowed([3, "a"])),
    ("automata", lambda: TokenAutomaton.union([])),
    ("automata\\[1\\]", lambda: TokenAutomaton.union([TokenAutomaton.from_allowed([1]), {}])),
    ("edges", lambda: TokenAutomaton([])),
    ("edges", lambda: TokenAutomaton({3: 0})),
    ("edges\\[1\\]", lambda: TokenAutomaton([{3: 0}, [4]])),
    ("edges\\[0\\]", lambda: TokenAutomaton([{-3: 0}])),
    ("edges\\[0\\]", lambda: TokenAutomaton([{True: 0}])),
    ("edges\\[0\\]\\[3\\]", lambda: TokenAutomaton([{3: 1}])),
    ("edges\\[0\\]\\[3\\]", lambda: TokenAutomaton([{3: -2}])),
    ("edges\\[0\\]\\[3\\]", lambda: TokenAutomaton([{3: 0.0}])),
    ("default", lambda: TokenAutomaton([{3: 0}], default=[0, 0])),
    ("default\\[0\\]", lambda: TokenAutomaton([{3: 0}], default=[1])),
    ("default\\[0\\]", lambda: TokenAutomaton([{3: 0}], default=[None])),
    ("start", lambda: TokenAutomaton([{3: 0}], start=1)),
    ("start", lambda: TokenAutomaton([{3: 0}], start=-1)),
])
def test_constructor_refusals_name_the_field(field, make):
    with pytest.raises(ValueError, match=field):
        make()


def test_the_constructor_takes_none_and_minus_one_as_banned():
    a = TokenAutomaton([{3: None, 4: -1, 9: 1}, {}], default=[1, -1], start=0)
    assert a.edges[0] == {3: -1, 4: -1, 9: 1} and a.default == [1, -1] and a.max_token == 9
    assert a.allowed(0, 6).tolist() == [True, True, True, False, False, True]            # sparse deny; id 9 lies above V = 6
    assert a.walk([3]) == -1 and a.walk([0]) == 1 and a.walk([0, 0]) == -1 and a.walk([9], start=1) == -1
    a.check_vocab(10)
    with pytest.raises(ValueError, match="edges\\[0\\] lists the id 9"):
        a.check_vocab(9)
    off, tok, nxt, dflt = a.tables()
    assert all(t.dtype == np.int32 for t in (off, tok, nxt, dflt))
    assert off.tolist() == [0, 3, 3] and tok.tolist() == [3, 4, 9] and nxt.tolist() == [-1, -1, 1] and dflt.tolist() == [1, -1]


def test_from_allowed_and_union():
    w = TokenAutomaton.from_allowed([7, 3, 3, 11])
    assert w.num_states == 1 and w.edges[0] == {3: 0, 7: 0, 11: 0} and w.default == [-1]
    assert w.walk([3, 11, 7, 7]) == 0 and w.walk([3, 4]) == -1
    c = TokenAutomaton.from_choices([[3, 4], [5]], eos_token_id=2)
    d = TokenAutomaton([{1: 1}, {}], default=[-1, 0], start=1)
    u, starts = TokenAutomaton.union([w, c, d])
    assert u.num_states == w.num_states + c.num_states + d.num_states
    assert starts == [0, 1, 1 + c.num_states + 1] and u.start == starts[0]
    for a, st in zip((w, c, d), starts):                                                 # each copy walks like its original
        base = st - a.start
        for ids in ([3], [3, 4], [3, 4, 2], [5, 2], [7, 11], [1], [9, 1], [9, 9, 1, 4], [3, 4, 2, 2]):
            for k in range(len(ids) + 1):
                want = a.walk(ids[:k])
                got = u.walk(ids[:k], start=st)
                assert got == (want + base if want >= 0 else -1), (ids[:k], st)
                if want >= 0:
                    assert np.array_equal(u.allowed(got, 13), a.allowed(want, 13))
                    assert base <= got < base + a.num_states                             # the copies are disjoint


def _random_automaton(rng, S, V):
    edges, default = [], []
    for _ in range(S):
        ids = rng.choice(V, size=int(rng.integers(0, min(V, 6) + 1)), replace=False)
        edges.append({int(t): (None if rng.random() < 0.3 else int(rng.integers(0, S))) for t in ids})
        default.append(-1 if rng.random() < 0.5 else int(rng.integers(0, S)))
    return TokenAutomaton(edges, default, start=int(rng.integers(0, S)))


def test_walk_and_allowed_agree_with_the_reference_on_random_automata():
    rng = np.random.default_rng(0)
    dead = 0
    for trial in range(60):
        S, V = int(rng.integers(1, 7)), int(rng.integers(1, 12))
        a = _random_automaton(rng, S, V)
        tables = a.tables()
        s = a.start
        _, ban = AR.step_row(tables, s, None, False, V)
        assert np.array_equal(a.allowed(s, V), ~ban)
        assert AR.step_row(tables, s, V, False, V)[0] == -1                              # an id outside the vocabulary: rule 3
        ids = [int(t) for t in rng.integers(-1, V, 8)]                                   # (-1: no id at all)
        for k, t in enumerate(ids):
            s, ban = AR.step_row(tables, s, t, False, V)
            assert s == a.walk(ids[:k + 1]), (trial, ids[:k + 1])
            assert np.array_equal(a.allowed(s, V), ~ban)
            if s < 0:
                dead += 1
                break
    assert 10 < dead < 60                                                                # both outcomes occur


# ---- generate(): the refusals come before the device check ----

def _models(batch=2):
    from helpers import tiny_config
    from kosmosx.model import Kosmos, KosmosLanguage
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    tok = torch.zeros(batch, 4, dtype=torch.long)
    img = torch.zeros(batch, 3, m.cfg.vit.image, m.cfg.vit.image)
    session = [G.Session(model, {"batch": batch}, 20) for model in (lm, m)]
    return [(lambda **kw: lm.generate(tok, 4, **kw), lm.embed.weight.shape[0]),
            (lambda **kw: m.generate(tok, img, 4, **kw), m.embed.weight.shape[0]),
            (lambda **kw: session[0].generate(tok, 4, **kw), lm.embed.weight.shape[0]),
            (lambda **kw: session[1].generate(tok, 4, **kw), m.embed.weight.shape[0])]


AUTO = TokenAutomaton.from_choices([[3, 4], [5]], eos_token_id=2)                      # 5 states
REFUSED = [("token_automaton", lambda V: dict(token_automaton=[{3: 0}])),
           ("token_automaton", lambda V: dict(token_automaton="a*")),
           ("token_automaton", lambda V: dict(token_automaton=TokenAutomaton.from_allowed([3, V]))),
           ("automaton_start", lambda V: dict(token_automaton=AUTO, automaton_start=[0])),
           ("automaton_start", lambda V: dict(token_automaton=AUTO, automaton_start=[0, 1, 2])),
           ("automaton_start", lambda V: dict(token_automaton=AUTO, automaton_start=[0, 5])),
           ("automaton_start", lambda V: dict(token_automaton=AUTO, automaton_start=[-1, 0])),
           ("automaton_start", lambda V: dict(token_automaton=AUTO, automaton_start=torch.tensor([0, 5]))),
           ("automaton_start", lambda V: dict(token_automaton=AUTO, automaton_start=torch.tensor([0.0, 1.0]))),
           ("automaton_start", lambda V: dict(token_automaton=AUTO, automaton_start=3)),
           ("automaton_start", lambda V: dict(automaton_start=[0, 0]))]


@pytest.mark.parametrize("name,make", REFUSED, ids=[f"{n}-{i}" for i, (n, _) in enumerate(REFUSED)])
def test_generate_refuses_before_the_device_check(name, make):
    """CPU tensors, for Kosmos, KosmosLanguage and Session: the ValueError names its argument and comes before the device check."""
    for gen, V in _models():
        with pytest.raises(ValueError, match=name):
            gen(**make(V))


def test_generate_refuses_an_automaton_with_prompt_lookup():
    for gen, _ in _models()[:2]:                                                         # (a Session takes no prompt lookup)
        with pytest.raises(ValueError, match="token_automaton.*prompt_lookup_num_tokens"):
            gen(token_automaton=AUTO, prompt_lookup_num_tokens=2)


def test_generate_with_an_automaton_reaches_the_device_check():
    """The same calls without the offending argument get as far as the device refusal (before this feature: TypeError)."""
    for i, (gen, V) in enumerate(_models()):
        calls = [dict(token_automaton=AUTO), dict(token_automaton=AUTO, automaton_start=[0, 4]),
                 dict(token_automaton=AUTO, automaton_start=torch.tensor([1, 0], dtype=torch.int32), output_logits=True),
                 dict(token_automaton=TokenAutomaton.from_allowed([3, V - 1]), do_sample=True, eos_token_id=2, min_new_tokens=1)]
        if i < 2:
            calls += [dict(token_automaton=AUTO, num_beams=2, eos_token_id=2, num_return_sequences=2),
                      dict(token_automaton=AUTO, do_sample=True, num_return_sequences=3, automaton_start=[0, 1]),
                      dict(token_automaton=AUTO, return_session=True, prompt_lengths=[3, 4])]
        for kw in calls:
            with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
                gen(**kw)


def test_check_automaton_args_returns_the_start_states():
    assert G.check_automaton_args(102, 3) is None
    assert G.check_automaton_args(102, 3, token_automaton=AUTO) == [0, 0, 0]
    u, starts = TokenAutomaton.union([AUTO, TokenAutomaton.from_allowed([7])])
    assert G.check_automaton_args(102, 2, token_automaton=u, automaton_start=starts) == [0, 5]
    assert G.check_automaton_args(102, 2, token_automaton=u, automaton_start=torch.tensor(starts)) == [0, 5]


def test_the_signatures_carry_the_keyword_only_arguments():
    from kosmosx.model import Kosmos, KosmosLanguage
    for fn in (Kosmos.generate, KosmosLanguage.generate, G.Session.generate, G.loop_options, G.beam_loop):
        p = inspect.signature(fn).parameters
        for name in ("token_automaton", "automaton_start"):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is None, (fn.__qualname__, name)


# ---- the C ABI ----

@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from kosmosx import _hip
    return _hip.load()


def test_the_header_declares_the_entry_point_and_the_mirror_lists_its_fields_in_order(lib):
    from kosmosx import _hip
    assert "int kx_automaton_step(const kx_automaton_args* args, void* stream);" in HEADER
    assert hasattr(lib, "kx_automaton_step") and "kx_automaton_step" in _hip.SYMBOLS
    assert lib.kx_version() == 7 and "#define KX_ABI_VERSION 7" in HEADER               # appended within ABI 7
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"typedef struct \{([^{}]*)\}\s*kx_automaton_args\s*;", body, flags=re.S)
    assert m
    names = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        names += [re.findall(r"([A-Za-z_0-9]+)\s*$", part.replace("*", " ").strip())[0] for part in decl.split(",")]
    assert names == [f[0] for f in _hip.AutomatonArgs._fields_] and names[0] == "struct_bytes"
    assert _hip.AutomatonArgs().struct_bytes == C.sizeof(_hip.AutomatonArgs)


# the pointers are never followed: every refusal comes before the launch
GOOD = dict(logits=4096, ld=10, B=2, V=10, edge_off=4096, edge_tok=4096, edge_next=4096, default_next=4096, S=3, E=4,
            state_in=8192, B_in=2, state_out=8192 + 8, src_row=0, last_token=0, finished=0)
HOST_REFUSALS = [("logits", dict(logits=0), KX_ERR_INVALID_ARG), ("B", dict(B=0), KX_ERR_INVALID_ARG),
                 ("V", dict(V=0, ld=0), KX_ERR_INVALID_ARG), ("ld", dict(ld=9), KX_ERR_INVALID_ARG),
                 ("E", dict(E=-1), KX_ERR_INVALID_ARG), ("edge_off", dict(edge_off=0), KX_ERR_INVALID_ARG),
                 ("default_next", dict(default_next=0), KX_ERR_INVALID_ARG), ("edge_tok", dict(edge_tok=0), KX_ERR_INVALID_ARG),
                 ("edge_next", dict(edge_next=0), KX_ERR_INVALID_ARG), ("state_in", dict(state_in=0), KX_ERR_INVALID_ARG),
                 ("state_out", dict(state_out=0), KX_ERR_INVALID_ARG), ("B_in", dict(B_in=0), KX_ERR_INVALID_ARG),
                 ("B_in", dict(B_in=3), KX_ERR_INVALID_ARG),                            # differs from B without a src_row
                 ("overlap", dict(state_out=8192), KX_ERR_INVALID_ARG), ("overlap", dict(state_out=8192 + 4), KX_ERR_INVALID_ARG),
                 ("overlap", dict(state_out=8192 - 4), KX_ERR_INVALID_ARG),
                 ("V", dict(V=(1 << 23) + 1, ld=1 << 24), KX_ERR_UNSUPPORTED), ("S", dict(S=0), KX_ERR_UNSUPPORTED),
                 ("S", dict(S=1 << 31), KX_ERR_UNSUPPORTED), ("E", dict(E=1 << 31), KX_ERR_UNSUPPORTED),
                 ("workgroups", dict(B=(1 << 31) - 1, V=8192, ld=8192, B_in=(1 << 31) - 1, state_out=1 << 40), KX_ERR_UNSUPPORTED)]


def test_the_library_refuses_bad_arguments_before_any_launch(lib):
    from kosmosx import _hip
    for name, change, code in HOST_REFUSALS:
        a = _hip.AutomatonArgs()
        for k, v in dict(GOOD, **change).items():
            setattr(a, k, v)
        rc = lib.kx_automaton_step(C.byref(a), None)
        msg = _hip.last_error()
        assert rc == code and "kx_automaton_step" in msg and name in msg, (name, rc, msg)
    a = _hip.AutomatonArgs()
    a.struct_bytes -= 8
    assert lib.kx_automaton_step(C.byref(a), None) == KX_ERR_INVALID_ARG and "stale binding" in _hip.last_error()
    assert lib.kx_automaton_step(None, None) == KX_ERR_INVALID_ARG and "null args" in _hip.last_error()
