"""Truncation sampling without a GPU: the float64 reference (tests/truncate_ref.py) against `transformers`' TypicalLogitsWarper /
EpsilonLogitsWarper / EtaLogitsWarper, the near-threshold band the GPU tests rely on, generation.check_truncation_args and generate()'s
refusals (which come before the device check), the public signatures, and the new entry point of the library, which validates before
any launch."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import sampling_ref as R
import truncate_ref as TR
from kosmosx import generation as G

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kosmosx_hip.h").read_text()
KX_ERR_INVALID_ARG = 1                                      # include/kosmosx_hip.h, kx_status
NAMES = ("typical_p", "epsilon_cutoff", "eta_cutoff")
NAN = float("nan")
VS = [37, 502, 1500, 4099, 64007]
ROWS = 4


def rows(V, scale, n=ROWS):
    return (np.random.default_rng(V).standard_normal((n, V)) * scale).astype(np.float32)


# ---- the reference against transformers ----

def _warped(cls, value, x):
    from transformers.generation import logits_process as LP
    out = getattr(LP, cls)(value)(None, torch.from_numpy(x[None].copy()))
    return (out[0] > -np.inf).numpy()


CASES = [("TypicalLogitsWarper", "typical_p", (0.2, 0.9, 0.95)), ("EpsilonLogitsWarper", "epsilon_cutoff", (3e-4, 2e-3, 0.02)),
         ("EtaLogitsWarper", "eta_cutoff", (3e-4, 2e-3, 0.05))]


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("cls,name,values", CASES, ids=[c[1] for c in CASES])
def test_the_reference_keeps_what_the_transformers_warper_keeps(cls, name, values, V):
    """Gaussian rows at scales 1 and 3: equal kept sets except inside the near-threshold band — at most one differing element per
    row — and the band is small: at most 16 unsure elements per row."""
    differ = bound = 0
    for scale in (1.0, 3.0):
        for x in rows(V, scale):
            for v in values:
                keep, unsure, _ = TR.truncate_keep(x, x > -np.inf, **{name: v})
                theirs = _warped(cls, v, x)
                bad = np.nonzero((keep != theirs) & ~unsure)[0]
                assert bad.size == 0, (scale, v, bad[:8])
                n = int((keep != theirs).sum())
                assert n <= 1, (scale, v, n)
                differ += n
                assert unsure.sum() <= 16, (scale, v, int(unsure.sum()))
                assert keep.any() and keep.sum() <= V
                bound += int(keep.sum() < V)
    assert bound > 0                                          # the filter is real at this size
    print(f"{name} V={V}: {differ} differing elements (all unsure)")


@pytest.mark.parametrize("V", sorted(TR.SEEDS))
def test_the_band_conditions_hold_on_the_rows_the_gpu_tests_compare(V):
    """tests/test_sample_truncate_gpu.py compares kept sets on TR.case_rows under TR.ALONE / FRONTED / TOGETHER.  For the chosen
    seeds: no row has more than 16 unsure elements, and up to V = 1500 — where the sets are compared for equality — none beyond
    typical-p's threshold element itself (the last one it keeps), none at all without typical-p; no element lies within eps_p of
    top-p's mass boundary there either."""
    data = TR.case_rows(V)
    assert data.shape == ((8 if V < 64007 else 2), V)
    for case in TR.ALONE + TR.FRONTED + TR.TOGETHER:
        for b, (x, keep, unsure, stages, s0) in enumerate(TR.case_keep(data, case)):
            n = int(unsure.sum())
            assert n <= 16 and keep.any() and keep[unsure | keep].sum() > 0, (case, b, n)
            if V <= TR.EXACT_V:
                assert n <= int(case.get("typical_p", 1.0) < 1.0) and stages[0][unsure].all(), (case, b, np.nonzero(unsure)[0])
                p = case.get("top_p", 1.0)
                if p < 1.0:
                    k = min(case.get("top_k", 0), V - 1)
                    xs = R.scaled(data[b], case.get("temperature", 1.0), TR.case_history(data)[b] if case.get("history") else None,
                                  case.get("repetition_penalty", 1.0))
                    ahead = R.filter_row(xs, k, p)[1]
                    assert np.abs(ahead[np.isfinite(ahead)] - float(np.float32(p))).min() > TR.EPS_P, (case, b)


def test_each_filter_binds_in_some_row_and_is_slack_in_another():
    """Over the shared cases: every stage drops something in one row and nothing in another (so both branches are compared)."""
    binds, slack = set(), set()
    for V in sorted(TR.SEEDS):
        data = TR.case_rows(V)
        for case in TR.ALONE + TR.FRONTED + TR.TOGETHER:
            for x, keep, unsure, stages, s0 in TR.case_keep(data, case):
                before = s0
                for name, after in zip(NAMES, stages):
                    if name in case:
                        (binds if after.sum() < before.sum() else slack).add(name)
                    before = after
    assert binds == set(NAMES) and slack == set(NAMES), (binds, slack)


# ---- the reference on rows made by hand ----

def test_typical_p_can_drop_the_arg_max():
    """p = (0.6, 0.3, 0.05, 0.05): H = 0.967; |-log p - H| = 0.457, 0.237, 2.03, 2.03 — token 1 is the most typical one.  With
    t = 0.25 it alone stays (nothing lies ahead of it, 0.3 lies ahead of token 0); with t = 0.5 tokens 1 and 0; the two ties at
    0.05 stay or go together."""
    x = np.log(np.array([0.6, 0.3, 0.05, 0.05])).astype(np.float32)
    every = x > -np.inf
    assert TR.truncate_keep(x, every, typical_p=0.25)[0].tolist() == [False, True, False, False]
    assert TR.truncate_keep(x, every, typical_p=0.5)[0].tolist() == [True, True, False, False]
    assert TR.truncate_keep(x, every, typical_p=0.92)[0].tolist() == [True, True, True, True]
    assert TR.truncate_keep(x, every, typical_p=1.0)[0].tolist() == [True] * 4
    assert _warped("TypicalLogitsWarper", 0.25, x).tolist() == [False, True, False, False]


def test_eta_sees_what_epsilon_left():
    """p = (0.5, 0.3, 0.15, 0.04, 0.01), epsilon = 0.045, eta = 0.2.  Eta alone: H = 1.167, cut-off min(0.2, 0.447 e^-H = 0.139):
    token 2 (0.15) stays.  Epsilon alone drops tokens 3 and 4.  Eta behind epsilon works on (0.526, 0.316, 0.158): H = 0.993, the
    cut-off rises to 0.447 e^-H = 0.166 and token 2 goes too — fewer tokens than either filter alone would leave."""
    p = np.array([0.5, 0.3, 0.15, 0.04, 0.01])
    x = np.log(p).astype(np.float32)
    every = x > -np.inf
    assert TR.truncate_keep(x, every, epsilon_cutoff=0.045)[0].tolist() == [True, True, True, False, False]
    assert TR.truncate_keep(x, every, eta_cutoff=0.2)[0].tolist() == [True, True, True, False, False]
    assert TR.truncate_keep(x, every, epsilon_cutoff=0.045, eta_cutoff=0.2)[0].tolist() == [True, True, False, False, False]
    # (eta = 0.02 alone keeps token 3 at 0.04; behind epsilon it is gone for good: no stage gives back what an earlier one dropped)
    assert TR.truncate_keep(x, every, eta_cutoff=0.02)[0].tolist() == [True, True, True, True, False]
    assert TR.truncate_keep(x, every, epsilon_cutoff=0.045, eta_cutoff=0.02)[0].tolist() == [True, True, True, False, False]
    # a peaked row: the entropy term is the smaller one.  p = (0.97, 0.02, 0.01): H = 0.154, eta = 0.09 gives min(0.09, 0.3 * 0.857)
    q = np.log(np.array([0.97, 0.02, 0.01])).astype(np.float32)
    assert TR.truncate_keep(q, q > -np.inf, eta_cutoff=0.015)[0].tolist() == [True, True, False]
    # the arg max survives any cut-off
    flat = np.zeros(50, dtype=np.float32)
    flat[7] = 1e-3
    assert np.nonzero(TR.truncate_keep(flat, flat > -np.inf, epsilon_cutoff=0.5)[0])[0].tolist() == [7]
    # ... while eta on a flat row keeps everything: sqrt(0.9) exp(-log 50) = 0.019 lies below 1 / 50
    assert TR.truncate_keep(flat, flat > -np.inf, eta_cutoff=0.9)[0].all()


def test_plus_inf_ties_underflow_and_rows_without_a_candidate():
    x = np.array([1.0, np.inf, -3.0, np.inf, -np.inf], dtype=np.float32)
    s0 = x > -np.inf
    for kw in (dict(typical_p=0.5), dict(epsilon_cutoff=0.1), dict(eta_cutoff=0.1), dict(typical_p=0.9, epsilon_cutoff=0.1, eta_cutoff=0.1)):
        assert TR.truncate_keep(x, s0, **kw)[0].tolist() == [False, True, False, True, False], kw
    # everything but the maximum has underflowed 2^-40 relative to it: every stage keeps the maximum alone
    y = np.full(40, -200.0, dtype=np.float32)
    y[3] = 0.0
    for kw in (dict(typical_p=0.5), dict(epsilon_cutoff=1e-4), dict(eta_cutoff=1e-4)):
        assert np.nonzero(TR.truncate_keep(y, y > -np.inf, **kw)[0])[0].tolist() == [3], kw
    none = np.full(6, -np.inf, dtype=np.float32)
    keep, unsure, _ = TR.truncate_keep(none, none > -np.inf, typical_p=0.5, epsilon_cutoff=0.1, eta_cutoff=0.1)
    assert not keep.any() and not unsure.any()
    assert TR.sample_row(none, typical_p=0.5)["none"]


def test_the_stages_follow_top_k_top_p_and_min_p():
    x = rows(502, 3.0)[0]
    _, keep, _, stages, s0 = TR.sample_keep(x, temperature=0.9, top_k=40, top_p=0.95, min_p=0.01, typical_p=0.8, epsilon_cutoff=0.01,
                                            eta_cutoff=0.05)
    assert s0.sum() <= 40 and (stages[0] <= s0).all() and (stages[1] <= stages[0]).all() and (stages[2] <= stages[1]).all()
    assert np.array_equal(keep, stages[2]) and keep.any()
    ref = TR.sample_row(x, temperature=0.9, top_k=40, typical_p=0.8, seed=3, position=5, sequence_id=2)
    assert ref["keep"][ref["token"]] and TR.check_draw(ref["token"], ref) == "exact"
    plain = R.sample_row(x, temperature=0.9, top_k=40, seed=3, position=5, sequence_id=2)
    assert np.array_equal(plain["score"], ref["score"])       # the same Gumbel scores, another kept set


# ---- the argument checks ----

BAD = [("typical_p", dict(typical_p=0.0)), ("typical_p", dict(typical_p=-0.5)), ("typical_p", dict(typical_p=1.5)),
       ("typical_p", dict(typical_p=NAN)), ("typical_p", dict(typical_p=True)), ("typical_p", dict(typical_p="0.9")),
       ("typical_p", dict(typical_p=None)),
       ("epsilon_cutoff", dict(epsilon_cutoff=-1e-3)), ("epsilon_cutoff", dict(epsilon_cutoff=1.0)), ("epsilon_cutoff", dict(epsilon_cutoff=NAN)),
       ("epsilon_cutoff", dict(epsilon_cutoff=False)), ("epsilon_cutoff", dict(epsilon_cutoff=None)),
       ("eta_cutoff", dict(eta_cutoff=-1e-3)), ("eta_cutoff", dict(eta_cutoff=1.0)), ("eta_cutoff", dict(eta_cutoff=NAN)),
       ("eta_cutoff", dict(eta_cutoff=True)), ("eta_cutoff", dict(eta_cutoff="1e-3"))]
ON = [("typical_p", dict(typical_p=0.9)), ("epsilon_cutoff", dict(epsilon_cutoff=3e-4)), ("eta_cutoff", dict(eta_cutoff=2e-3))]


def test_check_truncation_args_returns_only_what_is_switched_on():
    assert G.check_truncation_args() == {}
    assert G.check_truncation_args(typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0) == {}
    assert G.check_truncation_args(typical_p=1, num_beams=4, prompt_lookup_num_tokens=2) == {}   # nothing of it is asked for
    assert G.check_truncation_args(typical_p=0.9) == dict(typical_p=0.9)
    assert G.check_truncation_args(epsilon_cutoff=3e-4, eta_cutoff=2e-3) == dict(epsilon_cutoff=3e-4, eta_cutoff=2e-3)


@pytest.mark.parametrize("name,kw", BAD, ids=[f"{n}-{i}" for i, (n, _) in enumerate(BAD)])
def test_check_truncation_args_refuses_bad_values_naming_the_argument(name, kw):
    with pytest.raises(ValueError, match=name):
        G.check_truncation_args(**kw)


@pytest.mark.parametrize("name,kw", ON, ids=[n for n, _ in ON])
def test_each_keyword_is_refused_with_beams_and_with_lookup(name, kw):
    with pytest.raises(ValueError, match=f"{name}.*num_beams"):
        G.check_truncation_args(num_beams=2, **kw)
    with pytest.raises(ValueError, match=f"{name}.*prompt_lookup_num_tokens"):
        G.check_truncation_args(prompt_lookup_num_tokens=3, **kw)


def _models(batch=2):
    from helpers import tiny_config
    from kosmosx.model import Kosmos, KosmosLanguage
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    tok = torch.zeros(batch, 4, dtype=torch.long)
    img = torch.zeros(batch, 3, m.cfg.vit.image, m.cfg.vit.image)
    session = [G.Session(model, {"batch": batch}, 20) for model in (lm, m)]
    return [(lambda **kw: lm.generate(tok, 4, **kw)), (lambda **kw: m.generate(tok, img, 4, **kw)),
            (lambda **kw: session[0].generate(tok, 4, **kw)), (lambda **kw: session[1].generate(tok, 4, **kw))]


def test_generate_refuses_before_the_device_check():
    """CPU tensors, for Kosmos, KosmosLanguage and Session: the ValueError names its argument and comes before the device check."""
    gens = _models()
    for name, kw in BAD[:1] + BAD[2:5] + BAD[7:9] + BAD[10:11] + BAD[12:14] + BAD[15:16]:
        for gen in gens:
            with pytest.raises(ValueError, match=name):
                gen(**kw)
    for name, kw in ON:
        for gen in gens[:2]:                                                                     # (a Session takes neither beams nor lookup)
            with pytest.raises(ValueError, match=f"{name}.*num_beams"):
                gen(num_beams=2, **kw)
            with pytest.raises(ValueError, match=f"{name}.*prompt_lookup_num_tokens"):
                gen(prompt_lookup_num_tokens=2, **kw)


def test_generate_with_the_keywords_reaches_the_device_check():
    """The same calls with good values get as far as the device refusal (before this feature: TypeError)."""
    for i, gen in enumerate(_models()):
        calls = [kw for _, kw in ON] + [dict(typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3, min_p=0.05, do_sample=True, top_k=5,
                                             output_logits=True)]
        if i < 2:
            calls += [dict(typical_p=0.5, do_sample=True, num_return_sequences=3), dict(eta_cutoff=1e-3, return_session=True, prompt_lengths=[3, 4]),
                      dict(epsilon_cutoff=1e-3, do_sample=True, guidance_scale=1.5, negative_prompt_ids=torch.zeros(2, 3, dtype=torch.long))]
        for kw in calls:
            with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
                gen(**kw)


def test_the_signatures_carry_the_keyword_only_arguments():
    from kosmosx import ops
    from kosmosx.model import Kosmos, KosmosLanguage
    for fn in (Kosmos.generate, KosmosLanguage.generate, G.Session.generate, G.loop_options, G.check_truncation_args, ops.sample_logits):
        p = inspect.signature(fn).parameters
        for name, default in zip(NAMES, (1.0, 0.0, 0.0)):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, (fn.__qualname__, name)


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


def test_the_header_declares_the_entry_point_and_the_mirror_lists_the_fields_in_order(lib):
    from kosmosx import _hip
    assert ("int kx_sample_logits_truncate(const kx_sample_args* args, int32_t* positions, int64_t advance, const kx_truncate_args* trunc, "
            "void* stream);" in HEADER)
    assert hasattr(lib, "kx_sample_logits_truncate") and "kx_sample_logits_truncate" in _hip.SYMBOLS
    assert lib.kx_version() == 7 and "#define KX_ABI_VERSION 7" in HEADER                        # appended within ABI 7
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"typedef struct \{([^{}]*)\}\s*kx_truncate_args\s*;", body, flags=re.S)
    assert m
    names = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        names += [re.findall(r"([A-Za-z_0-9]+)\s*$", part.replace("*", " ").strip())[0] for part in decl.split(",")]
    assert names == [f[0] for f in _hip.TruncateArgs._fields_] and names[0] == "struct_bytes"
    t = _hip.TruncateArgs()
    assert t.struct_bytes == C.sizeof(_hip.TruncateArgs) == 24
    assert (t.min_p, t.typical_p, t.epsilon_cutoff, t.eta_cutoff) == (0.0, 1.0, 0.0, 0.0)        # the defaults switch everything off
    assert "KX_STRUCT_COUNT = 13" in HEADER                                                      # no kx_struct_id value is appended
    for prop in ("64-bit INTEGER sum", "single IEEE operations", "no result depends on the order"):
        assert prop in HEADER, prop                                                              # the three fixed properties are written down


def test_the_entry_point_refuses_bad_arguments_before_any_launch(lib):
    """The pointers are never followed: every refusal comes before the launch."""
    from kosmosx import _hip
    a = _hip.SampleArgs()
    call = lib.kx_sample_logits_truncate
    assert call(C.byref(a), None, 0, None, None) == KX_ERR_INVALID_ARG and "null trunc" in _hip.last_error()
    t = _hip.TruncateArgs(typical_p=0.9)
    t.struct_bytes -= 4
    assert call(C.byref(a), None, 0, C.byref(t), None) == KX_ERR_INVALID_ARG and "stale binding" in _hip.last_error()
    for name, values in (("min_p", (-0.25, 1.5, NAN)), ("typical_p", (0.0, -1.0, 1.5, NAN)), ("epsilon_cutoff", (-1e-3, 1.0, NAN)),
                         ("eta_cutoff", (-1e-3, 1.0, 2.0, NAN))):
        for v in values:
            t = _hip.TruncateArgs(**{name: v})
            rc = call(C.byref(a), None, 0, C.byref(t), None)
            assert rc == KX_ERR_INVALID_ARG and f"kx_sample_logits_truncate: {name}" in _hip.last_error(), (name, v, rc, _hip.last_error())
    t = _hip.TruncateArgs(eta_cutoff=1e-3)
    assert call(C.byref(a), 4096, -1, C.byref(t), None) == KX_ERR_INVALID_ARG and "advance" in _hip.last_error()
    for kw in (dict(), dict(min_p=0.5), dict(typical_p=0.9), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3)):
        t = _hip.TruncateArgs(**kw)                                                              # (the sampler's own checks come next)
        assert call(None, None, 0, C.byref(t), None) == KX_ERR_INVALID_ARG and "null args" in _hip.last_error()
        stale = _hip.SampleArgs()
        stale.struct_bytes -= 8
        assert call(C.byref(stale), None, 0, C.byref(t), None) == KX_ERR_INVALID_ARG and "stale binding" in _hip.last_error()
        assert call(C.byref(a), None, 0, C.byref(t), None) == KX_ERR_INVALID_ARG and "null logits" in _hip.last_error()
