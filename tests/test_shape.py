"""Logit shaping without a GPU: generation.check_shape_args and generate()'s refusals around ``logit_bias`` / ``presence_penalty`` /
``frequency_penalty`` / ``min_p`` (which come before the device check), the public signatures, the two new entry points of the
library — both validate before any launch — and the NumPy reference's min-p set against the sentence it restates."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import shape_ref as SR
from kosmosx import generation as G

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kosmosx_hip.h").read_text()
KX_ERR_INVALID_ARG, KX_ERR_UNSUPPORTED = 1, 4              # include/kosmosx_hip.h, kx_status
NAMES = ("logit_bias", "presence_penalty", "frequency_penalty", "min_p")
INF, NAN = float("inf"), float("nan")


def test_check_shape_args_returns_none_at_the_defaults():
    assert G.check_shape_args(102, 3) is None
    assert G.check_shape_args(102, 3, logit_bias=None, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0) is None
    assert G.check_shape_args(102, 3, logit_bias={}, presence_penalty=0, frequency_penalty=-0.0) is None
    assert G.check_shape_args(102, 3, num_beams=4, prompt_lookup_num_tokens=2) is None           # nothing of it is asked for


def test_check_shape_args_returns_sorted_per_row_biases_and_the_floats():
    got = G.check_shape_args(102, 2, logit_bias={7: 1.5, 3: -INF}, frequency_penalty=0.25)
    assert got["bias"] == [[(3, -INF), (7, 1.5)]] * 2 and got["launch"]
    assert (got["frequency"], got["presence"], got["min_p"]) == (0.25, 0.0, 0.0)
    got = G.check_shape_args(102, 2, logit_bias=[{101: 2}, {}], presence_penalty=-1)
    assert got["bias"] == [[(101, 2.0)], []] and got["presence"] == -1.0 and got["launch"]
    got = G.check_shape_args(102, 2, min_p=0.25)
    assert got["bias"] is None and got["min_p"] == 0.25 and not got["launch"]                    # min_p alone: no shaping launch
    assert G.check_shape_args(102, 2, min_p=1)["min_p"] == 1.0


BAD = [("logit_bias", dict(logit_bias={3: INF})), ("logit_bias", dict(logit_bias={3: NAN})),
       ("logit_bias", dict(logit_bias={3: 1e39})),
       ("logit_bias", dict(logit_bias={1000000: 1.0})), ("logit_bias", dict(logit_bias={-1: 1.0})),
       ("logit_bias", dict(logit_bias=[{3: 1.0}])), ("logit_bias", dict(logit_bias=[{3: 1.0}] * 3)),
       ("logit_bias", dict(logit_bias=[{3: 1.0}, [3, 1.0]])), ("logit_bias", dict(logit_bias={"a": 1.0})),
       ("logit_bias", dict(logit_bias={3.5: 1.0})),
       ("min_p", dict(min_p=-0.1)), ("min_p", dict(min_p=1.5)), ("min_p", dict(min_p=NAN)), ("min_p", dict(min_p="0.1")),
       ("presence_penalty", dict(presence_penalty=INF)), ("presence_penalty", dict(presence_penalty=NAN)),
       ("frequency_penalty", dict(frequency_penalty=-INF)), ("frequency_penalty", dict(frequency_penalty=NAN)),
       ("frequency_penalty", dict(frequency_penalty=1e39)), ("frequency_penalty", dict(frequency_penalty=None))]
ON = [("logit_bias", dict(logit_bias={3: 1.0})), ("presence_penalty", dict(presence_penalty=0.5)),
      ("frequency_penalty", dict(frequency_penalty=0.5)), ("min_p", dict(min_p=0.1))]


@pytest.mark.parametrize("name,kw", BAD, ids=[f"{n}-{i}" for i, (n, _) in enumerate(BAD)])
def test_check_shape_args_refuses_bad_values_naming_the_argument(name, kw):
    with pytest.raises(ValueError, match=name):
        G.check_shape_args(102, 2, **kw)


def test_a_duplicate_id_is_refused():
    class Twice(dict):                                                                           # (3 and np.int64(3) are one id)
        def items(self):
            return [(3, 1.0), (np.int64(3), 2.0)]
    with pytest.raises(ValueError, match="logit_bias.*twice"):
        G.check_shape_args(102, 2, logit_bias=Twice())


@pytest.mark.parametrize("name,kw", ON, ids=[n for n, _ in ON])
def test_each_keyword_is_refused_with_beams_and_with_lookup(name, kw):
    with pytest.raises(ValueError, match=f"{name}.*num_beams"):
        G.check_shape_args(102, 2, num_beams=2, **kw)
    with pytest.raises(ValueError, match=f"{name}.*prompt_lookup_num_tokens"):
        G.check_shape_args(102, 2, prompt_lookup_num_tokens=3, **kw)


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
    for name, kw in BAD[:2] + BAD[3:4] + BAD[5:6] + BAD[10:12] + BAD[14:15] + BAD[17:18]:
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
        calls = [kw for _, kw in ON] + [dict(logit_bias=[{3: -INF}, {4: 2.0, 0: -1.0}], presence_penalty=-0.5, frequency_penalty=0.3,
                                             min_p=0.05, do_sample=True, top_k=5, output_logits=True)]
        if i < 2:
            calls += [dict(min_p=0.5, do_sample=True, num_return_sequences=3, logit_bias=[{1: 1.0}, {}]),
                      dict(frequency_penalty=1.0, return_session=True, prompt_lengths=[3, 4])]
        for kw in calls:
            with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
                gen(**kw)


def test_the_signatures_carry_the_keyword_only_arguments():
    from kosmosx.model import Kosmos, KosmosLanguage
    for fn in (Kosmos.generate, KosmosLanguage.generate, G.Session.generate, G.loop_options):
        p = inspect.signature(fn).parameters
        for name, default in zip(NAMES, (None, 0.0, 0.0, 0.0)):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__qualname__, name)
            assert p[name].default is None if default is None else p[name].default == 0.0, (fn.__qualname__, name)
    p = inspect.signature(G.check_shape_args).parameters
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in NAMES)
    from kosmosx import ops
    assert inspect.signature(ops.sample_logits).parameters["min_p"].default == 0.0


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


def test_the_header_declares_both_entry_points_and_the_mirror_lists_the_fields_in_order(lib):
    from kosmosx import _hip
    assert "int kx_shape_logits(const kx_shape_args* args, void* stream);" in HEADER
    assert ("int kx_sample_logits_min_p(const kx_sample_args* args, int32_t* positions, int64_t advance, float min_p, void* stream);"
            in HEADER)
    for name in ("kx_shape_logits", "kx_sample_logits_min_p"):
        assert hasattr(lib, name) and name in _hip.SYMBOLS
    assert lib.kx_version() == 7 and "#define KX_ABI_VERSION 7" in HEADER                        # appended within ABI 7
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"typedef struct \{([^{}]*)\}\s*kx_shape_args\s*;", body, flags=re.S)
    assert m
    names = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        names += [re.findall(r"([A-Za-z_0-9]+)\s*$", part.replace("*", " ").strip())[0] for part in decl.split(",")]
    assert names == [f[0] for f in _hip.ShapeArgs._fields_] and names[0] == "struct_bytes"
    assert _hip.ShapeArgs().struct_bytes == C.sizeof(_hip.ShapeArgs)
    assert "KX_STRUCT_COUNT = 13" in HEADER                                                      # no kx_struct_id value is appended


# the pointers are never followed: every refusal comes before the launch
GOOD = dict(logits=4096, ld=10, B=2, V=10, bias_off=4096, bias_ids=4096, bias_val=4096, n_bias=3, counts=8192, frequency=0.5,
            presence=0.25, last_token=0, finished=0)
HOST_REFUSALS = [("logits", dict(logits=0), KX_ERR_INVALID_ARG), ("B", dict(B=0), KX_ERR_INVALID_ARG),
                 ("V", dict(V=0, ld=0), KX_ERR_INVALID_ARG), ("ld", dict(ld=9), KX_ERR_INVALID_ARG),
                 ("n_bias", dict(n_bias=-1), KX_ERR_INVALID_ARG), ("bias_off", dict(bias_off=0), KX_ERR_INVALID_ARG),
                 ("bias_ids", dict(bias_ids=0), KX_ERR_INVALID_ARG), ("bias_val", dict(bias_val=0), KX_ERR_INVALID_ARG),
                 ("frequency", dict(frequency=INF), KX_ERR_INVALID_ARG), ("frequency", dict(frequency=NAN), KX_ERR_INVALID_ARG),
                 ("presence", dict(presence=-INF), KX_ERR_INVALID_ARG), ("presence", dict(presence=NAN), KX_ERR_INVALID_ARG),
                 ("counts", dict(counts=0), KX_ERR_INVALID_ARG),
                 ("nothing to shape", dict(counts=0, frequency=0.0, presence=0.0, bias_off=0, n_bias=0), KX_ERR_INVALID_ARG),
                 ("V", dict(V=(1 << 23) + 1, ld=1 << 24), KX_ERR_UNSUPPORTED), ("n_bias", dict(n_bias=1 << 31), KX_ERR_UNSUPPORTED),
                 ("workgroups", dict(B=(1 << 31) - 1, V=8192, ld=8192), KX_ERR_UNSUPPORTED)]


def test_the_library_refuses_bad_shape_arguments_before_any_launch(lib):
    from kosmosx import _hip
    for name, change, code in HOST_REFUSALS:
        a = _hip.ShapeArgs()
        for k, v in dict(GOOD, **change).items():
            setattr(a, k, v)
        rc = lib.kx_shape_logits(C.byref(a), None)
        msg = _hip.last_error()
        assert rc == code and "kx_shape_logits" in msg and name in msg, (name, rc, msg)
    a = _hip.ShapeArgs()
    a.struct_bytes -= 8
    assert lib.kx_shape_logits(C.byref(a), None) == KX_ERR_INVALID_ARG and "stale binding" in _hip.last_error()
    assert lib.kx_shape_logits(None, None) == KX_ERR_INVALID_ARG and "null args" in _hip.last_error()


def test_the_min_p_entry_point_refuses_bad_arguments_before_any_launch(lib):
    from kosmosx import _hip
    for m in (0.0, 0.5, 1.0):                                                                    # (0: the old launch's own checks)
        assert lib.kx_sample_logits_min_p(None, None, 0, m, None) == KX_ERR_INVALID_ARG and "null args" in _hip.last_error()
    a = _hip.SampleArgs()
    a.struct_bytes -= 8
    assert lib.kx_sample_logits_min_p(C.byref(a), None, 0, 0.5, None) == KX_ERR_INVALID_ARG and "stale binding" in _hip.last_error()
    a = _hip.SampleArgs()
    for m in (-0.25, 1.5, NAN):
        rc = lib.kx_sample_logits_min_p(C.byref(a), None, 0, m, None)
        assert rc == KX_ERR_INVALID_ARG and "kx_sample_logits_min_p: min_p" in _hip.last_error(), (m, rc, _hip.last_error())
    assert lib.kx_sample_logits_min_p(C.byref(a), 4096, -1, 0.5, None) == KX_ERR_INVALID_ARG and "advance" in _hip.last_error()


# ---- the reference ----

def test_the_reference_min_p_set_equals_the_float64_sentence():
    """p_i >= m * p_max after top-k and top-p, in float64, on rows whose x_i all lie at least 1e-4 away from x_max + log m (so that
    the fp32 rounding of the threshold decides nothing)."""
    rng = np.random.default_rng(3)
    cases = kept_fewer = 0
    for trial in range(60):
        V = int(rng.choice([5, 37, 300]))
        logits = (rng.standard_normal(V) * rng.choice([0.5, 2.0, 6.0])).astype(np.float32)
        if trial % 7 == 0:
            logits[rng.integers(0, V, 2)] = -np.inf
        T = float(rng.choice([0.7, 1.0, 1.3]))
        k, p, m = int(rng.choice([0, 3, 20])), float(rng.choice([1.0, 0.9, 0.6])), float(rng.choice([0.02, 0.1, 0.3, 0.7]))
        x, keep = SR.sample_keep(logits, temperature=T, top_k=k, top_p=p, min_p=m)
        thr = float(x.max()) + float(SR.log_min_p(m))
        if np.abs(x[x > -np.inf].astype(np.float64) - thr).min() < 1e-4:
            continue
        cases += 1
        want = SR.min_p_keep_float64(x, k, p, m)
        assert np.array_equal(keep, want), (trial, V, T, k, p, m)
        assert keep[int(np.argmax(x))]
        kept_fewer += int(keep.sum() < SR.sample_keep(logits, temperature=T, top_k=k, top_p=p)[1].sum())
    assert cases > 40 and kept_fewer > 10                                                        # min-p is the binding filter in many of them


def test_the_reference_keeps_the_transformers_order_and_the_ties():
    row = np.log(np.array([0.6, 0.3, 0.05, 0.05])).astype(np.float32)
    assert SR.sample_keep(row, top_p=0.65, min_p=0.1)[1].tolist() == [True, True, False, False]
    # (min-p first would renormalise top-p over {0, 1, (2, 3 dropped)}: 0.6 / 0.9 = 0.667 >= 0.65 keeps token 0 alone)
    ties = np.array([1.0, 3.0, 3.0, 2.9999998, -np.inf], dtype=np.float32)
    assert SR.sample_keep(ties, min_p=1.0)[1].tolist() == [False, True, True, False, False]
    assert SR.sample_keep(ties, min_p=0.0)[1].tolist() == [True, True, True, True, False]
