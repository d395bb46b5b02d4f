"""Classifier-free guidance without a GPU: generation.check_guidance_args and generate()'s refusals around ``guidance_scale`` /
``negative_prompt_ids`` / ``negative_prompt_lengths`` / ``negative_images`` (which come before the device check), the public
signatures, the new entry point of the library — it validates before any launch — and the NumPy reference against an independent
statement of the rule."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import guidance_ref as GR
from kosmosx import generation as G

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kosmosx_hip.h").read_text()
KX_ERR_INVALID_ARG, KX_ERR_UNSUPPORTED = 1, 4              # include/kosmosx_hip.h, kx_status
INF, NAN = float("inf"), float("nan")
NEG = torch.zeros(2, 3, dtype=torch.long)


def test_check_guidance_args_returns_none_at_the_defaults():
    assert G.check_guidance_args(3) is None
    assert G.check_guidance_args(3, guidance_scale=1.0, negative_prompt_ids=None, negative_prompt_lengths=None, negative_images=None) is None
    assert G.check_guidance_args(3, guidance_scale=1, multimodal=True, min_len=2) is None
    # nothing of it is asked for: the other features are not refused
    assert G.check_guidance_args(3, num_beams=4, prompt_lookup_num_tokens=2, num_return_sequences=3, return_session=True) is None


def test_check_guidance_args_returns_the_scale_and_the_host_lengths():
    assert G.check_guidance_args(2, guidance_scale=1.5) == dict(scale=1.5, lengths=None)         # the text model's default negative
    assert G.check_guidance_args(2, guidance_scale=0, negative_prompt_ids=NEG) == dict(scale=0.0, lengths=None)
    assert G.check_guidance_args(2, guidance_scale=-0.5, negative_prompt_ids=NEG, negative_prompt_lengths=[3, 1]) == dict(
        scale=-0.5, lengths=[3, 1])
    got = G.check_guidance_args(2, guidance_scale=3.0, negative_prompt_ids=NEG, negative_prompt_lengths=torch.tensor([2, 3]))
    assert got == dict(scale=3.0, lengths=None)                                                  # a tensor is resolved after the device check
    img = torch.zeros(2, 3, 8, 8)
    assert G.check_guidance_args(2, guidance_scale=2.0, negative_images=img, multimodal=True, min_len=2)["scale"] == 2.0
    assert G.check_guidance_args(2, guidance_scale=2.0, negative_prompt_ids=NEG, multimodal=True, min_len=2)["scale"] == 2.0


BAD = [("guidance_scale", dict(guidance_scale=INF)), ("guidance_scale", dict(guidance_scale=-INF)),
       ("guidance_scale", dict(guidance_scale=NAN)), ("guidance_scale", dict(guidance_scale="1.5")),
       ("guidance_scale", dict(guidance_scale=None)), ("guidance_scale", dict(guidance_scale=1e39)),
       ("guidance_scale", dict(guidance_scale=True)),
       # a negative argument without a scale
       ("negative_prompt_ids", dict(negative_prompt_ids=NEG)),
       ("negative_prompt_ids", dict(guidance_scale=1.0, negative_prompt_ids=NEG)),
       ("negative_prompt_lengths", dict(negative_prompt_lengths=[1, 1])),
       ("negative_images", dict(negative_images=torch.zeros(2, 3, 8, 8), multimodal=True)),
       # wrong batch, too short, wrong dtype, no tensor, wrong rank
       ("negative_prompt_ids", dict(guidance_scale=2.0, negative_prompt_ids=torch.zeros(3, 3, dtype=torch.long))),
       ("negative_prompt_ids", dict(guidance_scale=2.0, negative_prompt_ids=torch.zeros(2, 0, dtype=torch.long))),
       ("negative_prompt_ids", dict(guidance_scale=2.0, negative_prompt_ids=torch.zeros(2, 1, dtype=torch.long), min_len=2, multimodal=True)),
       ("negative_prompt_ids", dict(guidance_scale=2.0, negative_prompt_ids=torch.zeros(2, 3))),
       ("negative_prompt_ids", dict(guidance_scale=2.0, negative_prompt_ids=torch.zeros(2, 3, dtype=torch.bool))),
       ("negative_prompt_ids", dict(guidance_scale=2.0, negative_prompt_ids=[[1, 2, 3], [4, 5, 6]])),
       ("negative_prompt_ids", dict(guidance_scale=2.0, negative_prompt_ids=torch.zeros(6, dtype=torch.long))),
       # bad lengths
       ("negative_prompt_lengths", dict(guidance_scale=2.0, negative_prompt_lengths=[1, 1])),   # without the ids
       ("negative_prompt_lengths", dict(guidance_scale=2.0, negative_prompt_ids=NEG, negative_prompt_lengths=[1])),
       ("negative_prompt_lengths", dict(guidance_scale=2.0, negative_prompt_ids=NEG, negative_prompt_lengths=[0, 1])),
       ("negative_prompt_lengths", dict(guidance_scale=2.0, negative_prompt_ids=NEG, negative_prompt_lengths=[4, 1])),
       ("negative_prompt_lengths", dict(guidance_scale=2.0, negative_prompt_ids=NEG, negative_prompt_lengths=[1.5, 1])),
       ("negative_prompt_lengths", dict(guidance_scale=2.0, negative_prompt_ids=NEG, negative_prompt_lengths=7)),
       ("negative_prompt_lengths", dict(guidance_scale=2.0, negative_prompt_ids=NEG, negative_prompt_lengths=torch.tensor([1.0, 2.0]))),
       ("negative_prompt_lengths", dict(guidance_scale=2.0, negative_prompt_ids=NEG, negative_prompt_lengths=torch.tensor([1, 2, 3]))),
       ("negative_prompt_lengths", dict(guidance_scale=2.0, negative_prompt_ids=NEG, negative_prompt_lengths=[1, 2], min_len=2, multimodal=True)),
       # the multimodal model
       ("negative_prompt_ids.*negative_images", dict(guidance_scale=2.0, multimodal=True, min_len=2)),
       ("negative_images", dict(guidance_scale=2.0, negative_images=torch.zeros(3, 3, 8, 8), multimodal=True)),
       ("negative_images", dict(guidance_scale=2.0, negative_images=torch.zeros(2, 3, 8, 8, dtype=torch.long), multimodal=True)),
       ("negative_images", dict(guidance_scale=2.0, negative_images=torch.zeros(2, 3, 8, 8)))]  # the text model takes none


@pytest.mark.parametrize("name,kw", BAD, ids=[f"{n.split('.')[0]}-{i}" for i, (n, _) in enumerate(BAD)])
def test_check_guidance_args_refuses_bad_values_naming_the_argument(name, kw):
    with pytest.raises(ValueError, match=name):
        G.check_guidance_args(2, **kw)


REFUSED = [("num_beams", dict(num_beams=2)), ("prompt_lookup_num_tokens", dict(prompt_lookup_num_tokens=2)),
           ("num_return_sequences", dict(num_return_sequences=2, do_sample=True)), ("return_session", dict(return_session=True))]


@pytest.mark.parametrize("other,kw", REFUSED, ids=[n for n, _ in REFUSED])
def test_guidance_is_refused_with_beams_lookup_parallel_sampling_and_sessions(other, kw):
    kw = {k: v for k, v in kw.items() if k != "do_sample"}
    with pytest.raises(ValueError, match=f"guidance_scale.*{other}"):
        G.check_guidance_args(2, guidance_scale=1.5, negative_prompt_ids=NEG, **kw)


def _models(batch=2):
    from helpers import tiny_config
    from kosmosx.model import Kosmos, KosmosLanguage
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    tok = torch.zeros(batch, 4, dtype=torch.long)
    img = torch.zeros(batch, 3, m.cfg.vit.image, m.cfg.vit.image)
    return (lambda **kw: lm.generate(tok, 4, **kw)), (lambda **kw: m.generate(tok, img, 4, **kw)), img


def test_generate_refuses_before_the_device_check():
    """CPU tensors, for Kosmos and KosmosLanguage: the ValueError names its argument and comes before the device check."""
    lm, mm, img = _models()
    for gen in (lm, mm):
        for other, kw in REFUSED:
            with pytest.raises(ValueError, match=f"guidance_scale.*{other}"):
                gen(guidance_scale=1.5, negative_prompt_ids=NEG, **kw)
        for name, kw in BAD[:5] + BAD[7:10] + BAD[11:13] + BAD[14:15] + BAD[18:22]:
            kw = {k: v for k, v in kw.items() if k not in ("min_len", "multimodal")}
            with pytest.raises(ValueError, match=name):
                gen(**kw)
    with pytest.raises(ValueError, match="negative_prompt_ids.*negative_images"):
        mm(guidance_scale=2.0)                                                                   # Kosmos with neither negative
    with pytest.raises(ValueError, match="negative_prompt_ids"):
        mm(guidance_scale=2.0, negative_prompt_ids=torch.zeros(2, 1, dtype=torch.long))          # the image is spliced after two tokens
    with pytest.raises(ValueError, match="negative_images"):
        mm(negative_images=img)                                                                  # without a scale
    with pytest.raises(ValueError, match="negative_images"):
        mm(guidance_scale=2.0, negative_images=img[:1])
    with pytest.raises(TypeError, match="negative_images"):
        lm(guidance_scale=2.0, negative_images=img)                                              # no keyword of the text model


def test_generate_with_the_keywords_reaches_the_device_check():
    """The same calls with good values get as far as the device refusal (before this feature: TypeError)."""
    lm, mm, img = _models()
    for kw in (dict(guidance_scale=1.5), dict(guidance_scale=0.0, negative_prompt_ids=NEG, negative_prompt_lengths=[1, 3]),
               dict(guidance_scale=3, negative_prompt_ids=NEG, prompt_lengths=[2, 4], do_sample=True, top_k=5, output_logits=True,
                    logit_bias={3: 1.0}, no_repeat_ngram_size=2, eos_token_id=2, prefill_chunk=2, output_logprobs=True),
               dict(guidance_scale=1.0)):
        with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
            lm(**kw)
    for kw in (dict(guidance_scale=1.5, negative_prompt_ids=NEG), dict(guidance_scale=1.5, negative_images=img),
               dict(guidance_scale=-1.0, negative_prompt_ids=NEG, negative_prompt_lengths=[2, 3], negative_images=img),
               dict(guidance_scale=1.0)):
        with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
            mm(**kw)


def test_the_signatures_carry_the_keyword_only_arguments():
    from kosmosx import ops
    from kosmosx.model import Kosmos, KosmosLanguage
    names = dict(guidance_scale=1.0, negative_prompt_ids=None, negative_prompt_lengths=None)
    # (the loop takes the scale alone: run_generate turns the negatives into rows)
    for fn, pinned in ((Kosmos.generate, names), (KosmosLanguage.generate, names), (G.loop_options, dict(guidance_scale=1.0))):
        p = inspect.signature(fn).parameters
        for name, default in pinned.items():
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__qualname__, name)
            assert p[name].default is None if default is None else p[name].default == 1.0, (fn.__qualname__, name)
    p = inspect.signature(Kosmos.generate).parameters["negative_images"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert "negative_images" not in inspect.signature(KosmosLanguage.generate).parameters
    assert not set(names) & set(inspect.signature(G.Session.generate).parameters)                # sessions do not take them
    p = inspect.signature(G.check_guidance_args).parameters
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in (*names, "negative_images"))
    p = inspect.signature(ops.guidance_logits).parameters
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("scale", "out", "finished", "positions", "advance"))


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
    assert "int kx_guidance_logits(const kx_guidance_args* args, void* stream);" in HEADER
    assert hasattr(lib, "kx_guidance_logits") and "kx_guidance_logits" in _hip.SYMBOLS
    assert lib.kx_version() == 7 and "#define KX_ABI_VERSION 7" in HEADER                        # appended within ABI 7
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"typedef struct \{([^{}]*)\}\s*kx_guidance_args\s*;", body, flags=re.S)
    assert m
    names = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        names += [re.findall(r"([A-Za-z_0-9]+)\s*$", part.replace("*", " ").strip())[0] for part in decl.split(",")]
    assert names == [f[0] for f in _hip.GuidanceArgs._fields_] and names[0] == "struct_bytes"
    assert _hip.GuidanceArgs().struct_bytes == C.sizeof(_hip.GuidanceArgs)
    assert "KX_STRUCT_COUNT = 13" in HEADER                                                      # no kx_struct_id value is appended


# the pointers are never followed: every refusal comes before the launch
GOOD = dict(cond=1 << 20, ld_cond=10, uncond=2 << 20, ld_uncond=12, out=3 << 20, ld_out=11, B=2, V=10, scale=1.5, finished=0,
            positions=0, advance=1)
HOST_REFUSALS = [("null cond", dict(cond=0), KX_ERR_INVALID_ARG), ("null uncond", dict(uncond=0), KX_ERR_INVALID_ARG),
                 ("null out", dict(out=0), KX_ERR_INVALID_ARG), ("B=", dict(B=0), KX_ERR_INVALID_ARG),
                 ("V=", dict(V=0), KX_ERR_INVALID_ARG), ("ld_cond", dict(ld_cond=9), KX_ERR_INVALID_ARG),
                 ("ld_uncond", dict(ld_uncond=9), KX_ERR_INVALID_ARG), ("ld_out", dict(ld_out=9), KX_ERR_INVALID_ARG),
                 ("scale", dict(scale=NAN), KX_ERR_INVALID_ARG), ("scale", dict(scale=INF), KX_ERR_INVALID_ARG),
                 ("scale", dict(scale=-INF), KX_ERR_INVALID_ARG), ("advance", dict(advance=2), KX_ERR_INVALID_ARG),
                 ("advance", dict(advance=-1), KX_ERR_INVALID_ARG),
                 ("out overlaps uncond", dict(out=2 << 20), KX_ERR_INVALID_ARG),
                 ("out overlaps uncond", dict(out=(2 << 20) + 4 * 21), KX_ERR_INVALID_ARG),       # the last element of uncond's row 1
                 ("out overlaps uncond", dict(out=(2 << 20) - 4 * 20), KX_ERR_INVALID_ARG),       # out's last element on uncond's first
                 ("out overlaps cond", dict(out=(1 << 20) + 4), KX_ERR_INVALID_ARG),
                 ("out overlaps cond", dict(out=1 << 20), KX_ERR_INVALID_ARG),                    # the same pointer, another ld
                 ("V=", dict(V=(1 << 23) + 1, ld_cond=1 << 24, ld_uncond=1 << 24, ld_out=1 << 24), KX_ERR_UNSUPPORTED)]


def test_the_library_refuses_bad_guidance_arguments_before_any_launch(lib):
    from kosmosx import _hip
    for name, change, code in HOST_REFUSALS:
        a = _hip.GuidanceArgs()
        for k, v in dict(GOOD, **change).items():
            setattr(a, k, v)
        rc = lib.kx_guidance_logits(C.byref(a), None)
        msg = _hip.last_error()
        assert rc == code and "kx_guidance_logits" in msg and name in msg, (name, rc, msg)
    a = _hip.GuidanceArgs()
    a.struct_bytes -= 8
    assert lib.kx_guidance_logits(C.byref(a), None) == KX_ERR_INVALID_ARG and "stale binding" in _hip.last_error()
    assert lib.kx_guidance_logits(None, None) == KX_ERR_INVALID_ARG and "null args" in _hip.last_error()


# ---- the reference ----

def test_the_float64_reference_equals_an_independent_statement():
    """torch.log_softmax in float64 and s * (lc - lu) + lu."""
    rng = np.random.default_rng(5)
    for V in (1, 5, 257, 4097):
        for s in (0.0, -0.5, 1.0, 1.5, 3.0, 7.5):
            c, u = (rng.standard_normal((2, V)) * 4).astype(np.float32), (rng.standard_normal((2, V)) * 4).astype(np.float32)
            lc, lu = (torch.log_softmax(torch.from_numpy(x).double(), dim=-1) for x in (c, u))
            want = (s * (lc - lu) + lu).numpy()
            got = GR.guided_row_f64(c, u, s)
            assert got.dtype == np.float64 and np.allclose(got, want, rtol=0, atol=1e-12 * (1 + abs(s)) * max(1.0, np.abs(want).max()))
    c = np.array([0.5, -np.inf, 2.0, 1.0], dtype=np.float32)
    u = np.array([1.5, 0.25, -np.inf, 1.0], dtype=np.float32)
    got = GR.guided_row_f64(c, u, 1.5)
    assert np.isneginf(got[1]) and np.isneginf(got[2]) and np.isfinite(got[[0, 3]]).all()         # -inf in either row: never a candidate


def test_the_fp32_reference_returns_the_row_itself_when_both_rows_are_equal():
    """lc - lu is exactly 0, s * 0 is 0 and lu + 0 is lu: guided_row_f32(l, l, s) is l bit for bit, for any s."""
    rng = np.random.default_rng(6)
    l = GR.log_softmax_f64(rng.standard_normal(3001) * 4).astype(np.float32)
    for s in (0.0, -0.5, 1.0, 1.5, 3.0, 7.5, -1e30, 3e38):
        assert np.array_equal(GR.guided_row_f32(l, l, s).view(np.uint32), l.view(np.uint32)), s
    l[7] = -np.inf
    l[9] = np.nan
    got = GR.guided_row_f32(l, l, 2.0)
    assert np.isneginf(got[7]) and np.isneginf(got[9])                                          # the non-finite rule
    keep = np.ones(l.size, bool)
    keep[[7, 9]] = False
    assert np.array_equal(got[keep].view(np.uint32), l[keep].view(np.uint32))

