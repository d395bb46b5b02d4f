"""Contrastive search (generate(penalty_alpha=)) without a GPU: the refusals, the defaults, the C surface and its host-side
argument checks, and the float64 reference (tests/contrast_ref.py) against a direct cosine-similarity formulation."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import contrast_ref as R
from kosmosx import _hip as H
from kosmosx import generation as G
from kosmosx.model import Kosmos, KosmosLanguage

ROOT = Path(__file__).resolve().parent.parent
NEW = ("kx_contrast_candidates", "kx_contrast_hidden", "kx_contrast_scratch_bytes", "kx_contrast_select", "kx_kv_cache_commit")
V = 102


@pytest.fixture(scope="module")
def lm():
    return KosmosLanguage(vocab_size=V, dim=128, depth=2, ffn_dim=256, decoder_heads=2, _seed=0, _perturb=0.1, _max_positions=64).eval()


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    return H.load()


TOK = torch.zeros(2, 5, dtype=torch.long)
ON = dict(penalty_alpha=0.6, top_k=4)

# what generate() itself refuses through check_contrast_args (every earlier check lets the call pass)
THROUGH_GENERATE = [dict(do_sample=True), dict(return_session=True), dict(guidance_scale=1.5),
                    dict(row_options=[{}, {}]), dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[3]]),
                    dict(min_new_tokens=2, eos_token_id=5), dict(stop_sequences=[[3, 4]]), dict(logit_bias={3: 1.0}),
                    dict(presence_penalty=0.5), dict(frequency_penalty=0.5), dict(min_p=0.1), dict(typical_p=0.9), dict(epsilon_cutoff=1e-3),
                    dict(eta_cutoff=1e-3), dict(repetition_penalty=1.2), dict(temperature=0.7), dict(top_p=0.9), dict(output_logprobs=True),
                    dict(prefill_chunk=2)]
# combinations an earlier check of run_generate already refuses in its own words: the check is called directly
DIRECT = [dict(num_beams=3), dict(num_return_sequences=2), dict(prompt_lookup_num_tokens=2)]


@pytest.mark.parametrize("extra", THROUGH_GENERATE, ids=lambda d: next(iter(d)))
def test_generate_refuses_the_combination_naming_penalty_alpha_before_the_device_check(lm, extra):
    if "guidance_scale" in extra:
        extra = dict(extra, negative_prompt_ids=None)
    with pytest.raises(ValueError, match="penalty_alpha") as e:
        lm.generate(TOK, 4, **ON, **extra)
    assert next(iter(extra)) in str(e.value)
    # the same call without penalty_alpha (top_k is then the sampler's) gets as far as the device check, or runs into it directly
    with pytest.raises(RuntimeError, match="no CPU fallback|not on a CUDA"):
        lm.generate(TOK, 4, top_k=4, **extra)


def test_a_token_automaton_is_refused():
    with pytest.raises(ValueError, match="penalty_alpha.*token_automaton"):       # (the check only asks whether one is given)
        G.check_contrast_args(V, **ON, token_automaton=object())


@pytest.mark.parametrize("extra", DIRECT + THROUGH_GENERATE, ids=lambda d: next(iter(d)))
def test_check_contrast_args_refuses_every_combination(extra):
    extra = {n: v for n, v in extra.items() if n in inspect.signature(G.check_contrast_args).parameters}
    with pytest.raises(ValueError, match="penalty_alpha") as e:
        G.check_contrast_args(V, **ON, **extra)
    assert next(iter(extra)) in str(e.value) and "DESIGN.md §8" in str(e.value)
    assert G.check_contrast_args(V, **extra) is None     # without the keyword the check has nothing to say


@pytest.mark.parametrize("alpha", [True, False, float("nan"), float("inf"), -0.1, 1.5, "0.5", [0.5]])
def test_a_bad_penalty_alpha_is_refused(lm, alpha):
    with pytest.raises(ValueError, match="penalty_alpha"):
        lm.generate(TOK, 4, penalty_alpha=alpha, top_k=4)


@pytest.mark.parametrize("k", [0, 17, -1, True, 2.0, V + 1])
def test_a_bad_top_k_is_refused_naming_penalty_alpha(lm, k):
    with pytest.raises(ValueError, match="penalty_alpha.*top_k"):
        lm.generate(TOK, 4, penalty_alpha=0.5, top_k=k)


def test_good_arguments_reach_the_device_check(lm):
    for kw in (dict(penalty_alpha=0.0, top_k=1), dict(penalty_alpha=1, top_k=16), dict(**ON, output_contrast=True, output_logits=True),
               dict(**ON, prompt_lengths=[2, 5], eos_token_id=3, pad_token_id=0, eos_poll=2)):
        with pytest.raises(RuntimeError, match="no CPU fallback|not on a CUDA"):
            lm.generate(TOK, 4, **kw)
    assert G.check_contrast_args(V, penalty_alpha=1, top_k=16, output_contrast=True) == dict(alpha=1.0, k=16, trace=True)


def test_output_contrast_needs_penalty_alpha(lm):
    with pytest.raises(ValueError, match="output_contrast"):
        lm.generate(TOK, 4, output_contrast=True)


def test_the_multimodal_model_refuses_alike():
    from helpers import tiny_config
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    img = torch.zeros(2, 3, m.cfg.vit.image, m.cfg.vit.image)
    with pytest.raises(ValueError, match="penalty_alpha.*do_sample"):
        m.generate(TOK, img, 4, **ON, do_sample=True)
    with pytest.raises(RuntimeError, match="no CPU fallback|not on a CUDA"):
        m.generate(TOK, img, 4, **ON)


def test_the_defaults_are_off():
    for fn in (Kosmos.generate, KosmosLanguage.generate, G.loop_options, G.check_contrast_args):
        p = inspect.signature(fn).parameters
        assert p["penalty_alpha"].kind is inspect.Parameter.KEYWORD_ONLY and p["penalty_alpha"].default is None, fn.__qualname__
        assert p["output_contrast"].default is False
    assert "penalty_alpha" not in inspect.signature(G.Session.generate).parameters          # sessions do not take it
    assert G.loop_options(V, 2).contrast is None
    assert G.loop_options(V, 2, **ON).contrast == dict(alpha=0.6, k=4, trace=False)
    src = inspect.getsource(G.run_generate)
    assert src.index("check_truncation_args(") < src.index("check_contrast_args(") < src.index("check_row_options(")


# ---- the C surface ----

def _header_prototypes():
    body = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kosmosx_hip.h").read_text(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|size_t)\s+(kx_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", body):
        out[m.group(2)] = (m.group(1), [a.strip() for a in m.group(3).split(",")])
    return out


def test_the_header_section_matches_the_ctypes_prototypes():
    text = (ROOT / "include" / "kosmosx_hip.h").read_text()
    assert "Contrastive search on the device" in text
    assert re.search(r"#define KX_ABI_VERSION 7\b", text) and re.search(r"KX_STRUCT_COUNT = 13\b", text) and len(H.STRUCT_IDS) == 13
    assert re.search(r"KX_RAGGED_ERR_COMMIT = 8\b", text) and H.KX_RAGGED_ERR_COMMIT == 8
    protos = _header_prototypes()

    def ctype(decl):
        if "*" in decl:
            return C.POINTER(H.DecoderWeights) if "kx_decoder_weights" in decl else C.c_void_p
        return {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float, "size_t": C.c_size_t}[decl.split()[-2]]
    for name in NEW:
        res, args = protos[name]
        bres, bargs = H.SYMBOLS[name]
        assert bres is {"int": C.c_int, "size_t": C.c_size_t}[res], name
        assert [ctype(a) for a in args] == list(bargs), name


def test_the_library_is_still_abi_7_and_exports_the_entry_points(lib):
    assert lib.kx_version() == 7
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.kx_contrast_scratch_bytes(3, 5, 100) == 3 * 4 * 5 * 4                       # ceil(100 / 32) chunks
    assert lib.kx_contrast_scratch_bytes(0, 5, 100) == 0


P = 4096        # a fake, 16-byte aligned device pointer: every call below is refused before anything is launched


def _select(lib, **over):
    a = dict(u=P, prob=P, history=P * 4096, B=2, k=4, D=128, cap=64, hist_rows=P, p_stride=1, hist_len=P, alpha=0.6, oma=0.4, step_tokens=P,
             finished=P, eos=-1, pad=1, next_token=P, chosen=P, out_tokens=0, out_ld=1, out_col=0, cand_penalty=0, chosen_trace=0,
             scratch=P, scratch_bytes=1 << 20, error_word=P)
    a.update(over)
    return lib.kx_contrast_select(*a.values(), None)


def test_host_checks_of_the_select_launch(lib):
    for over, word in ((dict(u=0), "null"), (dict(history=0), "null"), (dict(hist_rows=0), "hist_rows"), (dict(chosen=0), "chosen"),
                       (dict(scratch=0), "scratch"), (dict(error_word=0), "error_word"), (dict(k=0), "k=0"), (dict(k=17), "k=17"),
                       (dict(B=0), "B=0"), (dict(D=130), "D=130"), (dict(k=16, D=4096), "128 KB"), (dict(cap=1), "cap=1"),
                       (dict(p_stride=0), "p_stride"), (dict(alpha=1.5), "alpha"), (dict(oma=-0.5), "one_minus_alpha"),
                       (dict(out_tokens=P, out_col=1), "out_col"), (dict(u=P + 4), "aligned"), (dict(history=P), "overlap"),
                       (dict(scratch_bytes=16), "scratch")):
        assert _select(lib, **over) == 1, over
        assert word in H.last_error(), (over, H.last_error())
        assert "kx_contrast_select" in H.last_error()


def test_host_checks_of_the_candidates_launch(lib):
    def call(**over):
        a = dict(logits=P, ld=V, rows=8, B=2, V=V, k=4, chosen=P, k_prev=4, finished=0, step_tokens=P, prob=P, cand_id=0, cand_prob=0, out_ld=1,
                 out_col=0)
        a.update(over)
        return lib.kx_contrast_candidates(*a.values(), None)
    for over, word in ((dict(logits=0), "logits"), (dict(step_tokens=0), "step_tokens"), (dict(prob=0), "prob"), (dict(cand_id=P), "together"),
                       (dict(B=0), "B=0"), (dict(V=0), "V=0"), (dict(ld=V - 1), "ld="), (dict(k=0), "k=0"), (dict(k=17), "k=17"),
                       (dict(V=3, ld=3), "k=4"), (dict(k_prev=17), "k_prev"), (dict(chosen=0), "k_prev"), (dict(rows=7), "rows=7"),
                       (dict(cand_id=P, cand_prob=P, out_col=1), "out_col")):
        assert call(**over) == 1, over
        assert word in H.last_error() and "kx_contrast_candidates" in H.last_error(), (over, H.last_error())


def test_host_checks_of_the_commit_launch(lib):
    def call(**over):
        a = dict(ktail=P, vtail=2 * P, kcache=1 << 24, vcache=1 << 25, L=2, B=3, k=4, heads=2, Tmax=32, Ttail=1, eb=4, chosen=P, positions=P,
                 finished=0, error_word=P)
        a.update(over)
        return lib.kx_kv_cache_commit(*a.values(), None)
    for over, word in ((dict(ktail=0), "null"), (dict(vcache=0), "null"), (dict(chosen=0), "chosen"), (dict(positions=0), "positions"),
                       (dict(error_word=0), "error_word"), (dict(eb=3), "elem_bytes"), (dict(k=0), "k=0"), (dict(k=17), "k=17"),
                       (dict(L=0), "bad shape"), (dict(B=0), "bad shape"), (dict(Tmax=0), "bad shape"), (dict(Ttail=0), "bad shape"),
                       (dict(kcache=(1 << 24) + 8), "aligned"), (dict(vtail=P), "overlap"), (dict(vcache=1 << 24), "overlap"),
                       (dict(ktail=1 << 24), "overlap")):
        assert call(**over) == 1, over
        assert word in H.last_error() and "kx_kv_cache_commit" in H.last_error(), (over, H.last_error())


def test_host_checks_of_the_hidden_rows_launch(lib):
    w = H.DecoderWeights()
    w.struct_bytes, w.layer_bytes = C.sizeof(H.DecoderWeights), C.sizeof(H.DecoderLayer)
    w.dim, w.ffn, w.layers, w.heads, w.vocab = 128, 256, 2, 2, V
    w.ln_g = w.ln_b = P

    def call(w_=w, **over):
        a = dict(x=P, workspace=0, B=2, T=3, prec=0, step=0, lengths=0, out=1 << 20, out_ld=3 * 128, residual_out=0)
        a.update(over)
        return lib.kx_contrast_hidden(C.byref(w_), *a.values(), None)
    for over, word in ((dict(x=0), "null"), (dict(out=0), "null"), (dict(B=0), "B=0"), (dict(out_ld=100), "out_ld"),
                       (dict(step=1), "T == 1"), (dict(step=1, T=1, out_ld=128), "workspace"),
                       (dict(step=1, T=1, out_ld=128, workspace=P + 16), "aligned"), (dict(step=1, T=1, out_ld=128, workspace=P, prec=2), "precision")):
        assert call(**over) == 1, over
        assert word in H.last_error() and "kx_contrast_hidden" in H.last_error(), (over, H.last_error())
    stale = H.DecoderWeights()
    stale.struct_bytes = 8
    assert call(stale) == 1 and "stale binding" in H.last_error()


# ---- the reference ----

def test_the_reference_against_cosine_similarity_on_hand_made_rows():
    e = np.eye(4)
    hist = np.stack([e[0], e[1], (e[0] + e[1]) / np.sqrt(2.0)])
    u = np.stack([e[0], e[2], e[3], (e[0] + e[2]) / np.sqrt(2.0)])
    pen = R.penalty(u, hist)
    assert pen[0] == 1.0 and pen[1] == 0.0 and pen[2] == 0.0 and abs(pen[3] - np.sqrt(0.5)) < 1e-15
    assert np.allclose(pen, R.cosine_penalty(u, hist), atol=1e-15)
    assert np.allclose(R.penalty(u, hist[:1]), [1.0, 0.0, 0.0, np.sqrt(0.5)], atol=1e-15)  # P = 1
    # alpha = 0.5: the identical candidate loses its lead, the orthogonal ones keep their probability
    s = R.scores([0.5, 0.3, 0.1, 0.1], pen, 0.5)
    assert np.allclose(s, [-0.25, 0.15, 0.05, 0.05 - 0.5 * np.sqrt(0.5)]) and R.choose(s) == 1
    assert R.choose(R.scores([0.5, 0.3, 0.1, 0.1], pen, 0.0)) == 0                         # alpha = 0: greedy
    assert R.choose([0.2, 0.7, 0.7]) == 1 and R.choose([float("nan"), -5.0]) == 1 and R.choose([float("nan")] * 3) == 0
    # unscaled rows: the unit rows are what makes the dot product a cosine
    rng = np.random.default_rng(0)
    x, hx = rng.standard_normal((3, 16)), rng.standard_normal((7, 16))
    g, b = rng.standard_normal(16), rng.standard_normal(16)
    uu, hh = R.unit_rows(x, g, b), R.unit_rows(hx, g, b)
    assert np.allclose(np.linalg.norm(uu, axis=1), 1.0, atol=1e-14)
    c = x - x.mean(1, keepdims=True)
    ln = c / np.sqrt(c.var(1, keepdims=True) + R.EPS) * g + b
    c2 = hx - hx.mean(1, keepdims=True)
    ln2 = c2 / np.sqrt(c2.var(1, keepdims=True) + R.EPS) * g + b
    assert np.allclose(R.penalty(uu, hh), R.cosine_penalty(ln, ln2), atol=1e-13)


def test_the_fp32_restatements_stay_close_to_float64():
    for D, bound in ((128, 4e-8), (2048, 1.8e-8)):
        x, g, b = R.hidden_rows(0, 18, D)
        dev = np.abs(R.unit_rows_fp32(x, g, b).astype(np.float64) - R.unit_rows(x, g, b)).max()
        assert 0 < dev <= bound, (D, dev)                 # the figures of the module's docstring
    s32 = R.scores_fp32([0.5, 0.25], [0.75, 0.125], 0.6)
    assert s32.dtype == np.float32 and np.allclose(s32, R.scores([0.5, 0.25], [0.75, 0.125], 0.6), atol=1e-7)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: f"s{c[0]}-k{c[1]}-D{c[2]}-P{'_'.join(map(str, c[3]))}")
def test_the_best_two_scores_of_every_gpu_case_are_more_than_1e_3_apart(case):
    seed, k, D, Ps = case
    _, scs, _ = R.case_reference(R.select_case(seed, k, D, Ps))
    for b, s in enumerate(scs):
        assert R.best_gap(s) > 1e-3, (case, b, np.sort(s)[-2:])
