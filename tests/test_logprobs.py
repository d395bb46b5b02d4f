"""Per-token log-probs out of generate() without a GPU: the float64 reference of tests/logprob_ref.py against hand-made rows,
generate()'s refusals around ``output_logprobs`` / ``top_logprobs`` (which come before the device check), the public signatures, and
the library's new entry point, which validates before any launch."""
import inspect
from pathlib import Path

import pytest
import torch

import logprob_ref as R
from kosmosx import generation as G

ROOT = Path(__file__).resolve().parent.parent
NINF = float("-inf")
KX_ERR_INVALID_ARG = 1                                      # include/kosmosx_hip.h, kx_status


def test_the_reference_breaks_ties_by_the_lowest_id():
    row = torch.tensor([1.0, 3.0, 3.0, -2.0, 3.0, 1.0, 0.0, -0.0])
    ids, lps = R.top_ref(row, 8)
    assert ids.tolist() == [1, 2, 4, 0, 5, 6, 7, 3]                          # (-0.0 == 0.0: a tie, the lower id first)
    want = torch.log_softmax(row.double(), -1)
    assert torch.equal(lps, want[ids])
    assert bool((lps[:-1] >= lps[1:]).all())
    assert abs(float(torch.logsumexp(R.log_softmax_ref(row), -1))) < 1e-12


def test_the_reference_sorts_minus_infinity_last_and_pads_short_rows():
    row = torch.tensor([NINF, 2.0, NINF, 5.0, NINF])
    ids, lps = R.top_ref(row, 4)
    assert ids.tolist() == [3, 1, 0, 2]                                      # the -inf entries after every finite one, lowest id first
    assert lps[2:].tolist() == [NINF, NINF] and bool(torch.isfinite(lps[:2]).all())
    ids, lps = R.top_ref(torch.tensor([0.5, 1.5, -1.0]), 5)                  # V = 3 < n = 5
    assert ids.tolist() == [1, 0, 2, -1, -1] and lps[3:].tolist() == [NINF, NINF]
    ids, lps = R.top_ref(torch.tensor([7.0]), 2)
    assert ids.tolist() == [0, -1] and lps.tolist() == [0.0, NINF]


def test_the_step_reference_gathers_the_token_and_zeroes_a_bad_one():
    x = torch.randn(3, 9, generator=torch.Generator().manual_seed(0)) * 4
    lp, tl, ti = R.step_ref(x, torch.tensor([4, 9, -1]), 3)
    assert lp[0] == torch.log_softmax(x[0].double(), -1)[4] and lp[1:].tolist() == [0.0, 0.0]
    assert tl.shape == (3, 3) and ti.shape == (3, 3) and ti.dtype == torch.int64
    assert torch.equal(ti, torch.topk(x, 3, dim=-1).indices)                 # (no ties in random normals)
    lp0, tl0, ti0 = R.step_ref(x, torch.tensor([4, 9, -1]), 0)
    assert tl0.shape == (3, 0) and ti0.shape == (3, 0) and torch.equal(lp0, lp)


ON = dict(output_logprobs=True, beams=False, drafts=0)
REFUSED = [("top_logprobs", dict(ON, top_logprobs=-1)), ("top_logprobs", dict(ON, top_logprobs=G.MAX_TOP_LOGPROBS + 1)),
           ("top_logprobs", dict(ON, top_logprobs=True)), ("top_logprobs", dict(ON, top_logprobs=2.0)),
           ("top_logprobs", dict(ON, top_logprobs=None)), ("top_logprobs", dict(ON, top_logprobs=12, vocab=11)),
           ("top_logprobs", dict(ON, output_logprobs=False, top_logprobs=3)),
           ("output_logprobs", dict(ON, top_logprobs=0, beams=True)), ("output_logprobs", dict(ON, top_logprobs=2, drafts=3))]


@pytest.mark.parametrize("name,kw", REFUSED, ids=[f"{n}-{i}" for i, (n, _) in enumerate(REFUSED)])
def test_check_logprob_args_names_the_argument(name, kw):
    kw = dict(kw)
    with pytest.raises(ValueError, match=name):
        G.check_logprob_args(kw.pop("vocab", 102), **kw)


def test_check_logprob_args_accepts_what_is_offered():
    assert G.MAX_TOP_LOGPROBS == 16
    assert G.check_logprob_args(102, output_logprobs=False, top_logprobs=0, beams=True, drafts=4) == 0    # off: nothing to refuse
    for k in (0, 1, 16):
        assert G.check_logprob_args(102, output_logprobs=True, top_logprobs=k, beams=False, drafts=0) == k
    assert G.check_logprob_args(5, output_logprobs=True, top_logprobs=5, beams=False, drafts=0) == 5


def test_the_three_generate_signatures_carry_the_keyword_only_arguments():
    from kosmosx.model import Kosmos, KosmosLanguage
    for fn in (Kosmos.generate, KosmosLanguage.generate, G.Session.generate):
        p = inspect.signature(fn).parameters
        for name, default in (("output_logprobs", False), ("top_logprobs", 0)):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is default, (fn.__qualname__, name)
    p = inspect.signature(G.loop_options).parameters
    assert p["output_logprobs"].default is False and p["top_logprobs"].default == 0


def _models(batch=2):
    from helpers import tiny_config
    from kosmosx.model import Kosmos, KosmosLanguage
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    tok = torch.zeros(batch, 4, dtype=torch.long)
    img = torch.zeros(batch, 3, m.cfg.vit.image, m.cfg.vit.image)
    return [lambda **kw: lm.generate(tok, 4, **kw), lambda **kw: m.generate(tok, img, 4, **kw)]


def test_generate_with_logprobs_reaches_the_device_check():
    """CPU tokens: the call gets past the argument checks to the device refusal (before this feature: TypeError)."""
    for gen in _models():
        for kw in (dict(output_logprobs=True), dict(output_logprobs=True, top_logprobs=16, output_logits=True),
                   dict(output_logprobs=True, top_logprobs=5, do_sample=True, num_return_sequences=3, prompt_lengths=[3, 4]),
                   dict(output_logprobs=True, top_logprobs=1, return_session=True, stop_sequences=[[3, 4]], eos_token_id=2)):
            with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
                gen(**kw)


@pytest.mark.parametrize("name,kw", [("top_logprobs", dict(top_logprobs=3)),
                                     ("top_logprobs", dict(output_logprobs=True, top_logprobs=17)),
                                     ("top_logprobs", dict(output_logprobs=True, top_logprobs=True)),
                                     ("output_logprobs", dict(output_logprobs=True, num_beams=2)),
                                     ("output_logprobs", dict(output_logprobs=True, prompt_lookup_num_tokens=2))])
def test_generate_refuses_before_the_device_check(name, kw):
    for gen in _models():
        with pytest.raises(ValueError, match=name):
            gen(**kw)


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from kosmosx import _hip
    return _hip.load()


# (logits, ld, B, V, token, skip, token_logprob, out_ld, out_col, top_n, top_logprob, top_id): the pointers are never followed
GOOD = dict(logits=64, ld=10, B=2, V=10, token=64, skip=0, token_logprob=64, out_ld=4, out_col=3, top_n=5, top_logprob=64, top_id=64)
HOST_REFUSALS = [("logits", dict(logits=0)), ("token", dict(token=0)), ("token_logprob", dict(token_logprob=0)),
                 ("B", dict(B=0)), ("V", dict(V=0, ld=0)), ("ld", dict(ld=9)), ("out_col", dict(out_col=4)),
                 ("out_col", dict(out_col=-1)), ("top_n", dict(top_n=17)), ("top_n", dict(top_n=-1)),
                 ("top_logprob", dict(top_logprob=0)), ("top_id", dict(top_id=0))]


def step_logprobs_refusals(lib):
    """Every host refusal of kx_step_logprobs: -> [(argument, return code, message)]."""
    from kosmosx import _hip
    out = []
    for name, change in HOST_REFUSALS:
        a = dict(GOOD, **change)
        rc = lib.kx_step_logprobs(a["logits"], a["ld"], a["B"], a["V"], a["token"], a["skip"], a["token_logprob"], a["out_ld"],
                                  a["out_col"], a["top_n"], a["top_logprob"], a["top_id"], None)
        out.append((name, rc, _hip.last_error()))
    return out


def test_the_library_refuses_bad_arguments_before_any_launch(lib):
    assert lib.kx_version() == 7                                             # appended within ABI 7
    for name, rc, msg in step_logprobs_refusals(lib):
        assert rc == KX_ERR_INVALID_ARG and "kx_step_logprobs" in msg and name in msg, (name, rc, msg)
