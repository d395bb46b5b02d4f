"""Beam search — what needs no GPU: generate()'s argument checks (raised before the device check and any launch), the C
surface of kx_beam_step / kx_beam_finalize / kx_kv_cache_gather (exported, sized, validated without a launch), and the
reference restatement (beam_ref) against itself: exhaustive search where the beam never prunes, and no near-tie of its own
under fp32 rounding of Gaussian inputs."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import beam_ref as BR

ROOT = Path(__file__).resolve().parent.parent
BEAM_SYMBOLS = ("kx_beam_step", "kx_beam_finalize", "kx_kv_cache_gather")


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
    from helpers import tiny_config
    from kosmosx.model import Kosmos, KosmosLanguage
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    tok = torch.zeros(2, 4, dtype=torch.long)
    img = torch.zeros(2, 3, m.cfg.vit.image, m.cfg.vit.image)
    return [(lambda **kw: lm.generate(tok, 4, **kw), 102), (lambda **kw: m.generate(tok, img, 4, **kw), m.cfg.vocab)]


REFUSED = [("do_sample", dict(do_sample=True)), ("temperature", dict(temperature=0.7)), ("top_k", dict(top_k=5)),
           ("top_p", dict(top_p=0.9)), ("repetition_penalty", dict(repetition_penalty=1.2)),
           ("prompt_lengths", dict(prompt_lengths=[3, 4])), ("sequence_ids", dict(sequence_ids=torch.arange(2))),
           ("output_logits", dict(output_logits=True)), ("num_beams", dict(num_beams=17)),
           ("num_return_sequences", dict(num_return_sequences=5)), ("length_penalty", dict(length_penalty=-0.5))]


@pytest.mark.parametrize("name,kw", REFUSED, ids=[n for n, _ in REFUSED])
def test_generate_refuses_what_beam_search_does_not_offer(name, kw):
    """CPU tensors: the ValueError comes before the device check, hence before any launch, and names the argument."""
    for gen, _ in _models():
        with pytest.raises(ValueError, match=name):
            gen(**{"num_beams": 4, **kw})
    # the same call without the offending argument gets as far as the device check
    for gen, _ in _models():
        with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
            gen(num_beams=4)


def test_generate_refuses_more_candidates_than_the_vocabulary():
    from kosmosx.model import KosmosLanguage
    lm = KosmosLanguage(vocab_size=20, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    with pytest.raises(ValueError, match="num_beams.*vocabulary"):
        lm.generate(torch.zeros(1, 4, dtype=torch.long), 4, num_beams=11)
    with pytest.raises(ValueError, match="num_beams"):
        lm.generate(torch.zeros(1, 4, dtype=torch.long), 4, num_beams=0)
    with pytest.raises(ValueError, match="output_scores"):
        lm.generate(torch.zeros(1, 4, dtype=torch.long), 4, output_scores=True)      # an output of beam search only


def test_the_library_exports_the_beam_entry_points_within_abi_7(lib):
    from kosmosx import _hip
    for name in BEAM_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _hip.SYMBOLS
    assert lib.kx_version() == 7
    assert _hip.KX_RAGGED_ERR_GATHER == 4
    sid = _hip.STRUCT_IDS.index(_hip.BeamArgs)
    assert sid == 11 and lib.kx_struct_bytes(sid) == C.sizeof(_hip.BeamArgs) > 0
    header = (ROOT / "include" / "kosmosx_hip.h").read_text()
    assert "KX_STRUCT_BEAM_ARGS = 11" in header and "KX_RAGGED_ERR_GATHER = 4" in header


def _good_args():
    from kosmosx import _hip
    a = _hip.BeamArgs()
    a.logits, a.ld, a.B, a.Win, a.W, a.V, a.step, a.length_penalty = 256, 512, 2, 4, 4, 502, 1, 1.0
    a.eos_id, a.pad_id = -1, 1
    for f in ("scores_in", "scores_out", "next_token", "parent", "src_row", "pool_score", "pool_end", "pool_parent", "pool_count",
              "done", "scratch"):
        setattr(a, f, 256)
    return a


def test_beam_entry_points_validate_without_a_launch(lib):
    from kosmosx import _hip
    assert lib.kx_beam_step(None, None) == 1 and "null" in _hip.last_error()
    a = _good_args()
    a.struct_bytes -= 8
    assert lib.kx_beam_step(C.byref(a), None) == 1 and "stale binding" in _hip.last_error()
    for field, value, word in (("logits", None, "null"), ("scratch", None, "null"), ("W", 17, "W="), ("Win", 2, "Win="),
                               ("V", 7, "V="), ("ld", 500, "ld="), ("step", -1, "step="), ("length_penalty", -1.0, "length_penalty"),
                               ("B", 0, "B=")):
        a = _good_args()
        setattr(a, field, value)
        assert lib.kx_beam_step(C.byref(a), None) == 1 and word in _hip.last_error(), field
    a = _good_args()
    a.Win, a.step = 1, 0                                   # scores_in == scores_out with Win != W
    assert lib.kx_beam_step(C.byref(a), None) == 1 and "scores_in" in _hip.last_error()
    # finalize: scores_live, done, pool x 4, parent, token, trace_ld, B, W, R, n, alpha, eos, pad, out_tokens, out_ld, out_scores
    assert lib.kx_beam_finalize(None, 256, 256, 256, 256, 256, 256, 256, 8, 2, 4, 2, 5, 1.0, -1, 1, 256, 5, 256, None) == 1
    assert "null" in _hip.last_error()
    assert lib.kx_beam_finalize(256, 256, 256, 256, 256, 256, 256, 256, 8, 2, 4, 5, 5, 1.0, -1, 1, 256, 5, 256, None) == 1
    assert "R=" in _hip.last_error()
    assert lib.kx_beam_finalize(256, 256, 256, 256, 256, 256, 256, 256, 8, 2, 4, 2, 6, 1.0, -1, 1, 256, 5, 256, None) == 1
    assert "n=" in _hip.last_error()
    assert lib.kx_beam_finalize(256, 256, 256, 256, 256, 256, 256, 256, 7, 2, 4, 2, 5, 1.0, -1, 1, 256, 5, 256, None) == 1
    assert "trace_ld" in _hip.last_error()
    # gather: src_k, src_v, dst_k, dst_v, L, B_src, B_dst, heads, Tmax, t, elem_bytes, src_row, error_word, stream
    big = 1 << 30
    assert lib.kx_kv_cache_gather(None, 256, 256, 256, 2, 2, 6, 3, 10, 7, 4, 256, 256, None) == 1 and "null" in _hip.last_error()
    assert lib.kx_kv_cache_gather(big, 2 * big, 3 * big, 4 * big, 2, 2, 6, 3, 10, 7, 4, 256, None, None) == 1
    assert "null" in _hip.last_error()
    assert lib.kx_kv_cache_gather(big, 2 * big, 3 * big, 4 * big, 2, 2, 6, 3, 10, 7, 3, 256, 256, None) == 1
    assert "elem_bytes" in _hip.last_error()
    assert lib.kx_kv_cache_gather(big, 2 * big, 3 * big, 4 * big, 2, 2, 6, 3, 10, 11, 4, 256, 256, None) == 1
    assert "t=" in _hip.last_error()
    assert lib.kx_kv_cache_gather(big + 8, 2 * big, 3 * big, 4 * big, 2, 2, 6, 3, 10, 7, 4, 256, 256, None) == 1
    assert "aligned" in _hip.last_error()
    # dst_k starts inside src_k ([2, 2, 3, 10, 64] fp32 = 30720 bytes): refused, nothing launched
    assert lib.kx_kv_cache_gather(big, 2 * big, big + 4096, 4 * big, 2, 2, 6, 3, 10, 7, 4, 256, 256, None) == 1
    assert "overlap" in _hip.last_error()
    assert lib.kx_kv_cache_gather(big, 2 * big, 3 * big, 4 * big, 2, 2, 6, 3, 10, 0, 4, 256, 256, None) == 0   # t = 0: nothing to copy


def test_beam_ref_equals_exhaustive_search_when_the_beam_never_prunes():
    """V = 3, n = 3, W = 16 >= the 9 prefixes ever alive: beam search is then exhaustive search.  Without EOS, alpha = 0.7."""
    V, n, W, alpha = 3, 3, 16, 0.7
    rng = np.random.default_rng(3)
    table = {}

    def step_logits(prefix):
        if prefix not in table:
            table[prefix] = (rng.standard_normal(V) * 2).astype(np.float32)
        return table[prefix]

    want = BR.brute_force(step_logits, n, W, alpha)
    prefixes, scores, pool = [()], np.zeros(1), []
    parent, token = [], []
    for g in range(n):
        Win = 1 if g == 0 else W
        rows = np.stack([step_logits(prefixes[j]) if j < len(prefixes) and prefixes[j] is not None else np.zeros(V, np.float32)
                         for j in range(Win)])
        # V = 3 < 2W: the reference does not need the kernel's V >= 2W; dead beams carry -inf
        r = BR.step(rows, scores, pool, g, W=W, alpha=alpha)
        assert r["pool"] == [] and not r["done"]
        prefixes = [None if not np.isfinite(s) else prefixes[p] + (t,) for t, p, s in zip(r["token"], r["parent"], r["score"])]
        scores = np.array(r["score"])
        parent.append(r["parent"]), token.append(r["token"])
    assert sum(p is not None for p in prefixes) == 16                       # 27 sequences exist, the 16 best are alive
    fin = BR.finalize(scores, pool, False, n, W=W, R=W, alpha=alpha)
    got = [(s, BR.backtrack(fin["pool"][k], parent, token, n)) for s, k in zip(fin["score"], fin["order"])]
    assert len(got) == len(want) == 16
    for (gs, gt), (ws, wt) in zip(got, want):
        assert gt == wt and abs(gs - ws) < 1e-12


def test_beam_ref_pool_rules():
    """EOS inside the first W enters the pool, between W and 2W it is skipped; a full pool takes only strictly better scores; done."""
    W, V, eos = 2, 8, 5
    x = np.full((1, V), -10.0, np.float32)
    x[0, [5, 3, 2, 6]] = [3.0, 2.0, 1.0, 0.0]                               # EOS ranked first
    r = BR.step(x, np.zeros(1), [], 0, W=W, eos=eos)
    assert r["token"] == [3, 2] and [p["end"] for p in r["pool"]] == [0] and not r["done"]
    x[0, [3, 2, 5, 6]] = [3.0, 2.0, 1.0, 0.0]                               # EOS ranked third (>= W): skipped
    r = BR.step(x, np.zeros(1), [], 0, W=W, eos=eos)
    assert r["token"] == [3, 2] and r["pool"] == []
    full = [dict(score=-1.0, end=0, parent=0), dict(score=-2.0, end=0, parent=1)]
    assert BR._offer(full, W, -2.0, 3, 0, [])[1]["end"] == 0                # equal to the worst: kept out
    assert BR._offer(full, W, -1.5, 3, 0, [])[1]["end"] == 3                # strictly better: replaces the worst
    x2 = np.stack([x[0], x[0]])
    assert BR.step(x2, np.array([-0.1, -0.2]), full, 1, W=W, eos=eos, early=True)["done"]
    assert not BR.step(x2, np.array([-0.1, -0.2]), full, 1, W=W, eos=eos)["done"]       # a live beam can still beat -2
    assert BR.step(x2, np.array([-9.0, -9.5]), full, 1, W=W, eos=eos)["done"]
    fr = BR.step(x2, np.array([-0.1, -0.2]), full, 2, W=W, eos=eos, done=True)
    assert fr["token"] == [1, 1] and fr["parent"] == [0, 1] and fr["score"] == [-0.1, -0.2] and fr["pool"] == full


@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_beam_ref_has_no_near_tie_of_its_own_under_fp32_rounding(scale):
    """Gaussian logits at the scales the GPU tests use, 24 steps, cumulative scores inside (-256, 0]: the reference on the
    float64 values and on their fp32-rounded copy takes the same decisions at every step and its scores agree far inside
    EPS_S: rounding the inputs alone produces no counted case, so the 1 % cap is the device's to use."""
    B, W, V, n = 3, 4, 502, 24
    rng = np.random.default_rng(11)
    tally = BR.Tally()
    for b in range(B):
        scores, pool, done = np.zeros(1), [], False
        for g in range(n):
            x64 = rng.standard_normal((1 if g == 0 else W, V)) * scale
            x32 = x64.astype(np.float32)
            eos = int(np.argsort(-x64[0])[1]) if g % 5 == 4 else None
            a = BR.step(x64, scores, pool, g, W=W, eos=eos, done=done)
            r = BR.step(x32, scores, pool, g, W=W, eos=eos, done=done)
            assert abs(max(scores)) < 256
            got = dict(token=r["token"], parent=r["parent"], score=r["score"], done=r["done"],
                       pool=([p["score"] for p in r["pool"]], [p["end"] for p in r["pool"]], [p["parent"] for p in r["pool"]],
                             len(r["pool"])))
            assert BR.check_step(got, a, tally) == "exact"
            assert np.allclose(a["score"], r["score"], atol=1e-5, rtol=0)
            scores, pool, done = np.array(r["score"]), r["pool"], r["done"]
    assert tally.cases == B * n and tally.counted == 0, (tally.counted, tally.cases)
