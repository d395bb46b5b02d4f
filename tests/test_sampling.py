"""Token sampling, the parts that need no GPU: the CPU restatement of the contract (tests/sampling_ref.py) against known
answers, against the `transformers` logits processors and against the exact distribution; and the C entry point's
argument validation (no launch)."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import sampling_ref as R

ROOT = Path(__file__).resolve().parent.parent


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    out = R.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(w) for w in out] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xFFFFFFFF
    out = R.philox4x32_10(f, f, f, f, f, f)
    assert [int(w) for w in out] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    u = R.uniforms(seed=3, sequence_id=5, position=7, V=1003)
    assert u.shape == (1003,) and (u > 0).all() and (u < 1).all()
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)            # exact in fp32
    w = R.philox4x32_10(7, 5, 2, 0, 3, 0)                                        # element 9 = word 1 of block 2
    assert u[9] == (2.0 * (int(w[1]) >> 9) + 1.0) * 2.0 ** -24


def test_reference_filter_equals_the_transformers_processors():
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(0)
    checked = 0
    for V in (502, 1002, 32002, 64007):
        for case in range(6):
            s = (1.0, 2.0, 3.0)[case % 3]
            logits = (rng.standard_normal(V) * s).astype(np.float32)
            hist = rng.integers(0, V, 40)
            hist[5] = hist[3]                                                     # a duplicate: penalised once
            T, k, p, r = (0.8, 50, 0.9, 1.3) if case % 2 else (1.3, 0, 0.95, 1.0)
            x = R.scaled(logits, T, hist, r)
            keep, ahead, _ = R.filter_row(x, k, p)
            scores = torch.from_numpy(logits)[None]                               # fp32 through the two divisions, as the contract
            ids = torch.from_numpy(hist)[None]
            if r != 1.0:
                scores = lp.RepetitionPenaltyLogitsProcessor(r)(ids, scores)
            scores = lp.TemperatureLogitsWarper(T)(ids, scores)
            assert np.array_equal(scores[0].numpy(), x)
            scores = scores.double()
            if k:
                scores = lp.TopKLogitsWarper(k)(ids, scores)
            scores = lp.TopPLogitsWarper(p)(ids, scores)
            hf_keep = torch.isfinite(scores[0]).numpy()
            band = np.abs(ahead - float(np.float32(p))) < 1e-9                  # the boundary itself: summation order decides
            assert np.array_equal(keep[~band], hf_keep[~band]), (V, case)
            assert keep[int(np.argmax(x))]
            checked += 1
    assert checked == 24


def test_reference_sampler_draws_from_the_filtered_softmax():
    """V = 16, 200 000 draws over distinct (sequence id, position) pairs; chi-square against the exact probabilities at
    significance 1e-6."""
    rng = np.random.default_rng(1)
    V, N = 16, 200_000
    logits = (rng.standard_normal(V) * 2).astype(np.float32)
    T, k, p = 0.8, 12, 0.9
    x = R.scaled(logits, T)
    keep, _, _ = R.filter_row(x, k, p)
    assert 2 <= int(keep.sum()) < V
    e = np.where(keep, np.exp(x.astype(np.float64) - x.max()), 0.0)
    prob = e / e.sum()
    # all draws at once: one Philox block set per (sequence id, position)
    seq = np.repeat(np.arange(N // 100), 100)
    pos = np.tile(np.arange(100), N // 100)
    words = [R.philox4x32_10(pos, seq, np.full(N, blk), 0, 11, 0) for blk in range(V // 4)]
    w = np.stack([wd for blk in words for wd in blk], axis=1).astype(np.uint64)  # [N, V], element i = word i & 3 of block i >> 2
    u = (2.0 * (w >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    score = np.where(keep[None], x.astype(np.float64)[None] - np.log(-np.log(u)), -np.inf)
    tok = np.argmax(score, axis=1)
    for j in (0, 1234, N - 1):                                                    # the vectorised form is sample_row's draw
        assert tok[j] == R.sample_row(logits, temperature=T, top_k=k, top_p=p, seed=11, position=int(pos[j]),
                                      sequence_id=int(seq[j]))["token"]
    counts = np.bincount(tok, minlength=V)
    assert counts[~keep].sum() == 0
    chi2 = float(((counts[keep] - N * prob[keep]) ** 2 / (N * prob[keep])).sum())
    assert int(keep.sum()) - 1 == 8                                               # seeded: the degrees of freedom are fixed
    assert chi2 < 42.7010, chi2                                                   # chi-square upper 1e-6 point, 8 dof


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from kosmosx import _hip
    return _hip.load()


def _good_args():
    from kosmosx import _hip
    a = _hip.SampleArgs()
    a.do_sample, a.logits, a.ld, a.B, a.V = 1, 256, 512, 2, 502
    a.temperature, a.top_k, a.top_p, a.repetition_penalty = 1.0, 0, 1.0, 1.0
    a.next_token = 256
    a.eos_id, a.pad_id = -1, 1
    return a


def test_entry_point_is_exported_and_validates_without_a_launch(lib):
    from kosmosx import _hip
    assert hasattr(lib, "kx_sample_logits") and hasattr(lib, "kx_embed_step")
    assert lib.kx_version() == 7
    assert lib.kx_struct_bytes(_hip.STRUCT_IDS.index(_hip.SampleArgs)) == C.sizeof(_hip.SampleArgs)
    assert lib.kx_sample_logits(None, None) == 1 and "null" in _hip.last_error()
    for field, value, word in (("logits", 0, "logits"), ("V", 0, "V="), ("ld", 501, "ld="), ("temperature", -0.5, "temperature"),
                               ("temperature", math.nan, "temperature"), ("top_p", 0.0, "top_p"),
                               ("repetition_penalty", 0.0, "repetition_penalty"), ("repetition_penalty", -1.0, "repetition_penalty"),
                               ("next_token", 0, "next_token"), ("B", 0, "B=")):
        a = _good_args()
        setattr(a, field, value)
        assert lib.kx_sample_logits(C.byref(a), None) == 1, field
        assert word in _hip.last_error(), (field, _hip.last_error())
    a = _good_args()
    a.history, a.hist_ld, a.hist_len = 256, 8, 8                                 # no room to append
    assert lib.kx_sample_logits(C.byref(a), None) == 1 and "hist_ld" in _hip.last_error()
    a = _good_args()
    a.struct_bytes -= 8
    assert lib.kx_sample_logits(C.byref(a), None) == 1 and "stale binding" in _hip.last_error()
    # kx_embed_step: either position beyond the table is the out-of-range error of kx_embed_splice
    assert lib.kx_embed_step(256, 256, 256, 256, 2, 256, 502, 64, 62, -1, None) == 1 and "out of range" in _hip.last_error()
    assert lib.kx_embed_step(256, 256, 256, 256, 2, 256, 502, 64, 10, 62, None) == 1 and "out of range" in _hip.last_error()
    assert lib.kx_embed_step(None, 256, 256, 256, 2, 256, 502, 64, 10, -1, None) == 1 and "null" in _hip.last_error()


def test_ops_and_generate_refuse_cpu_tensors():
    from kosmosx import ops
    from kosmosx.model import KosmosLanguage
    with pytest.raises(RuntimeError, match="not on a CUDA"):
        ops.sample_logits(torch.zeros(2, 8))
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=16).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.generate(torch.zeros(1, 4, dtype=torch.long), 4)
