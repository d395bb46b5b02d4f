"""score() without a GPU: the float64 references of tests/score_ref.py against independent restatements, the GPU tests' inputs
against the stand-ins a broken kernel would compute, score()'s refusals (which come before the device check), and the library's
new entry points, which validate before any launch."""
import ctypes as C
from pathlib import Path

import pytest
import torch

import decode_ref as DR
import score_ref as R

ROOT = Path(__file__).resolve().parent.parent
BOUND = 2e-5                                                # what tests/test_attention_decode_shared_gpu.py holds the kernel to


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from kosmosx import _hip
    return _hip.load()


@pytest.mark.parametrize("K", R.ROWS)
def test_the_attention_reference_is_a_causal_attention_over_prefix_and_candidate(K):
    for t0 in (0, 1, 5, 130):
        qkv, kc, vc, _, seq = R.shared_inputs(t0, K, torch.float32, seed=3 + K)
        out, k1, v1 = R.shared_attention_ref(qkv, kc, vc, t0, seq, K, nan_to_num=True)
        assert k1 is kc and v1 is vc and out.dtype == torch.float64 and bool(torch.isfinite(out).all())
        for c in range(len(seq)):
            want = R.causal_full_attention(qkv, kc, vc, t0, int(seq[c]), c, K)
            assert float((out[c * K:(c + 1) * K] - want).abs().max()) < 1e-12, (t0, c)


def test_the_logprob_reference_is_log_softmax_gather():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 300, generator=g) * 4
    tg = torch.randint(0, 257, (11,), generator=g)
    idx = torch.randint(0, 7, (11,), generator=g)
    want = torch.log_softmax(x[idx, :257].double(), -1).gather(1, tg[:, None])[:, 0]
    got = R.token_logprob_ref(x, tg, idx, vocab=257)
    assert float((got - want).abs().max()) < 1e-12
    assert float((R.token_logprob_ref(x, torch.arange(7)) - torch.log_softmax(x.double(), -1).diagonal()).abs().max()) < 1e-12
    bad = R.token_logprob_ref(x, torch.tensor([257, -1, 3, 3]), torch.tensor([0, 0, 7, -1]), vocab=257)
    assert bad.tolist() == [0.0] * 4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_gpu_inputs_tell_the_wrong_kernels_from_the_right_one(dtype):
    """Each stand-in must miss the float64 reference by far more than the bound (or be NaN) on the inputs the GPU test uses:
    - keys t0 + i read from the poisoned cache rows instead of the qkv rows (every K: key t0 itself for K = 1 is row j's own);
    - candidate 0's rows used for every candidate (K >= 2: row 0 has no earlier row);
    - c used as the cache sequence instead of cache_seq[c] (t0 >= 1: with no cached key there is nothing to tell)."""
    nan = dtype == torch.float32
    for K in R.ROWS:
        for i, t0 in enumerate(R.BASES):
            qkv, kc, vc, _, seq = R.shared_inputs(t0, K, dtype, seed=1000 * K + i)
            ref, _, _ = R.shared_attention_ref(qkv, kc, vc, t0, seq, K, nan)
            assert bool(torch.isfinite(ref).all())

            def off(wrong, rows):
                out, _, _ = R.shared_attention_ref(qkv, kc, vc, t0, seq, K, nan, wrong=wrong)
                e = [DR.rel_err64(out[r:r + 1], ref[r:r + 1]) for r in rows]
                return min(1.0 if e_ != e_ else e_ for e_ in e)               # NaN: as wrong as it gets
            later = [c * K + j for c in range(len(seq)) for j in range(1, K)]
            if K >= 2:
                if dtype == torch.bfloat16:                                   # (the fp32 path's nan_to_num turns a NaN score into 0:
                    assert off("cache_keys", later) > 100 * BOUND             #  the value row is still NaN, checked through bf16 here)
                out, _, _ = R.shared_attention_ref(qkv, kc, vc, t0, seq, K, nan, wrong="cache_keys")
                assert all(bool(torch.isnan(out[r]).any()) or DR.rel_err64(out[r:r + 1], ref[r:r + 1]) > 100 * BOUND for r in later)
                assert off("candidate0", [r for r in later if r >= K]) > 100 * BOUND
            if t0 >= 1:
                assert off("identity_seq", range(len(seq) * K)) > 100 * BOUND, (K, t0)


def _models(batch=2):
    from helpers import tiny_config
    from kosmosx.model import Kosmos, KosmosLanguage
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    tok = torch.zeros(batch, 4, dtype=torch.long)
    img = torch.zeros(batch, 3, m.cfg.vit.image, m.cfg.vit.image)
    return [lambda cont, **kw: lm.score(tok, cont, **kw), lambda cont, **kw: m.score(tok, img, cont, **kw)]


def _cont(C=4, L=3, dtype=torch.int64):
    return torch.ones(C, L, dtype=dtype)


REFUSED = [("continuations", _cont(4, 17), {}), ("continuations", _cont(4, 0), {}), ("continuations", _cont(4, 3, torch.int32), {}),
           ("continuations", torch.ones(4, dtype=torch.int64), {}), ("continuations", torch.ones(2, 2, 2, dtype=torch.int64), {}),
           ("continuations", [[1, 2]], {}),
           ("continuation_lengths", _cont(), dict(continuation_lengths=[3, 3, 0, 3])),
           ("continuation_lengths", _cont(), dict(continuation_lengths=[3, 4, 1, 3])),
           ("continuation_lengths", _cont(), dict(continuation_lengths=[3, 3, 3])),
           ("continuation_lengths", _cont(), dict(continuation_lengths=torch.tensor([3, 3, 3, 3, 3]))),
           ("continuation_lengths", _cont(), dict(continuation_lengths=torch.tensor([1.0, 2.0, 3.0, 3.0]))),
           ("continuation_lengths", _cont(), dict(continuation_lengths=[1, 2.5, 3, 3])),
           ("prompt_index", _cont(), dict(prompt_index=[0, 1, 2, 0])), ("prompt_index", _cont(), dict(prompt_index=[0, -1, 1, 0])),
           ("prompt_index", _cont(), dict(prompt_index=[0, 1, 1])), ("prompt_index", _cont(), dict(prompt_index=[0, 1, 1, 0, 0])),
           ("prompt_index", _cont(3, 3), {})]                                            # 3 candidates, 2 prompts, no map


@pytest.mark.parametrize("name,cont,kw", REFUSED, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(REFUSED)])
def test_score_refuses_with_a_value_error_that_names_the_argument(name, cont, kw):
    """CPU tensors: the ValueError comes before the device check, hence before any launch."""
    for score in _models():
        with pytest.raises(ValueError, match=name):
            score(cont, **kw)
    # the same call without the offending argument gets as far as the device check
    for score in _models():
        with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
            score(_cont())


def test_the_limit_is_stated_as_the_k_row_steps():
    for score in _models():
        with pytest.raises(ValueError, match=r"1\.\.16.*K-row decode step"):
            score(_cont(2, 17))


def test_what_score_accepts_reaches_the_device_check():
    for score in _models():
        for cont, kw in ((_cont(4, 16), {}), (_cont(4, 1), {}), (_cont(3, 2), dict(prompt_index=[1, 1, 0])),
                         (_cont(5, 2), dict(prompt_index=[0] * 5, continuation_lengths=torch.tensor([1, 2, 1, 2, 2], dtype=torch.int32))),
                         (_cont(2, 3), dict(prompt_lengths=[2, 4], output_logits=True))):
            with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
                score(cont, **kw)


def test_check_score_args_returns_the_host_lists():
    from kosmosx import generation
    assert generation.check_score_args(2, _cont(6, 2)) == ([2] * 6, [0, 0, 0, 1, 1, 1])
    assert generation.check_score_args(3, _cont(2, 4), torch.tensor([1, 4]), (2, 0)) == ([1, 4], [2, 0])
    assert generation.MAX_SCORE_LEN == generation.MAX_STEP_ROWS == 16


def test_the_library_exports_the_score_entry_points_within_abi_7(lib):
    from kosmosx import _hip
    for name in ("kx_attention_decode_shared", "kx_decoder_score_step", "kx_token_logprob"):
        assert hasattr(lib, name) and name in _hip.SYMBOLS, name
    assert lib.kx_version() == 7 and lib.kx_struct_bytes(13) == 0 and len(_hip.STRUCT_IDS) == 13
    header = (ROOT / "include" / "kosmosx_hip.h").read_text()
    assert "KX_STRUCT_COUNT = 13" in header
    assert "int kx_attention_decode_shared(const void* qkv, const void* kcache, const void* vcache," in header   # the caches are const


def test_the_score_entry_points_validate_before_any_launch(lib):
    from kosmosx import _hip
    sh = lib.kx_attention_decode_shared
    #      qkv  kc   vc   out  odt stats C  K  H  positions cache_seq Bc Tmax prec err stream
    assert sh(256, 256, 256, 256, 0, None, 3, 4, 2, None, 256, 2, 64, 1, 256, None) == 1 and "null positions" in _hip.last_error()
    assert sh(256, 256, 256, 256, 0, None, 3, 4, 2, 256, None, 2, 64, 1, 256, None) == 1 and "cache_seq" in _hip.last_error()
    assert sh(256, 256, 256, 256, 0, None, 3, 4, 2, 256, 256, 2, 64, 1, None, None) == 1 and "error_word" in _hip.last_error()
    for K in (0, 17):
        assert sh(256, 256, 256, 256, 0, None, 3, K, 2, 256, 256, 2, 64, 1, 256, None) == 1 and f"K={K} " in _hip.last_error()
    assert sh(256, 256, 256, 256, 0, None, 0, 4, 2, 256, 256, 2, 64, 1, 256, None) == 1 and "C=0 " in _hip.last_error()
    assert sh(256, 256, 256, 256, 0, None, 3, 4, 2, 256, 256, 0, 64, 1, 256, None) == 1 and "Bc=0 " in _hip.last_error()
    assert sh(256, 256, 256, 256, 0, None, 3, 4, 2, 256, 256, 2, 0, 1, 256, None) == 1 and "Tmax=0 " in _hip.last_error()
    assert sh(None, 256, 256, 256, 0, None, 3, 4, 2, 256, 256, 2, 64, 1, 256, None) == 1 and "null pointer" in _hip.last_error()
    step = lib.kx_decoder_score_step
    w = _hip.DecoderWeights()
    #       tokens embed pos vocab max_pos shift x  C  K  positions cache_seq Bc  tables + rows   kc   vc  Tmax logits ldt ws  bytes  prec err stream
    args = [256, 256, 256, 102, 32, 0, 256, 3, 4, 256, 256, 2] + [None] * 5 + [256, 256, 30, 256, 0, 256, 1 << 20, 1, 256, None]
    assert step(None, *args) == 1 and "null pointer" in _hip.last_error()
    for K in (0, 17):
        bad = list(args)
        bad[8] = K
        assert step(C.byref(w), *bad) == 1 and f"K={K} " in _hip.last_error()
    bad = list(args)
    bad[10] = None
    assert step(C.byref(w), *bad) == 1 and "null pointer" in _hip.last_error()
    stale = _hip.DecoderWeights()
    stale.layer_bytes -= 8
    assert step(C.byref(stale), *args) == 1 and "stale binding" in _hip.last_error()
    lp = lib.kx_token_logprob
    #      logits rows_available V ld row_index target out rows stream
    assert lp(None, 4, 10, 10, None, 256, 256, 4, None) == 1 and "null pointer" in _hip.last_error()
    assert lp(256, 4, 10, 10, None, None, 256, 4, None) == 1 and "null pointer" in _hip.last_error()
    assert lp(256, 4, 10, 10, None, 256, None, 4, None) == 1 and "null pointer" in _hip.last_error()
    assert lp(256, 4, 0, 10, None, 256, 256, 4, None) == 1 and "V=0" in _hip.last_error()
    assert lp(256, 4, 10, 9, None, 256, 256, 4, None) == 1 and "ld=9" in _hip.last_error()
    assert lp(256, 4, 10, 10, None, 256, 256, 0, None) == 1 and "rows=0" in _hip.last_error()
    assert lp(256, 0, 10, 10, None, 256, 256, 4, None) == 1 and "rows_available=0" in _hip.last_error()
