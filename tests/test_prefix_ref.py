"""Parallel sampling without a GPU: the float64 reference of tests/prefix_ref.py against an independent restatement, the GPU tests'
inputs against the stand-ins a broken kernel would compute, generate()'s refusals around ``num_return_sequences`` (which come before
the device check), and the library's two new entry points, which validate before any launch."""
import ctypes as C
from pathlib import Path

import pytest
import torch

import decode_ref as DR
import prefix_ref as R

ROOT = Path(__file__).resolve().parent.parent
BOUND = 2e-5                                                # what tests/test_attention_decode_prefix_gpu.py holds the kernel to


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from kosmosx import _hip
    return _hip.load()


def test_the_reference_is_a_softmax_over_prefix_tail_and_new_key():
    for i, (P, fill) in enumerate([(0, 0), (0, 5), (1, 0), (3, 1), (130, 17), ([0, 2, 5, 1, 7], [3, 0, 1, 2, 4])]):
        qkv, kp, vp, kt, vt, pos, seq, plen = R.prefix_inputs(P, fill, torch.float32, seed=7 + i)
        out, kt2, vt2 = R.prefix_attention_ref(qkv, kp, vp, kt, vt, pos, seq, plen, nan_to_num=True)
        assert out.dtype == torch.float64 and bool(torch.isfinite(out).all())
        _, kn, vn = DR.new_token(qkv, R.HH)
        for r in range(R.M):
            t, c, p = int(pos[r]), int(seq[r]), int(plen[r])
            want = R.direct_attention(qkv, kp, vp, kt, vt, t, c, p, r)
            assert float((out[r] - want).abs().max()) < 1e-12, (P, fill, r)
            # the append: tail row t - P holds the new k | v, every other tail row its bits
            assert torch.equal(kt2[r, :, t - p], kn[r]) and torch.equal(vt2[r, :, t - p], vn[r])
            keep = torch.arange(R.TTAIL) != t - p
            assert torch.equal(DR.bits(kt2[r][:, keep]), DR.bits(kt[r][:, keep]))
            assert torch.equal(DR.bits(vt2[r][:, keep]), DR.bits(vt[r][:, keep]))


def test_the_assembled_cache_is_prefix_rows_then_tail_rows():
    qkv, kp, vp, kt, vt, pos, seq, plen = R.prefix_inputs([2, 0, 3, 1, 2], [1, 4, 0, 2, 3], torch.float32, seed=1)
    priv = R.assemble(kp, kt, pos, seq, plen)
    assert tuple(priv.shape) == (R.M, R.HH, R.TMAX, 64)
    for r in range(R.M):
        t, c, p = int(pos[r]), int(seq[r]), int(plen[r])
        assert torch.equal(priv[r, :, :p], kp[c, :, :p]) and torch.equal(priv[r, :, p:t], kt[r, :, :t - p])
        assert bool(torch.isnan(priv[r, :, t:]).all()) and bool(torch.isfinite(priv[r, :, :t]).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_gpu_inputs_tell_the_wrong_kernels_from_the_right_one(dtype):
    """Each stand-in must miss the float64 reference by far more than the bound (or be NaN) on every input of the GPU test on which
    it differs from the contract at all:
    - the tail indexed at j instead of j - P (P >= 1 and a tail key: with P = 0 the two are the same row);
    - prefix sequence r instead of prefix_seq[r] (P >= 1, the rows r whose r mod Bp is another sequence);
    - key t read from the (poisoned) tail row instead of the qkv row (every input);
    - the prefix stopped one key early (P >= 1)."""
    nan = dtype == torch.float32
    other = [r for r in range(R.M) if r % R.BP != R.PREFIX_SEQ[r]]
    assert len(other) >= 2
    for i, (P, fill) in enumerate(R.CASES):
        qkv, kp, vp, kt, vt, pos, seq, plen = R.prefix_inputs(P, fill, dtype, seed=100 + i)
        ref, _, _ = R.prefix_attention_ref(qkv, kp, vp, kt, vt, pos, seq, plen, nan)
        assert bool(torch.isfinite(ref).all())

        def off(wrong, rows):
            out, _, _ = R.prefix_attention_ref(qkv, kp, vp, kt, vt, pos, seq, plen, nan, wrong=wrong)
            e = [DR.rel_err64(out[r:r + 1], ref[r:r + 1]) for r in rows]
            return min(1.0 if e_ != e_ else e_ for e_ in e)                   # NaN: as wrong as it gets
        assert off("key_t_from_tail", range(R.M)) > 100 * BOUND, (P, fill)
        if P >= 1:
            assert off("identity_seq", other) > 100 * BOUND, (P, fill)
            assert off("prefix_short", range(R.M)) > 100 * BOUND, (P, fill)
            if fill >= 1:
                assert off("tail_at_j", range(R.M)) > 100 * BOUND, (P, fill)


def _models(batch=2):
    from helpers import tiny_config
    from kosmosx.model import Kosmos, KosmosLanguage
    lm = KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    tok = torch.zeros(batch, 4, dtype=torch.long)
    img = torch.zeros(batch, 3, m.cfg.vit.image, m.cfg.vit.image)
    return [lambda **kw: lm.generate(tok, 4, **kw), lambda **kw: m.generate(tok, img, 4, **kw)]


REFUSED = [("greedy", dict(num_return_sequences=2)),
           ("prompt_lookup", dict(num_return_sequences=2, do_sample=True, prompt_lookup_num_tokens=2)),
           ("return_session", dict(num_return_sequences=3, do_sample=True, return_session=True))]


@pytest.mark.parametrize("what,kw", REFUSED, ids=[n for n, _ in REFUSED])
def test_generate_refuses_with_a_value_error_that_names_num_return_sequences(what, kw):
    """CPU tensors: the ValueError comes before the device check, hence before any launch."""
    for gen in _models():
        with pytest.raises(ValueError, match="num_return_sequences"):
            gen(**kw)


def test_parallel_sampling_reaches_the_device_check():
    for gen in _models():
        for kw in (dict(num_return_sequences=2, do_sample=True),
                   dict(num_return_sequences=3, do_sample=True, top_k=5, temperature=0.7, prompt_lengths=[3, 4], output_logits=True),
                   dict(num_return_sequences=2, do_sample=True, sequence_ids=torch.arange(4), no_repeat_ngram_size=2)):
            with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
                gen(**kw)


def test_the_refusal_with_beams_stays():
    for gen in _models():
        with pytest.raises(ValueError, match="num_return_sequences = 5 exceeds num_beams = 4"):
            gen(num_beams=4, num_return_sequences=5)
        with pytest.raises(ValueError, match="num_return_sequences"):
            gen(num_return_sequences=0)


def test_check_parallel_args_returns_the_samples_per_prompt():
    from kosmosx import generation
    assert generation.check_parallel_args(num_return_sequences=1) == 1
    assert generation.check_parallel_args(num_return_sequences=4) == 4
    assert generation.check_parallel_args(num_return_sequences=4, beams=True, return_session=True) == 1   # beam search's own business
    assert generation.check_beam_args(100, num_beams=1, num_return_sequences=4, do_sample=True) is False


def test_the_library_exports_the_prefix_entry_points_within_abi_7(lib):
    from kosmosx import _hip
    header = (ROOT / "include" / "kosmosx_hip.h").read_text()
    for name in ("kx_attention_decode_prefix", "kx_decoder_decode_step_prefix"):
        assert hasattr(lib, name) and name in _hip.SYMBOLS and f"int {name}(" in header, name
    assert lib.kx_version() == 7 and lib.kx_struct_bytes(13) == 0 and len(_hip.STRUCT_IDS) == 13
    assert "KX_STRUCT_COUNT = 13" in header
    assert "int kx_attention_decode_prefix(const void* qkv, const void* kprefix, const void* vprefix, void* ktail" in header   # const


def test_the_prefix_entry_points_validate_before_any_launch(lib):
    from kosmosx import _hip
    at = lib.kx_attention_decode_prefix
    #       qkv  kp   vp   kt   vt   out odt stats M  H  pos  seq  len  Bp Tmax Ttail prec err stream
    good = [256, 256, 256, 256, 256, 256, 0, None, 5, 2, 256, 256, 256, 2, 64, 8, 1, 256, None]

    def bad(i, v):
        a = list(good)
        a[i] = v
        return at(*a)
    for i in range(6):
        assert bad(i, None) == 1 and "null pointer" in _hip.last_error(), i
    for i, name in ((10, "positions"), (11, "prefix_seq"), (12, "prefix_len"), (17, "error_word")):
        assert bad(i, None) == 1 and name in _hip.last_error(), name
    for M in (0, 65536):
        assert bad(8, M) == 1 and f"M={M} " in _hip.last_error()
    assert bad(9, 65536) == 1 and "H=65536 " in _hip.last_error()
    for i, name in ((13, "Bp"), (14, "Tmax"), (15, "Ttail")):
        for v in (0, 1 << 31):
            assert bad(i, v) == 1 and f"{name}={v}" in _hip.last_error(), (name, v)
    step = lib.kx_decoder_decode_step_prefix
    w = _hip.DecoderWeights()
    #       tokens embed pos vocab max_pos shift x   M  pos  seq  len Bp  tables + rows   kp   vp  Tmax kt   vt  Ttail logits ldt ws  bytes  prec err stream
    args = [256, 256, 256, 102, 32, 0, 256, 6, 256, 256, 256, 2] + [None] * 5 + [256, 256, 30, 256, 256, 8, 256, 0, 256, 1 << 20, 1, 256, None]
    assert step(None, *args) == 1 and "null pointer" in _hip.last_error()
    for i in (8, 9, 10, 17, 18, 20, 21, 28):                # positions, prefix_seq, prefix_len, the four caches, error_word
        a = list(args)
        a[i] = None
        assert step(C.byref(w), *a) == 1 and "null pointer" in _hip.last_error(), i
    for i, name, vals in ((7, "M", (0, 65536)), (11, "Bp", (0, 1 << 31)), (19, "Tmax", (0, 1 << 31)), (22, "Ttail", (0, 1 << 31))):
        for v in vals:
            a = list(args)
            a[i] = v
            assert step(C.byref(w), *a) == 1 and f"{name}={v}" in _hip.last_error(), (name, v)
    stale = _hip.DecoderWeights()
    stale.layer_bytes -= 8
    assert step(C.byref(stale), *args) == 1 and "stale binding" in _hip.last_error()
