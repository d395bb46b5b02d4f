"""tests/extend_ref.py (the float64 reference of kx_attention_extend) checked on the CPU against two other statements of the
same contract, and the host-only refusals of the chunked prefill: generation.check_prefill_chunk and KosmosLanguage.extend."""
import pytest
import torch

import decode_ref as DR
import extend_ref as ER

CASES = [(0, 1), (0, 5), (1, 1), (5, 33), (63, 2), (64, 64), (30, 70)]     # (P, Tn)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("P,Tn", CASES)
def test_reference_equals_successive_decode_steps(P, Tn, dtype):
    """Tn rows in one pass = Tn single-token steps at t = P, P + 1, ...: outputs and caches agree to 1e-12."""
    B, Hh, Tmax = 2, 3, 140
    qkv, kc, vc = ER.random_extend(B, Hh, Tmax, P, Tn, dtype, seed=100 * P + Tn)
    nan_to_num = dtype == torch.float32
    out, k2, v2 = ER.extend_attention_ref(qkv, kc, vc, P, nan_to_num)
    rows = qkv.reshape(B, Tn, -1)
    ks, vs = kc, vc
    for i in range(Tn):
        o, ks, vs = DR.decode_attention_ref(rows[:, i], ks, vs, P + i, nan_to_num)
        assert float((o - out.reshape(B, Tn, -1)[:, i]).abs().max()) < 1e-12, i
    assert torch.equal(DR.bits(ks), DR.bits(k2)) and torch.equal(DR.bits(vs), DR.bits(v2))
    # the poison survives where nothing was appended, and only there
    assert bool(torch.isnan(k2[:, :, P + Tn:].float()).all()) and bool(torch.isfinite(k2[:, :, :P + Tn].float()).all())
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("P,Tn", CASES)
def test_reference_equals_masked_softmax_on_the_concatenation(P, Tn):
    B, Hh, Tmax = 2, 2, 140
    qkv, kc, vc = ER.random_extend(B, Hh, Tmax, P, Tn, torch.float32, seed=7 + P + Tn)
    out, _, _ = ER.extend_attention_ref(qkv, kc, vc, P, True)
    q, kn, vn = (t.double() for t in ER.new_rows(qkv, B, Hh))
    K, V = torch.cat([kc[:, :, :P].double(), kn], 2), torch.cat([vc[:, :, :P].double(), vn], 2)
    mask = torch.ones(Tn, P + Tn, dtype=torch.bool).tril(diagonal=P)             # query i sees keys 0 .. P + i
    s = (q @ K.transpose(-1, -2)).masked_fill(~mask, float("-inf"))
    ref = (torch.softmax(s, -1) @ V).permute(0, 2, 1, 3).reshape(B * Tn, Hh * 64)
    assert float((out - ref).abs().max()) < 1e-12


def test_reference_applies_nan_to_num_to_fp32_scores_only():
    """A score beyond the fp32 range (1e20 * 1e20) is clamped to FLT_MAX: a one-hot row, finite output."""
    B, Hh, Tmax, P, Tn = 1, 1, 16, 4, 3
    qkv, kc, vc = ER.random_extend(B, Hh, Tmax, P, Tn, torch.float32, seed=3)
    qkv[1, 0] = 1e20
    kc[0, 0, 2, 0] = 1e20
    out, _, _ = ER.extend_attention_ref(qkv, kc, vc, P, True)
    assert bool(torch.isfinite(out).all())
    assert float((out[1] - vc[0, 0, 2].double()).abs().max()) < 1e-12


@pytest.mark.parametrize("bad", [0, -1, True, False, 2.0, "64", [64], 1.5])
def test_check_prefill_chunk_refuses_what_is_not_a_positive_int(bad):
    from kosmosx import generation
    with pytest.raises(ValueError, match="prefill_chunk"):
        generation.check_prefill_chunk(bad)


def test_check_prefill_chunk_accepts_none_and_positive_ints():
    from kosmosx import generation
    assert generation.check_prefill_chunk(None) is None
    assert generation.check_prefill_chunk(1) == 1 and generation.check_prefill_chunk(4096) == 4096


def _lm():
    from kosmosx.model import KosmosLanguage
    return KosmosLanguage(vocab_size=102, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=16).eval()


def test_generate_and_score_refuse_a_bad_prefill_chunk_before_the_device_check():
    lm = _lm()
    x = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="prefill_chunk"):
        lm.generate(x, 2, prefill_chunk=0)
    with pytest.raises(ValueError, match="prefill_chunk"):
        lm.score(x, torch.zeros(1, 2, dtype=torch.long), prefill_chunk=True)


def test_extend_refusals_that_need_no_device():
    lm = _lm()
    x = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(TypeError, match="torch.Tensor"):
        lm.extend([1, 2], {})
    with pytest.raises(TypeError, match="incremental_state"):
        lm.extend(x, None)
    with pytest.raises(ValueError, match=r"\[batch, new tokens\]"):
        lm.extend(x[0], {})
    with pytest.raises(ValueError, match="ragged incremental state"):
        lm.extend(x, {"len": 4, "positions": torch.zeros(1, dtype=torch.int32)})
    with pytest.raises(RuntimeError, match="not on a CUDA|no CPU fallback"):
        lm.extend(x, {})                                                     # the prefill itself: no CPU path
