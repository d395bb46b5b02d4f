"""generate(typical_p=, epsilon_cutoff=, eta_cutoff=) end to end on the device, on the tiny LM of tests/test_generate_shape_gpu.py.

``output_logits`` returns the model's own logits of every step; every emitted token is replayed on the HOST through the float64
reference sampler (tests/truncate_ref.py) on those logits, with the call's seed, the row's position and its sequence id.  A token
that is not the reference's goes through truncate_ref.check_draw (the drawn-token rule of sampling_ref.check_draw, widened by the
unsure elements); as in tests/test_generate_shape_gpu.py, whose replay is exact, no such case is allowed."""
import numpy as np
import pytest
import torch

import guidance_ref as GR
import truncate_ref as TR
from kosmosx import ops
from kosmosx.model import KosmosLanguage

pytestmark = pytest.mark.gpu

V = 502
PAD = 1
SAMPLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, seed=21)
TRUNC = [dict(typical_p=0.9), dict(epsilon_cutoff=2e-3), dict(eta_cutoff=0.02), dict(typical_p=0.95, epsilon_cutoff=3e-4, eta_cutoff=2e-3, min_p=0.02)]
ALLOWED_SHARE = 0.0                                         # of the draws that may take check_draw's "eps" branch


@pytest.fixture(scope="module")
def lm():
    m = KosmosLanguage(vocab_size=V, dim=128, depth=2, ffn_dim=256, decoder_heads=2, _seed=7, _perturb=0.1, _max_positions=64).eval().to("cuda")
    m.precision = "fp32"
    return m


def _tok(B, T, seed=4):
    return torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(seed))


def _replay(tokens, logits, kw, positions, *, seq_ids=None):
    """Every token of every row from the returned rows ``logits`` (numpy or a device tensor) through the reference sampler."""
    tokens = tokens.cpu().numpy()
    logits = logits if isinstance(logits, np.ndarray) else logits.cpu().numpy()
    B, n = tokens.shape
    names = ("temperature", "top_k", "top_p", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
    used = 0
    for b in range(B):
        for g in range(n):
            ref = TR.sample_row(logits[b, g], seed=kw["seed"], position=positions[b] + g, sequence_id=b if seq_ids is None else seq_ids[b],
                                pad_token_id=PAD, **{k: kw[k] for k in names if k in kw})
            used += TR.check_draw(int(tokens[b, g]), ref) == "eps"
    assert used <= ALLOWED_SHARE * B * n, used


@pytest.mark.parametrize("trunc", TRUNC, ids=["typical", "epsilon", "eta", "all"])
def test_plain_and_ragged_tokens_replay_and_repeat(lm, trunc):
    B, P, N = 3, 9, 10
    tok = _tok(B, P).cuda()
    kw = dict(SAMPLE, **trunc)
    got, logits = lm.generate(tok, N, output_logits=True, pad_token_id=PAD, **kw)
    assert got.shape == (B, N)
    _replay(got, logits, kw, [P] * B)
    assert torch.equal(lm.generate(tok, N, pad_token_id=PAD, **kw), got)     # a fixed seed is repeatable, with or without the logits kept
    lens = [4, 9, 6]
    rag, rlogits = lm.generate(tok, N, prompt_lengths=lens, output_logits=True, pad_token_id=PAD, **kw)
    _replay(rag, rlogits, kw, lens)
    assert torch.equal(lm.generate(tok, N, prompt_lengths=lens, pad_token_id=PAD, **kw), rag)
    for b, L in enumerate(lens):
        alone = lm.generate(tok[b:b + 1, :L].contiguous(), N, pad_token_id=PAD, sequence_ids=torch.tensor([b]), **kw)
        assert torch.equal(alone[0], rag[b]), b                              # a ragged row is the row run alone


def test_the_filters_are_real(lm):
    tok = _tok(3, 9).cuda()
    plain = lm.generate(tok, 12, pad_token_id=PAD, **SAMPLE)
    for tight in (dict(typical_p=0.2), dict(epsilon_cutoff=0.3), dict(eta_cutoff=0.6)):
        assert not torch.equal(plain, lm.generate(tok, 12, pad_token_id=PAD, **SAMPLE, **tight)), tight
    for kw in (dict(typical_p=0.2), dict(epsilon_cutoff=0.3, eta_cutoff=0.6)):
        assert torch.equal(lm.generate(tok, 8, **kw), lm.generate(tok, 8))   # ignored under greedy


def test_parallel_samples_replay_and_equal_the_prompt_repeated(lm):
    B, N, n = 2, 8, 2
    tok = _tok(B, 9).cuda()
    kw = dict(SAMPLE, **TRUNC[3])
    got, logits = lm.generate(tok, N, num_return_sequences=n, output_logits=True, pad_token_id=PAD, **kw)
    assert got.shape == (B * n, N)
    _replay(got, logits, kw, [9] * (B * n))
    assert torch.equal(got, lm.generate(tok.repeat_interleave(n, dim=0), N, pad_token_id=PAD, **kw))
    assert torch.equal(got, lm.generate(tok, N, num_return_sequences=n, pad_token_id=PAD, **kw))


def test_a_session_turn_replays(lm):
    B, P, N1, N2 = 3, 9, 6, 6
    tok = _tok(B, P)
    kw = dict(SAMPLE, **TRUNC[3])
    out1, logits1, session = lm.generate(tok.cuda(), N1, output_logits=True, pad_token_id=PAD, return_session=True, **kw)
    _replay(out1, logits1, kw, [P] * B)
    assert torch.equal(out1, lm.generate(tok.cuda(), N1, pad_token_id=PAD, **kw))
    x2 = _tok(B, 3, seed=9)
    kw2 = dict(SAMPLE, typical_p=0.8, eta_cutoff=0.01)
    out2, logits2 = session.generate(x2.cuda(), N2, output_logits=True, pad_token_id=PAD, **kw2)
    _replay(out2, logits2, kw2, [P + N1 + 3] * B)
    cat = torch.cat([tok, out1.cpu(), x2], dim=1)
    fresh = lm.generate(cat.cuda(), N2, prompt_lengths=[cat.shape[1]] * B, pad_token_id=PAD, **kw2)
    assert torch.equal(out2, fresh)


def test_guided_tokens_replay(lm):
    """The guided row is rebuilt as tests/test_generate_guidance_gpu.py does: the device's own log-probs of the two returned raw rows,
    combined by tests/guidance_ref.py."""
    B, P, N, s = 3, 9, 8, 1.5
    tok, neg = _tok(B, P).cuda(), _tok(B, 4, seed=11).cuda()
    kw = dict(SAMPLE, **TRUNC[3])
    got, cond, uncond = lm.generate(tok, N, output_logits=True, pad_token_id=PAD, guidance_scale=s, negative_prompt_ids=neg, **kw)

    def logprobs(rows):
        Rn, Vn = rows.shape
        tgt = torch.arange(Vn, dtype=torch.int64, device=rows.device).repeat(Rn)
        idx = torch.arange(Rn, dtype=torch.int32, device=rows.device).repeat_interleave(Vn)
        return ops.token_logprob(rows, tgt, row_index=idx).view(Rn, Vn).cpu().numpy()
    guided = GR.guided_row_f32(logprobs(cond.reshape(B * N, V).contiguous()), logprobs(uncond.reshape(B * N, V).contiguous()), s)
    _replay(got, guided.reshape(B, N, V), kw, [P] * B)
    assert torch.equal(lm.generate(tok, N, pad_token_id=PAD, guidance_scale=s, negative_prompt_ids=neg, **kw), got)
    assert not torch.equal(got, lm.generate(tok, N, pad_token_id=PAD, guidance_scale=s, negative_prompt_ids=neg, **SAMPLE, typical_p=0.2))


def test_with_the_defaults_nothing_is_launched(lm, monkeypatch):
    tok = _tok(3, 9).cuda()
    calls = [lambda **kw: lm.generate(tok, 6, **kw), lambda **kw: lm.generate(tok, 6, prompt_lengths=[4, 9, 6], **SAMPLE, **kw),
             lambda **kw: lm.generate(tok, 6, num_return_sequences=2, **SAMPLE, **kw)]
    before = [c() for c in calls]
    real, names = ops.H.load(), []

    class Spy:
        def __getattr__(self, name):
            names.append(name)
            return getattr(real, name)
    monkeypatch.setattr(ops.H, "load", lambda: Spy())
    for call, out in zip(calls, before):
        assert torch.equal(call(typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0), out)
        assert torch.equal(call(typical_p=1, epsilon_cutoff=0, eta_cutoff=0), out)
    assert "kx_sample_logits" in names and "kx_sample_logits_ragged" in names
    assert "kx_sample_logits_truncate" not in names and "kx_sample_logits_min_p" not in names
    lm.generate(tok, 4, min_p=0.3, **SAMPLE)                                # min_p alone: still its own entry point
    assert "kx_sample_logits_min_p" in names and "kx_sample_logits_truncate" not in names
    lm.generate(tok, 4, eta_cutoff=1e-3, **SAMPLE)
    assert names.count("kx_sample_logits_truncate") == 4                    # one launch per token, nothing else new
    assert "kx_shape_logits" not in names
