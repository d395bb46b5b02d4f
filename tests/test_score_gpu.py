"""score(): the log-likelihood of candidate continuations over a shared prompt KV cache (kosmosx.generation.score_loop), on the
tiny models of tests/test_generate_lookup_gpu.py.

Model parity and log-prob parity are checked separately, as the generate tests separate model and pick parity: the logits rows the
log-probs were taken from are returned (``output_logits``) and compared with the CPU oracle's forward over prompt ‖ continuation
at the incremental path's tolerances, and every log-prob must be the float64 log-softmax gather OF THOSE ROWS at the row kernel's
bound — so a logits difference inside the tolerance cannot hide in, or be blamed on, the log-prob arithmetic."""
import pytest
import torch

from helpers import oracle_cfg, oracle_switches, oracle_weights, rel_err, tiny_config
from kosmosx.config import Switches
from kosmosx.model import Decoder, Kosmos, KosmosLanguage
from oracle import kosmos_oracle as O

pytestmark = pytest.mark.gpu

CFG = O.DecoderCfg(layers=2, dim=256, ffn=512, heads=4, vocab=502, max_pos=64)
LP_BOUND = 2e-5         # absolute over float64: the row kernel's bound (tests/test_token_logprob_gpu.py)
PRECS = [("fp32", 2e-4), ("mixed", 1e-3)]                  # the incremental path's tolerances (tests/test_generate_lookup_gpu.py)
# measured (MI355X), worst over this file: rows vs oracle 2.0e-6 (fp32) / 1.3e-4 (mixed); rows vs generate()'s rows 1.2e-6;
# log-probs vs float64 of the returned rows 8.7e-7 (bound 2e-5)


def _lm(seed=5):
    return KosmosLanguage(vocab_size=502, dim=256, depth=2, ffn_dim=512, decoder_heads=4, _seed=seed, _perturb=0.1,
                          _max_positions=64).eval()


def _logprobs_are_the_gather_of_the_rows(lp, rows, cont, lens):
    """token_logprobs against float64 log_softmax of the RETURNED rows; padded slots exactly 0.0 in both outputs."""
    lp, rows, cont = lp.cpu(), rows.cpu(), cont.cpu()
    C, L = cont.shape
    assert lp.shape == (C, L) and lp.dtype == torch.float32 and rows.shape[:2] == (C, L) and rows.dtype == torch.float32
    want = torch.log_softmax(rows.double(), -1).gather(2, cont.clamp(0, rows.shape[2] - 1)[:, :, None])[:, :, 0]
    worst = 0.0
    for c in range(C):
        n = lens[c]
        worst = max(worst, float((lp[c, :n].double() - want[c, :n]).abs().max()))
        assert not bool(lp[c, n:].any()) and not bool(rows[c, n:].any()), c              # exactly 0.0
        assert bool((lp[c, :n] < 0).all())
    assert worst <= LP_BOUND, worst
    return worst


def _language_rows_against_the_oracle(w, prompts, pidx, cont, lens, rows, plens=None):
    """The oracle's forward over prompt ‖ continuation per candidate, at the live slots -> worst rel_err."""
    worst = 0.0
    for c in range(cont.shape[0]):
        b, n = pidx[c], lens[c]
        P = prompts.shape[1] if plens is None else plens[b]
        full = torch.cat([prompts[b, :P], cont[c, :n - 1]])[None]
        ref = O.kosmos_language_forward(w, full, CFG)[0, P - 1:]
        worst = max(worst, rel_err(rows[c, :n], ref))
    return worst


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("C,L,lens", [(4, 4, [4, 1, 3, 2]), (6, 5, [5, 2, 5, 1, 4, 3])], ids=["12_rows_streaming", "24_rows_tiles"])
def test_language_rows_against_the_oracle_and_logprobs_against_the_rows(C, L, lens, prec, tol):
    lm0 = _lm(seed=7)
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = prec
    g = torch.Generator().manual_seed(4)
    tok = torch.randint(0, 502, (2, 9), generator=g)
    cont = torch.randint(0, 502, (C, L), generator=g)
    junk = cont.clone()
    for c, n in enumerate(lens):
        junk[c, n:] = 10 ** 9                                  # padding is ignored whatever it holds: never range-checked or embedded
    lp, rows = lm.score(tok.cuda(), junk.cuda(), continuation_lengths=lens, output_logits=True)
    e = _language_rows_against_the_oracle(w, tok, [c // (C // 2) for c in range(C)], cont, lens, rows)
    elp = _logprobs_are_the_gather_of_the_rows(lp, rows, cont, lens)
    print(f"score rows vs oracle ({prec}, {C * (L - 1)} step rows): {e:.3e} (tol {tol:.0e}); log-probs vs float64 of the rows: {elp:.3e}")
    assert e < tol
    again = lm.score(tok.cuda(), junk.cuda(), continuation_lengths=torch.tensor(lens).cuda(), output_logits=True)   # (a device tensor)
    assert torch.equal(again[0], lp) and torch.equal(again[1], rows)                      # bit for bit
    assert torch.equal(lm.score(tok.cuda(), cont.cuda(), continuation_lengths=lens), lp)  # without the rows; other padding


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("alias", [True, False])
def test_kosmos_rows_against_the_oracle_forward_over_prompt_and_continuation(prec, tol, alias):
    """Both u1_inplace_alias values: under the alias a continuation token carries two position rows (pos_shift in kx_step_prepare)."""
    sw = Switches(u1_inplace_alias=alias)
    m0 = Kosmos._from_config(tiny_config(), seed=1, switches=sw, perturb=0.1).eval()
    w, cfg = oracle_weights(m0), oracle_cfg(m0.cfg)
    m = m0.to("cuda")
    m.precision = prec
    g = torch.Generator().manual_seed(5)
    Tt, C, L = 9, 4, 4
    lens = [4, 1, 3, 2]
    tok = torch.randint(0, m.cfg.vocab, (2, Tt), generator=g)
    img = torch.randn(2, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g)
    cont = torch.randint(0, m.cfg.vocab, (C, L), generator=g)
    n_img = m.cfg.perceiver.latents
    lp, rows = m.score(tok.cuda(), img.cuda(), cont.cuda(), continuation_lengths=lens, output_logits=True)
    worst = 0.0
    for c in range(C):
        b, n = c // 2, lens[c]
        text = torch.cat([tok[b], cont[c, :n - 1]])[None]
        ref = O.kosmos_forward(w, text, img[b:b + 1], cfg, oracle_switches(sw))[0, Tt + n_img - 1:]
        worst = max(worst, rel_err(rows[c, :n], ref))
    elp = _logprobs_are_the_gather_of_the_rows(lp, rows, cont, lens)
    print(f"Kosmos score rows vs oracle ({prec}, alias={alias}): {worst:.3e} (tol {tol:.0e}); log-probs: {elp:.3e}")
    assert worst < tol


def test_one_token_continuations_launch_no_step(monkeypatch):
    lm0 = _lm(seed=3)
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = "fp32"
    calls = []
    real = Decoder._device_step
    monkeypatch.setattr(Decoder, "_device_step", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    g = torch.Generator().manual_seed(8)
    tok = torch.randint(0, 502, (2, 9), generator=g)
    cont = torch.randint(0, 502, (6, 1), generator=g)
    lp, rows = lm.score(tok.cuda(), cont.cuda(), output_logits=True)
    assert not calls
    prefill = lm(tok.cuda(), incremental_state={})[:, -1]                                 # the prefill's last rows
    assert torch.equal(rows[:, 0], prefill[torch.tensor([0, 0, 0, 1, 1, 1])])
    _logprobs_are_the_gather_of_the_rows(lp, rows, cont, [1] * 6)
    assert _language_rows_against_the_oracle(w, tok, [0, 0, 0, 1, 1, 1], cont, [1] * 6, rows) < 2e-4
    lm.score(tok.cuda(), torch.randint(0, 502, (2, 2), generator=g).cuda())
    assert calls == [1]                                                                   # (the counter does count)


@pytest.mark.parametrize("prec,tol", PRECS)
def test_an_unordered_prompt_index_and_ragged_prompts(prec, tol):
    lm0 = _lm(seed=9)
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = prec
    g = torch.Generator().manual_seed(6)
    tok = torch.randint(0, 502, (3, 9), generator=g)
    cont = torch.randint(0, 502, (5, 3), generator=g)
    lens = [3, 2, 3, 1, 3]
    pidx = [2, 0, 2, 0, 0]                                     # unordered, repeated, prompt 1 unused
    lp, rows = lm.score(tok.cuda(), cont.cuda(), continuation_lengths=lens, prompt_index=pidx, output_logits=True)
    e = _language_rows_against_the_oracle(w, tok, pidx, cont, lens, rows)
    _logprobs_are_the_gather_of_the_rows(lp, rows, cont, lens)
    assert e < tol
    # ragged prompts: the oracle runs on the unpadded prompts; the padding holds ids that would fail the range check
    plens = [9, 4, 6]
    padded = tok.clone()
    for b, n in enumerate(plens):
        padded[b, n:] = 10 ** 9
    lp2, rows2 = lm.score(padded.cuda(), cont.cuda(), continuation_lengths=lens, prompt_index=pidx, prompt_lengths=plens,
                          output_logits=True)
    e2 = _language_rows_against_the_oracle(w, tok, pidx, cont, lens, rows2, plens=plens)
    _logprobs_are_the_gather_of_the_rows(lp2, rows2, cont, lens)
    print(f"score with prompt_index ({prec}): {e:.3e}; with ragged prompts: {e2:.3e} (tol {tol:.0e})")
    assert e2 < tol


def test_permuting_the_candidates_permutes_the_outputs_bit_for_bit():
    lm = _lm(seed=2).to("cuda")
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, 502, (2, 9), generator=g).cuda()
    cont = torch.randint(0, 502, (4, 4), generator=g)
    lens, pidx = [4, 2, 3, 4], [0, 1, 1, 0]
    lp, rows = lm.score(tok, cont.cuda(), continuation_lengths=lens, prompt_index=pidx, output_logits=True)
    perm = [2, 0, 3, 1]
    lp2, rows2 = lm.score(tok, cont[perm].cuda(), continuation_lengths=[lens[p] for p in perm], prompt_index=[pidx[p] for p in perm],
                          output_logits=True)
    assert torch.equal(lp2, lp[perm]) and torch.equal(rows2, rows[perm])


@pytest.mark.parametrize("prec,tol", PRECS)
def test_score_of_generated_tokens_agrees_with_generate(prec, tol):
    """Not bitwise: generate() steps one row per sequence, score() five — the step may take another GEMM path."""
    lm = _lm(seed=4).to("cuda")
    lm.precision = prec
    tok = torch.randint(0, 502, (2, 9), generator=torch.Generator().manual_seed(1)).cuda()
    got, logits = lm.generate(tok, 6, output_logits=True)
    lp, rows = lm.score(tok, got, output_logits=True)
    e = rel_err(rows, logits)
    print(f"score rows vs generate rows ({prec}): {e:.3e} (tol {tol:.0e})")
    assert e < tol
    _logprobs_are_the_gather_of_the_rows(lp, rows, got, [6, 6])


def test_the_budget_and_the_vocabulary_are_checked_and_the_next_call_succeeds():
    lm = _lm(seed=1).to("cuda")
    g = torch.Generator().manual_seed(2)
    tok = torch.randint(0, 502, (2, 9), generator=g).cuda()
    cont = torch.randint(0, 502, (2, 3), generator=g).cuda()
    good = lm.score(tok, cont)
    long_prompt = torch.randint(0, 502, (2, 60), generator=g).cuda()                      # 60 + 2 fed tokens = the 62-row table: fits
    assert bool(torch.isfinite(lm.score(long_prompt, cont)).all())
    with pytest.raises(IndexError, match="position table"):
        lm.score(torch.randint(0, 502, (2, 61), generator=g).cuda(), cont)               # 61 + 2 > 62
    assert torch.equal(lm.score(tok, cont), good)
    bad = cont.clone()
    bad[1, 1] = 502
    with pytest.raises(IndexError, match="index out of range"):
        lm.score(tok, bad)
    assert torch.equal(lm.score(tok, cont), good)
    bad[1, 1] = -1
    with pytest.raises(IndexError, match="index out of range"):
        lm.score(tok, bad, continuation_lengths=[3, 3])
    assert torch.equal(lm.score(tok, bad, continuation_lengths=[3, 1]), lm.score(tok, cont, continuation_lengths=[3, 1]))
