"""generate(penalty_alpha=, top_k=) end to end on the device, in the precisions "fp32" and "mixed", on the tiny LM of the neighbouring
tests and on the tiny multimodal model.

top_k = 1 is plain greedy decoding, bit for bit.  For k > 1 a host-driven restatement reproduces ``output_logits`` bit for bit from
existing pieces alone — the caches repeated k times, the ragged decode step at B * k rows on the trace's candidates, torch indexing
to keep the chosen row's caches — so a wrong tail address, commit or position shows from the second token on.  The trace is checked
against ops.step_logprobs on the returned logits and against tests/contrast_ref.py over the returned history."""
import numpy as np
import pytest
import torch

import contrast_ref as R
from helpers import tiny_config
from kosmosx import generation as G
from kosmosx import ops
from kosmosx.model import Kosmos, KosmosLanguage

pytestmark = pytest.mark.gpu
V, D, PAD, N = 102, 128, 1, 12
STEP = ["kx_contrast_candidates", "kx_decoder_decode_step_prefix", "kx_contrast_hidden", "kx_contrast_select", "kx_kv_cache_commit"]
NEW = set(STEP) - {"kx_decoder_decode_step_prefix"} | {"kx_contrast_scratch_bytes"}


@pytest.fixture(scope="module", params=["fp32", "mixed"])
def lm(request):
    m = KosmosLanguage(vocab_size=V, dim=128, depth=2, ffn_dim=256, decoder_heads=2, _seed=7, _perturb=0.1, _max_positions=64).eval().to("cuda")
    m.precision = request.param
    return m


def _tok(B, T, seed=4):
    return torch.randint(2, V, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()


LENS = {1: [6], 2: [9, 4], 3: [5, 9, 1]}


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_one_candidate_is_greedy_decoding_bit_for_bit(lm, ragged):
    tok = _tok(3, 9)
    kw = dict(prompt_lengths=LENS[3]) if ragged else {}
    want, wl = lm.generate(tok, N, output_logits=True, **kw)
    got, gl, tr = lm.generate(tok, N, penalty_alpha=0.6, top_k=1, output_logits=True, output_contrast=True, **kw)
    assert torch.equal(got, want)
    assert torch.equal(gl.view(torch.int32), wl.view(torch.int32))
    assert not tr["chosen"].any() and torch.equal(tr["candidate_id"][:, :, 0], got)


def test_alpha_zero_always_takes_the_most_likely_candidate(lm):
    tok = _tok(2, 7)
    got, tr = lm.generate(tok, N, penalty_alpha=0.0, top_k=5, output_contrast=True)
    assert not tr["chosen"].any() and torch.equal(got, tr["candidate_id"][:, :, 0])
    assert torch.equal(got, lm.generate(tok, N))                           # ... which is greedy decoding


def _restate(lm, tok, lens, k, cand_id, chosen):
    """``output_logits`` of the contrastive call from existing pieces: the prefill at B rows, its caches repeated k times, the ragged
    step at B * k rows on the trace's candidates, the chosen row's caches kept by torch indexing."""
    dec, prec = lm.decoder, lm.precision
    B, n = chosen.shape
    M = B * k
    tokens = G.mask_padding(tok[:, :max(lens)].long(), lens)
    state = {"max_len": tokens.shape[1] + n}
    logits = dec._forward_incremental(tokens, state, None, prec)
    ar = torch.arange(B, device="cuda")
    cur = logits[ar, torch.tensor(lens, device="cuda") - 1]
    state["kcache"] = state["kcache"].repeat_interleave(k, dim=1).contiguous()
    state["vcache"] = state["vcache"].repeat_interleave(k, dim=1).contiguous()
    positions = torch.tensor(lens, dtype=torch.int32, device="cuda").repeat_interleave(k).contiguous()
    state.update(batch=M, positions=positions, pos_max=max(lens))
    dec._ragged_scratch(state, "cuda", rows=M)
    cols = []
    for g in range(n):
        cols.append(cur)
        lg = dec._forward_incremental(None, state, None, prec, next_token=cand_id[:, g].reshape(M).contiguous())[:, 0]
        src = (ar * k + chosen[:, g].long()).repeat_interleave(k)
        state["kcache"], state["vcache"] = state["kcache"][:, src].contiguous(), state["vcache"][:, src].contiguous()
        positions += 1
        cur = lg[ar * k + chosen[:, g].long()]
    assert int(state["error"].item()) == 0
    return torch.stack(cols, 1)


def _check_trace(tokens, logits, tr, lens, k, alpha, dim=D):
    """The trace against ops.step_logprobs on the returned logits and against float64 over the returned history."""
    B, n = tokens.shape
    cid, cpr, cpen, ch = (tr[x].cpu().numpy() for x in ("candidate_id", "candidate_prob", "candidate_penalty", "chosen"))
    hist = tr["history"].cpu().numpy()
    assert tr["candidate_id"].dtype == torch.int64 and tr["chosen"].dtype == torch.int32 and tr["history_len"].dtype == torch.int32
    assert cid.shape == cpr.shape == cpen.shape == (B, n, k) and ch.shape == (B, n) and hist.shape[0] == B and hist.shape[2] == dim
    lp, top_lp, top_id = (torch.zeros(B, 1, device="cuda"), torch.zeros(B, 1, k, device="cuda"),
                          torch.zeros(B, 1, k, dtype=torch.int64, device="cuda"))
    tol = 2 * dim * 2.0 ** -24
    close = 0
    for g in range(n):
        ops.step_logprobs(logits[:, g].contiguous(), tokens[:, g].contiguous(), out=lp, col=0, top_n=k, top_out=top_lp, top_ids=top_id)
        assert np.array_equal(cid[:, g], top_id[:, 0].cpu().numpy())
        want = np.exp(top_lp[:, 0].double().cpu().numpy())
        assert (np.abs(cpr[:, g].astype(np.float64) - want) <= 4 * 2.0 ** -23 * want).all()          # 4 ulp through the expf
        for b in range(B):
            P = lens[b] + g
            j = int(ch[b, g])
            # the chosen candidate's unit vector is history row P; the others' are not kept, so the penalty of the chosen one is
            # what float64 can restate from the returned history
            want_pen = float(R.penalty(hist[b, P][None], hist[b, :P])[0])
            assert abs(float(cpen[b, g, j]) - want_pen) <= tol, (b, g, cpen[b, g, j], want_pen)
            s32 = R.scores_fp32(cpr[b, g], cpen[b, g], alpha)
            assert j == R.choose(s32), (b, g)                              # the fp32 restatement on the device's own values: exact
            s64 = R.scores(cpr[b, g], cpen[b, g], alpha)
            if R.best_gap(s64) > 2 * alpha * tol:                          # (below the penalties' own error bound float64 decides nothing)
                assert j == R.choose(s64), (b, g)
            else:
                close += 1
            assert int(tokens[b, g]) == int(cid[b, g, j])
    print(f"B={B} k={k}: {close} of {B * n} choices closer than the penalty's error bound")
    assert tr["history_len"].tolist() == [l + n for l in lens]
    norms = np.linalg.norm(hist[0, :lens[0] + n].astype(np.float64), axis=1)
    assert np.abs(norms - 1.0).max() < 1e-6


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("B,k", [(1, 2), (2, 3), (3, 6)])
def test_the_plumbing_exactly_and_the_trace(lm, B, k, ragged):
    """M = 2 (the residual pair), 6 (streaming) and 18 (tile GEMMs)."""
    tok = _tok(B, 9, seed=R.GENERATE_SEEDS[(B, k)])
    lens = LENS[B] if ragged else [9] * B
    got, logits, tr = lm.generate(tok, N, penalty_alpha=R.ALPHA, top_k=k, output_logits=True, output_contrast=True,
                                  **(dict(prompt_lengths=lens) if ragged else {}))
    assert tuple(got.shape) == (B, N) and tuple(logits.shape) == (B, N, V)
    want = _restate(lm, tok, lens, k, tr["candidate_id"], tr["chosen"])
    assert torch.equal(logits.view(torch.int32), want.view(torch.int32))
    _check_trace(got, logits, tr, lens, k, R.ALPHA)
    if k > 2:
        assert tr["chosen"].any()                                          # the penalty does overrule the most likely candidate somewhere
    again = lm.generate(tok, N, penalty_alpha=R.ALPHA, top_k=k, **(dict(prompt_lengths=lens) if ragged else {}))
    assert torch.equal(again, got)                                         # without the outputs: the same tokens


def test_an_eos_finishes_its_row_and_leaves_the_others_alone(lm):
    tok, lens, k = _tok(3, 9, seed=11), LENS[3], 3
    free, ftr = lm.generate(tok, N, penalty_alpha=R.ALPHA, top_k=k, prompt_lengths=lens, output_contrast=True)
    free = free.cpu()
    row, at = 1, 5
    eos = int(free[row, at])
    first = {b: next((g for g in range(N) if int(free[b, g]) == eos), None) for b in range(3)}
    got, tr = lm.generate(tok, N, penalty_alpha=R.ALPHA, top_k=k, prompt_lengths=lens, eos_token_id=eos, pad_token_id=PAD, eos_poll=4,
                          output_contrast=True)
    got = got.cpu()
    for b in range(3):
        stop = first[b]
        if stop is None:
            assert torch.equal(got[b], free[b, :got.shape[1]])
        else:
            assert torch.equal(got[b, :stop + 1], free[b, :stop + 1]) and (got[b, stop + 1:] == PAD).all()
            assert (tr["chosen"][b, stop + 1:] == -1).all() and (tr["candidate_id"][b, stop + 1:] == -1).all()
    assert first[row] is not None and first[row] <= at
    emitted = [N if first[b] is None else first[b] + 1 for b in range(3)]
    assert tr["history_len"].tolist() == [l + min(e, got.shape[1]) for l, e in zip(lens, emitted)]


def test_the_multimodal_model_with_an_image():
    m = Kosmos._from_config(tiny_config(), seed=0, perturb=0.1).eval().to("cuda")
    g = torch.Generator().manual_seed(2)
    B, k, n = 2, 3, 8
    tok = torch.randint(2, m.cfg.vocab, (B, 7), generator=g).cuda()
    img = torch.randn(B, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g).cuda()
    lens = [7, 4]
    got, logits, tr = m.generate(tok, img, n, penalty_alpha=R.ALPHA, top_k=k, prompt_lengths=lens, output_logits=True, output_contrast=True)
    n_img = int(tr["history_len"][0]) - lens[0] - n                        # the image rows are ordinary history rows
    assert n_img > 0
    _check_trace(got, logits, tr, [l + n_img for l in lens], k, R.ALPHA, dim=tr["history"].shape[2])


def test_the_launch_list_per_token_and_nothing_new_without_the_keyword(lm, monkeypatch):
    tok = _tok(2, 7)
    plain = lm.generate(tok, 6)
    real, names = ops.H.load(), []

    class Spy:
        def __getattr__(self, name):
            names.append(name)
            return getattr(real, name)
    monkeypatch.setattr(ops.H, "load", lambda: Spy())
    assert torch.equal(lm.generate(tok, 6, penalty_alpha=None), plain)
    assert not NEW & set(names) and "kx_decoder_decode_step_prefix" not in names
    del names[:]
    lm.generate(tok, 6, penalty_alpha=0.6, top_k=4, output_contrast=True)
    seen = [x for x in names if x in STEP]
    assert seen == ["kx_contrast_hidden"] + STEP * 6                       # the history from the prefill, then five fetches per token
    assert names.count("kx_contrast_scratch_bytes") == 1 and not [x for x in names if x.startswith("kx_sample_logits")]
