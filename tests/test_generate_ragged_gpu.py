"""Ragged generate(): every row of a batch at its own, device-resident position (``prompt_lengths``).

The contract is "each row generates what it would generate alone": the logits a row's tokens were drawn from are compared with
the CPU oracle's forward over THAT ROW's unpadded prompt + generated tokens (teacher forced) at the tolerances the uniform
generate tests use for the same arithmetic, and the tokens with the CPU restatement of the sampler on those logits, at the
row's own Philox position len_b + g and with the row's own history.  The per-row-position kernels are also checked on their
own, bit for bit against their uniform forms."""
import numpy as np
import pytest
import torch

import sampling_ref as R
from helpers import oracle_cfg, oracle_switches, oracle_weights, rel_err, tiny_config
from kosmosx import _hip as H
from kosmosx import ops
from kosmosx.config import Switches
from kosmosx.model import Kosmos, KosmosLanguage
from oracle import kosmos_oracle as O

pytestmark = pytest.mark.gpu

EPS_P, EPS_G = 1e-5, 1e-4
SAMPLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, repetition_penalty=1.2, seed=21)
KWS = pytest.mark.parametrize("kw", [dict(), SAMPLE], ids=["greedy", "sampled"])
PRECS = pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("mixed", 1e-3)])


def _lm(seed=5, max_pos=64):
    return KosmosLanguage(vocab_size=502, dim=256, depth=2, ffn_dim=512, decoder_heads=4, _seed=seed, _perturb=0.1,
                          _max_positions=max_pos).eval()


def _cfg(max_pos=64):
    return O.DecoderCfg(layers=2, dim=256, ffn=512, heads=4, vocab=502, max_pos=max_pos)


def _row_sampler_parity(tokens, logits, prompts, starts, seq_ids, kw):
    """Every token of every row against the reference sampler on the returned logits: position starts[b] + g, the row's own
    prompt (never the padding) as history.  At most 1 % of the draws may take check_draw's epsilon branch."""
    tokens, logits = tokens.cpu().numpy(), logits.cpu().numpy()
    B, n = tokens.shape
    used = 0
    for b in range(B):
        for g in range(n):
            ref = R.sample_row(logits[b, g], temperature=kw.get("temperature", 1.0), top_k=kw.get("top_k", 0),
                               top_p=kw.get("top_p", 1.0), repetition_penalty=kw.get("repetition_penalty", 1.0),
                               do_sample=kw.get("do_sample", False), seed=kw.get("seed", 0), position=starts[b] + g,
                               sequence_id=seq_ids[b], history=np.concatenate([prompts[b], tokens[b, :g]]))
            used += R.check_draw(int(tokens[b, g]), ref, EPS_P, EPS_G, kw.get("top_p", 1.0)) == "eps"
    assert used <= 0.01 * B * n, used


def _language_contract(lm, w, cfg, tok, lens, n, kw, tol, seq_ids=None):
    ids = None if seq_ids is None else torch.tensor(seq_ids).cuda()
    got, logits = lm.generate(tok.cuda(), n, output_logits=True, prompt_lengths=lens, sequence_ids=ids, **kw)
    B = tok.shape[0]
    assert got.shape == (B, n) and logits.shape == (B, n, 502) and logits.dtype == torch.float32
    assert int(got.min()) >= 0 and int(got.max()) < 502
    for b, L in enumerate(lens):
        full = torch.cat([tok[b, :L], got[b, :-1].cpu()])[None]
        ref = O.kosmos_language_forward(w, full, cfg)[0, L - 1:]
        e = rel_err(logits[b], ref)
        print(f"ragged generate, row {b} (len {L}) logits vs the oracle on the row alone: {e:.3e}")
        assert e < tol, (b, L, e)
    _row_sampler_parity(got, logits, [tok[b, :L].numpy() for b, L in enumerate(lens)], lens,
                        list(range(B)) if seq_ids is None else seq_ids, kw)
    again = lm.generate(tok.cuda(), n, prompt_lengths=torch.tensor(lens).cuda(), sequence_ids=ids, **kw)   # (a device tensor this time)
    assert torch.equal(again, got)
    return got, logits


# ---- 1. uniform lengths through the per-row-position kernels: the old path's bits -----------------------------------------------
@PRECS
@KWS
def test_uniform_lengths_give_the_bits_of_the_call_without_them(prec, tol, kw):
    lm = _lm(seed=7).to("cuda")
    lm.precision = prec
    B, P, n = 3, 9, 20
    tok = torch.randint(0, 502, (B, P), generator=torch.Generator().manual_seed(4)).cuda()
    want, want_logits = lm.generate(tok, n, output_logits=True, **kw)
    got, got_logits = lm.generate(tok, n, output_logits=True, prompt_lengths=[P] * B, **kw)
    assert torch.equal(got, want)
    assert torch.equal(got_logits, want_logits)


# ---- 2. the attention kernel ---------------------------------------------------------------------------------------------------
# 16 slots; 128 (fp32) / 256 (bf16) keys in flight per round: slot boundaries, round boundaries, the second-round reload
POSITIONS = [0, 1, 15, 16, 17, 127, 128, 129, 255, 256]


@pytest.mark.parametrize("dtype,odt", [(torch.float32, "f32"), (torch.float32, "f16c"), (torch.float32, "f16p"),
                                       (torch.bfloat16, "bf16")], ids=["fp32", "fp32-f16c", "fp32-f16p", "bf16"])
def test_attention_decode_ragged_against_the_uniform_kernel(dtype, odt):
    Hh, Tmax, B = 4, 320, len(POSITIONS)
    D = Hh * 64
    g = torch.Generator().manual_seed(11)
    kc = torch.randn(B, Hh, Tmax, 64, generator=g).to(dtype).cuda()
    vc = torch.randn(B, Hh, Tmax, 64, generator=g).to(dtype).cuda()
    qkv = torch.randn(B, 3 * D, generator=g).to(dtype).cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")

    def stats():
        return torch.zeros(B, Hh, 2, device="cuda")
    # equal positions: the bits of kx_attention_decode at that t, outputs, statistics and caches
    for t in (17, 129, 256):
        k1, v1, k2, v2, s1, s2 = kc.clone(), vc.clone(), kc.clone(), vc.clone(), stats(), stats()
        want = ops.attention_decode(qkv, k1, v1, t, out_dtype=odt, stats_out=s1)
        got = ops.attention_decode(qkv, k2, v2, positions=torch.full((B,), t, dtype=torch.int32, device="cuda"), error_word=err,
                                   out_dtype=odt, stats_out=s2)
        assert torch.equal(got, want) and torch.equal(s2, s1) and torch.equal(k2, k1) and torch.equal(v2, v1), t
    # unequal positions: row b = the B = 1 launch at t = positions[b] on that row's cache
    pos = torch.tensor(POSITIONS, dtype=torch.int32, device="cuda")
    k2, v2, s2 = kc.clone(), vc.clone(), stats()
    got = ops.attention_decode(qkv, k2, v2, positions=pos, error_word=err, out_dtype=odt, stats_out=s2)
    for b, t in enumerate(POSITIONS):
        k1, v1, s1 = kc[b:b + 1].clone(), vc[b:b + 1].clone(), torch.zeros(1, Hh, 2, device="cuda")
        want = ops.attention_decode(qkv[b:b + 1].contiguous(), k1, v1, t, out_dtype=odt, stats_out=s1)
        assert torch.equal(got[b], want[0]) and torch.equal(s2[b], s1[0]), (b, t)
        assert torch.equal(k2[b], k1[0]) and torch.equal(v2[b], v1[0]), (b, t)
        # the appended row is row positions[b] — the new token's k | v — and no other row moved
        assert torch.equal(k2[b, :, t], qkv[b, D:2 * D].view(Hh, 64)) and torch.equal(v2[b, :, t], qkv[b, 2 * D:].view(Hh, 64))
        keep = torch.ones(Tmax, dtype=torch.bool, device="cuda")
        keep[t] = False
        assert torch.equal(k2[b][:, keep], kc[b][:, keep]) and torch.equal(v2[b][:, keep], vc[b][:, keep])
    assert int(err.item()) == 0
    # a position outside the cache: that row writes nothing and the sticky word says so; the other rows are served
    bad = pos.clone()
    bad[3] = Tmax
    bad[6] = -1
    k3, v3 = kc.clone(), vc.clone()
    out3 = ops.attention_decode(qkv, k3, v3, positions=bad, error_word=err, out_dtype=odt)
    assert int(err.item()) == H.KX_RAGGED_ERR_CACHE
    for b in (3, 6):
        assert torch.equal(k3[b], kc[b]) and torch.equal(v3[b], vc[b]) and not bool(out3[b].any())
    for b in (0, 5, 9):
        assert torch.equal(out3[b], got[b]) and torch.equal(k3[b], k2[b])
    ops.attention_decode(qkv, k3, v3, positions=pos, error_word=err, out_dtype=odt)
    assert int(err.item()) == H.KX_RAGGED_ERR_CACHE                        # sticky: a later good launch does not clear it


# ---- 3. the step-prepare kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_shift", [0, 8], ids=["language", "n_img"])
def test_step_prepare_against_embed_step_and_index_select(pos_shift):
    g = torch.Generator().manual_seed(12)
    V, d, rows = 502, 256, 62
    embed = torch.randn(V, d, generator=g).cuda()
    pos = torch.randn(rows + 2, d, generator=g).cuda()
    tables = [torch.randn(rows, 32, generator=g).cuda() for _ in range(4)]
    positions = [8, 9, 23, 40, 61] if pos_shift else [0, 1, 23, 40, 61]
    B = len(positions)
    tokens = torch.randint(0, V, (B,), generator=g).cuda()
    p = torch.tensor(positions, dtype=torch.int32, device="cuda")
    x, xrows, err = ops.step_prepare(tokens, embed, pos, p, tables, pos_shift=pos_shift)
    for b, t in enumerate(positions):
        want = ops.embed_step(tokens[b:b + 1], embed, pos, t - pos_shift if pos_shift else t, t if pos_shift else -1)
        assert torch.equal(x[b], want[0]), (b, t)
    for k in range(4):
        assert torch.equal(xrows[k], tables[k].index_select(0, p.long()))
    assert int(err.item()) == 0
    # without XPos tables the embedding alone
    x2, none, _ = ops.step_prepare(tokens, embed, pos, p, None, pos_shift=pos_shift)
    assert none is None and torch.equal(x2, x)
    # positions beyond the tables (and, shifted, before the first text row): reported, the row is neither read nor written
    bad = p.clone()
    bad[1] = rows                                                          # 2 + t is one past the position table, t one past XPos
    bad[3] = 10 ** 6
    if pos_shift:
        bad[0] = pos_shift - 1
    x3, xr3 = torch.full((B, d), 7.0, device="cuda"), torch.full((4, B, 32), 7.0, device="cuda")
    ops.step_prepare(tokens, embed, pos, bad, tables, pos_shift=pos_shift, error_word=err, out=x3, xpos_rows=xr3)
    assert int(err.item()) == H.KX_RAGGED_ERR_TABLE
    for b in range(B):
        if b in (1, 3) or (pos_shift and b == 0):
            assert bool((x3[b] == 7.0).all()) and bool((xr3[:, b] == 7.0).all()), b
        else:
            assert torch.equal(x3[b], x[b]) and torch.equal(xr3[:, b], xrows[:, b]), b


def test_sampler_draws_at_the_rows_own_position_and_advances_it():
    g = torch.Generator().manual_seed(13)
    B, V = 4, 502
    logits = torch.randn(B, V, generator=g).cuda()
    kw = dict(temperature=0.9, top_k=40, top_p=0.95, seed=3)
    start = [5, 70, 5, 9]
    for adv in (0, 1):
        p = torch.tensor(start, dtype=torch.int32, device="cuda")
        fin = torch.tensor([0, 0, 1, 0], dtype=torch.uint8, device="cuda")
        got = ops.sample_logits(logits, positions=p, advance=adv, finished=fin, **kw)
        assert p.tolist() == [s + adv for s in start]                       # finished rows move on too
        for b in range(B):
            want = ops.sample_logits(logits[b:b + 1], position=start[b] + adv, sequence_ids=torch.tensor([b]).cuda(),
                                     finished=fin[b:b + 1].clone(), **kw)
            assert int(got[b]) == int(want[0]), (adv, b)


# ---- 4. the contract -----------------------------------------------------------------------------------------------------------
@PRECS
@KWS
def test_each_row_generates_what_it_would_generate_alone(prec, tol, kw):
    lm0 = _lm(seed=7)
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = prec
    lens = [3, 9, 1, 6]
    tok = torch.randint(0, 502, (4, 9), generator=torch.Generator().manual_seed(4))     # the padding holds in-range ids: reading it would show
    _language_contract(lm, w, _cfg(), tok, lens, 20, kw, tol, seq_ids=[7, 3, 11, 5])


def test_padding_is_ignored_whatever_it_holds():
    lm = _lm(seed=7).to("cuda")
    lm.precision = "fp32"
    lens = [3, 9, 1, 6]
    tok = torch.randint(0, 502, (4, 9), generator=torch.Generator().manual_seed(4))
    a, la = lm.generate(tok.cuda(), 8, output_logits=True, prompt_lengths=lens, **SAMPLE)
    junk = torch.cat([tok, torch.zeros(4, 5, dtype=torch.long)], 1)          # a wider batch, ids no vocabulary has in the padding
    for b, L in enumerate(lens):
        junk[b, L:] = torch.tensor([10 ** 9, -1, 502, 77] * 4)[: 14 - L]
    b_, lb = lm.generate(junk.cuda(), 8, output_logits=True, prompt_lengths=lens, **SAMPLE)
    assert torch.equal(a, b_) and torch.equal(la, lb)


# ---- 5. one long row: it crosses the 128-key round while its neighbour does not ------------------------------------------------
def test_a_long_row_beside_a_short_one():
    lm0 = _lm(seed=9, max_pos=192)
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = "fp32"
    tok = torch.randint(0, 502, (2, 130), generator=torch.Generator().manual_seed(5))
    for kw in (dict(), SAMPLE):
        _language_contract(lm, w, _cfg(192), tok, [3, 130], 8, kw, 2e-4)


# ---- 6. both step paths --------------------------------------------------------------------------------------------------------
@PRECS
@pytest.mark.parametrize("B", [5, 17], ids=["B5-streaming", "B17-tile-gemm"])
def test_both_step_paths(prec, tol, B):
    """B = 5: the weight-streaming step with the wave-per-row LayerNorm prologue (mixed: fp16-pieces operands); B = 17: the
    tile-GEMM step, whose qkv epilogue reads the gathered tables with xpos_T = B."""
    lm0 = _lm(seed=10)
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = prec
    g = torch.Generator().manual_seed(6)
    lens = [int(v) for v in torch.randint(1, 8, (B,), generator=g)]
    lens[0], lens[-1] = 7, 1
    tok = torch.randint(0, 502, (B, 7), generator=g)
    _language_contract(lm, w, _cfg(), tok, lens, 6, SAMPLE, tol)


# ---- 7. the multimodal prompt --------------------------------------------------------------------------------------------------
@PRECS
@pytest.mark.parametrize("alias", [True, False])
def test_kosmos_rows_against_the_oracle_forward_of_each_row_alone(prec, tol, alias):
    sw = Switches(u1_inplace_alias=alias)
    m0 = Kosmos._from_config(tiny_config(), seed=1, switches=sw, perturb=0.1).eval()
    w, cfg = oracle_weights(m0), oracle_cfg(m0.cfg)
    m = m0.to("cuda")
    m.precision = prec
    g = torch.Generator().manual_seed(5)
    lens, n = [10, 4], 14
    tok = torch.randint(0, m.cfg.vocab, (2, 10), generator=g)
    img = torch.randn(2, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g)
    n_img = m.cfg.perceiver.latents
    for kw in (dict(), SAMPLE):
        got, logits = m.generate(tok.cuda(), img.cuda(), n, output_logits=True, prompt_lengths=lens, **kw)
        assert got.shape == (2, n) and logits.shape == (2, n, m.cfg.vocab)
        for b, L in enumerate(lens):
            text = torch.cat([tok[b, :L], got[b, :-1].cpu()])[None]
            ref = O.kosmos_forward(w, text, img[b:b + 1], cfg, oracle_switches(sw))[0, L + n_img - 1:]
            e = rel_err(logits[b], ref)
            print(f"ragged Kosmos.generate row {b} (text len {L}) vs oracle ({prec}, alias={alias}, {'sampled' if kw else 'greedy'}): {e:.3e}")
            assert e < tol, (b, e)
        _row_sampler_parity(got, logits, [tok[b, :L].numpy() for b, L in enumerate(lens)], [n_img + L for L in lens], [0, 1], kw)


# ---- 8. EOS in a ragged batch --------------------------------------------------------------------------------------------------
def test_eos_pads_the_finished_row_and_leaves_the_others_alone():
    lm = _lm(seed=8).to("cuda")
    lm.precision = "fp32"
    lens = [3, 9, 1, 6]
    tok = torch.randint(0, 502, (4, 9), generator=torch.Generator().manual_seed(6)).cuda()
    n, pad = 24, 1
    free = lm.generate(tok, n, prompt_lengths=lens).cpu()
    eos = int(free[1, 3])                                       # a token greedy produces at step 3 for row 1
    got = lm.generate(tok, n, prompt_lengths=lens, eos_token_id=eos, pad_token_id=pad, eos_poll=4).cpu()
    first = [(free[b] == eos).nonzero()[0].item() if (free[b] == eos).any() else None for b in range(4)]
    assert first[1] is not None and first[1] <= 3
    assert any(f is None or f > first[1] for f in first), first  # somebody runs on after row 1 has finished
    for b in range(4):
        f = n if first[b] is None else first[b]
        assert torch.equal(got[b, : min(f + 1, got.shape[1])], free[b, : min(f + 1, got.shape[1])])   # up to and including EOS
        assert (got[b, f + 1:] == pad).all()
    # the poll ends the loop once every row has finished
    one = lm.generate(tok[1:2], n, prompt_lengths=lens[1:2], eos_token_id=eos, pad_token_id=pad, eos_poll=4).cpu()
    assert one.shape[1] < n and one.shape[1] <= first[1] + 1 + 4


def test_a_device_position_outside_the_cache_is_reported_as_index_error():
    """The host cannot see device positions per step: the kernels' sticky word is what the loop reads after its last step."""
    from kosmosx import generation
    lm = _lm(seed=8).to("cuda")
    lm.precision = "fp32"
    tok = torch.randint(0, 502, (2, 6), generator=torch.Generator().manual_seed(6)).cuda()
    with torch.no_grad():
        state = {"max_len": 6 + 4}
        logits = lm.decoder._forward_incremental(tok, state, None, "fp32")
        state["positions"] = torch.tensor([6, 10], dtype=torch.int32, device="cuda")     # row 1: one past the 10-row cache
        state["pos_max"] = 6
        nxt = torch.zeros(2, dtype=torch.int64, device="cuda")
        lm.decoder._forward_incremental(None, state, None, "fp32", next_token=nxt)
        assert int(state["error"].item()) == H.KX_RAGGED_ERR_TABLE | H.KX_RAGGED_ERR_CACHE
        with pytest.raises(IndexError, match="index out of range in self"):
            generation._raise_position_error(int(state["error"].item()), state)
