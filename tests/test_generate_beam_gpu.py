"""generate(num_beams=W): beam search end to end for both model classes.

As in test_generate_gpu.py, model parity and search parity are checked separately: the logits rows every step ranked are
returned (``output_trace``) and compared, along each surviving lineage, with the CPU oracle's full forward over prompt +
hypothesis — a wrong parent in any cache gather fails there; the search itself is replayed step by step through the CPU
restatement (beam_ref) on THOSE logits, so a logits difference inside the tolerance cannot change a decision in the test."""
import numpy as np
import pytest
import torch

import beam_ref as BR
from helpers import oracle_cfg, oracle_switches, oracle_weights, rel_err, tiny_config
from kosmosx import generation
from kosmosx.config import Switches
from kosmosx.model import Kosmos, KosmosLanguage
from oracle import kosmos_oracle as O

pytestmark = pytest.mark.gpu

CFG = O.DecoderCfg(layers=2, dim=256, ffn=512, heads=4, vocab=502, max_pos=64)
PAD = 1


def _lm(seed=5):
    return KosmosLanguage(vocab_size=502, dim=256, depth=2, ffn_dim=512, decoder_heads=4, _seed=seed, _perturb=0.1,
                          _max_positions=64).eval()


def _np(tr):
    return {k: v.cpu().numpy() for k, v in tr.items()}


def _replay(tr, seqs, scores, *, B, W, R, eos=None, alpha=1.0, early=False):
    """Every step of the trace through beam_ref.step from the device's own previous live state, then finalize / backtrack
    against what generate() returned.  Returns the tally."""
    tr = _np(tr)
    n = tr["token"].shape[0]
    seqs = seqs.cpu().numpy().reshape(B, R, n)
    scores = scores.cpu().numpy()
    tally = BR.Tally()
    for b in range(B):
        rows = slice(b * W, (b + 1) * W)
        pool, done = [], False
        for g in range(n):
            x = tr["logits"][g, rows][: 1 if g == 0 else W]
            s_in = np.zeros(1) if g == 0 else tr["score"][g - 1, rows]
            ref = BR.step(x, s_in, pool, g, W=W, eos=eos, pad=PAD, alpha=alpha, early=early, done=done)
            # (the trace keeps the pool and the done byte as they are after the last step only: per step they follow the reference,
            # and are compared below)
            got = dict(token=tr["token"][g, rows], parent=tr["parent"][g, rows], score=tr["score"][g, rows], done=ref["done"],
                       pool=([p["score"] for p in ref["pool"]], [p["end"] for p in ref["pool"]], [p["parent"] for p in ref["pool"]],
                             len(ref["pool"])))
            BR.check_step(got, ref, tally, msg=f"row {b} step {g}")
            pool, done = ref["pool"], ref["done"]
        assert bool(tr["done"][b]) == done, (b, done)
        fin = BR.finalize(tr["score"][n - 1, rows], pool, done, n, W=W, R=R, alpha=alpha)
        BR.check_pool((tr["pool_score"][b], tr["pool_end"][b], tr["pool_parent"][b], tr["pool_count"][b]), fin["pool"], f"final pool {b}")
        want = [BR.backtrack(None if k is None else fin["pool"][k], tr["parent"][:, rows], tr["token"][:, rows], n, eos=eos, pad=PAD)
                for k in fin["order"]]
        if [list(map(int, seqs[b, r])) for r in range(R)] != want:
            assert fin["margin"] <= BR.EPS_M, (b, seqs[b], want)              # only a near-tie may order them otherwise
            tally.counted += 1
        for r in range(R):
            assert (scores[b, r] == fin["score"][r]) if not np.isfinite(fin["score"][r]) else abs(scores[b, r] - fin["score"][r]) <= BR.EPS_S
    tally.check()
    return tally


def _lineages(tr, B, W):
    """The B * W final live beams: (tokens [n], input rows [n]) — the logits row of step g that the lineage was ranked from."""
    tr = _np(tr)
    n = tr["token"].shape[0]
    out = []
    for b in range(B):
        for i in range(W):
            slot, toks, rows = i, [0] * n, [0] * n
            for g in range(n - 1, -1, -1):
                toks[g] = int(tr["token"][g, b * W + slot])
                slot = int(tr["parent"][g, b * W + slot])
                rows[g] = b * W + slot
            out.append((b, toks, rows))
    return out


def _check_lineages(tr, oracle_logits_of, B, W, tol, what):
    """oracle_logits_of(batch rows [N], token lists [N][n]) -> [N, n, V]: the oracle's logits at the positions each token was drawn at."""
    lin = _lineages(tr, B, W)
    assert bool(torch.isfinite(tr["score"][-1]).all())                       # no EOS here: every live beam is a real hypothesis
    ref = oracle_logits_of([b for b, _, _ in lin], [t for _, t, _ in lin])
    n = tr["token"].shape[0]
    worst = 0.0
    for k, (_, _, rows) in enumerate(lin):
        got = torch.stack([tr["logits"][g, rows[g]] for g in range(n)])
        worst = max(worst, rel_err(got, ref[k]))
    print(f"beam lineages vs oracle ({what}): {worst:.3e}")
    assert worst < tol
    assert len({(b, tuple(t)) for b, t, _ in lin}) == B * W                  # the beams of a batch row are distinct hypotheses


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("mixed", 1e-3)])
def test_language_beam_search_replays_and_follows_its_lineages(prec, tol):
    lm0 = _lm(seed=7)
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = prec
    B, P, n, W = 3, 9, 20, 4
    tok = torch.randint(0, 502, (B, P), generator=torch.Generator().manual_seed(4))
    seqs, scores, tr = lm.generate(tok.cuda(), n, num_beams=W, output_scores=True, output_trace=True)
    assert seqs.shape == (B, n) and seqs.dtype == torch.int64 and scores.shape == (B, 1) and scores.dtype == torch.float32
    assert tr["logits"].shape == (n, B * W, 502) and tr["parent"].dtype == torch.int32 and tr["token"].dtype == torch.int64
    assert bool((tr["logits"][0].view(B, W, 502)[:, 1:] == 0).all())        # step 0 holds the B prefill rows in rows b * W
    t = _replay(tr, seqs, scores, B=B, W=W, R=1)
    print(f"replay ({prec}): {t.counted} of {t.cases} cases inside the margin")

    def oracle(rows, toks):
        full = torch.cat([tok[rows], torch.tensor(toks)[:, :-1]], 1)
        return O.kosmos_language_forward(w, full, CFG)[:, P - 1:]
    _check_lineages(tr, oracle, B, W, tol, prec)
    # R = W: all hypotheses, best first, [B, R, n]; the best is what R = 1 returned
    allseq, allsc = lm.generate(tok.cuda(), n, num_beams=W, num_return_sequences=W, output_scores=True, length_penalty=0.6)
    assert allseq.shape == (B, W, n) and bool((allsc[:, :-1] >= allsc[:, 1:]).all())
    assert lm.generate(tok.cuda(), n, num_beams=W).equal(seqs)


def test_one_beam_through_the_beam_loop_is_greedy():
    lm = _lm(seed=6).to("cuda")
    lm.precision = "fp32"
    tok = torch.randint(0, 502, (3, 9), generator=torch.Generator().manual_seed(2)).cuda()
    n = 20
    greedy = lm.generate(tok, n).cpu()
    got, tr = lm.generate(tok, n, num_beams=1, _beam_path=True, output_trace=True)
    assert got.shape == (3, n)
    top2 = tr["logits"].topk(2, dim=-1).values.cpu()                         # [n, B, 2]
    for b in range(3):
        for g in range(n):
            if float(top2[g, b, 0] - top2[g, b, 1]) <= 2e-4:
                break                                                        # a near-tie may send the two searches apart from here
            assert int(got[b, g]) == int(greedy[b, g]), (b, g)
        else:
            g = n
        assert g >= n // 2                                                   # the comparison covered something


def test_eos_pool_padding_order_and_early_stopping():
    lm = _lm(seed=8).to("cuda")
    lm.precision = "fp32"
    # (model and prompt seeds: on the CPU oracle's logits the reference's smallest deciding margin of the runs below is 3.1e-4,
    # outside EPS_M; this tiny model scores the beams of a row almost alike, and other seeds leave margins of 1e-6)
    tok = torch.randint(0, 502, (3, 9), generator=torch.Generator().manual_seed(9)).cuda()
    B, n, W = 3, 24, 4
    _, free = lm.generate(tok, n, num_beams=W, output_trace=True)
    second = free["token"][1:8, 1].cpu()                                     # row 0's second-ranked tokens of steps 1 .. 7
    eos = int(second.mode().values)
    seqs, scores, tr = lm.generate(tok, n, num_beams=W, num_return_sequences=W, eos_token_id=eos, pad_token_id=PAD, eos_poll=0,
                                   output_scores=True, output_trace=True, length_penalty=1.2)
    assert seqs.shape == (B, W, n) and scores.shape == (B, W)
    assert int(tr["pool_count"][0]) >= 1                                     # row 0 finished at least one hypothesis
    s = seqs.cpu()
    for b in range(B):
        for r in range(W):
            hit = (s[b, r] == eos).nonzero()
            if len(hit):
                assert bool((s[b, r, int(hit[0]) + 1:] == PAD).all())        # padded after its EOS
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())                     # best first
    _replay(tr, seqs, scores, B=B, W=W, R=W, eos=eos, alpha=1.2)
    # early stopping: a row is done as soon as its pool is full, and the poll then ends the loop
    N = 50
    one, sc1, tr1 = lm.generate(tok[:1], N, num_beams=2, num_return_sequences=2, eos_token_id=eos, pad_token_id=PAD, eos_poll=4,
                                early_stopping=True, output_scores=True, output_trace=True)
    print(f"early stopping: {one.shape[2]} of {N} steps, pool ends {tr1['pool_end'].tolist()}")
    assert one.shape[2] < N and bool(tr1["done"].all())
    assert one.shape[2] <= int(tr1["pool_end"].max()) + 1 + 4                # no later than eos_poll steps after the row was done
    _replay(tr1, one, sc1, B=1, W=2, R=2, eos=eos, early=True)
    assert bool((one[0] == eos).any(dim=-1).all())                           # both returned hypotheses are finished ones


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("mixed", 1e-3)])
@pytest.mark.parametrize("alias", [True, False])
def test_kosmos_beam_search_replays_and_follows_its_lineages(prec, tol, alias):
    sw = Switches(u1_inplace_alias=alias)
    m0 = Kosmos._from_config(tiny_config(), seed=1, switches=sw, perturb=0.1).eval()
    w, cfg = oracle_weights(m0), oracle_cfg(m0.cfg)
    m = m0.to("cuda")
    m.precision = prec
    g = torch.Generator().manual_seed(5)
    B, W, Tt, n = 2, 3, 10, 12
    tok = torch.randint(0, m.cfg.vocab, (B, Tt), generator=g)
    img = torch.randn(B, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g)
    n_img = m.cfg.perceiver.latents
    seqs, scores, tr = m.generate(tok.cuda(), img.cuda(), n, num_beams=W, output_scores=True, output_trace=True)
    assert seqs.shape == (B, n)
    _replay(tr, seqs, scores, B=B, W=W, R=1)

    def oracle(rows, toks):
        text = torch.cat([tok[rows], torch.tensor(toks)[:, :-1]], 1)
        return O.kosmos_forward(w, text, img[rows], cfg, oracle_switches(sw))[:, Tt + n_img - 1:]
    _check_lineages(tr, oracle, B, W, tol, f"Kosmos {prec} alias={alias}")


def test_repeatable_and_the_default_path_is_untouched():
    lm = _lm(seed=9).to("cuda")
    lm.precision = "mixed"
    tok = torch.randint(0, 502, (2, 9), generator=torch.Generator().manual_seed(7)).cuda()
    kw = dict(num_beams=3, num_return_sequences=2, output_scores=True, length_penalty=0.8)
    a, sa = lm.generate(tok, 12, **kw)
    b, sb = lm.generate(tok, 12, **kw)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    # num_beams = 1 without the switch is generate_loop on the prefill, argument for argument
    sample = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, repetition_penalty=1.2, seed=21)
    for extra in (dict(), sample):
        got = lm.generate(tok, 12, num_beams=1, **extra)
        state = {"max_len": 9 + 12}
        with torch.no_grad():
            logits = lm.decoder._forward_incremental(tok, state, None, lm.precision)
            want = generation.generate_loop(lm.decoder, lm.precision, state, logits, tok.long(), 12,
                                            generation.loop_options(502, 2, **extra))
        assert torch.equal(got, want) and torch.equal(got, lm.generate(tok, 12, **extra))


@pytest.mark.parametrize("prec", ["fp32", "mixed", "bf16"])
def test_beam_search_under_the_row_major_cache_layout(prec):
    """Tuning key 9 = 1 (caches [Tmax][heads*64] per sequence): prefill, decode steps and kx_kv_cache_gather all read the key, so
    the search returns the tokens and scores of the default layout — every step's arithmetic is the same on the same values."""
    from kosmosx import _hip
    tok = torch.randint(0, 502, (3, 9), generator=torch.Generator().manual_seed(4)).cuda()
    lib = _hip.load()
    res = []
    for key in (0, 1):
        lm = _lm(seed=7).to("cuda")
        lm.precision = prec
        lib.kx_set_tuning(9, key)
        try:
            seqs, scores = lm.generate(tok, 20, num_beams=4, num_return_sequences=4, output_scores=True)
            torch.cuda.synchronize()
        finally:
            lib.kx_set_tuning(9, 0)
        res.append((seqs.cpu(), scores.cpu()))
    assert res[0][0].shape == (3, 4, 20) and bool(torch.isfinite(res[0][1]).all())
    assert torch.equal(res[1][0], res[0][0]) and torch.equal(res[1][1], res[0][1])
