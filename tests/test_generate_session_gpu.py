"""Sessions: generate(return_session=True), then Session.generate / Session.append on the kept KV cache.

The contract under test: after any number of turns row b behaves like a fresh ragged generate() whose prompt is the row's whole
logical sequence so far.  Every returned logits row is compared with the CPU oracle's forward over that row's own sequence
(tolerances of tests/test_decoder_extend_gpu.py: fp32 2e-4, mixed 1e-3), and every token is replayed on ITS returned row through
the NumPy restatements of the constraint and sampler kernels (tests/test_generate_constrain_gpu._replay) with the conversation's
ids as the history and the absolute position as the Philox position — so a logits difference inside the tolerance cannot flip a
token in these tests.  The greedy scenario is also compared token for token with a fresh generate() over the concatenated ragged
prompts; that is only asserted because no pick is close (test_the_prompt_seed_leaves_a_wide_top_two_gap)."""
import numpy as np
import pytest
import torch

from helpers import oracle_cfg, oracle_switches, oracle_weights, rel_err, tiny_config
from kosmosx.config import Switches
from kosmosx.generation import Session
from kosmosx.model import Kosmos, KosmosLanguage
from oracle import kosmos_oracle as O
from test_generate_constrain_gpu import _replay

pytestmark = pytest.mark.gpu

CFG = O.DecoderCfg(layers=2, dim=256, ffn=512, heads=4, vocab=502, max_pos=324)
TOL = {"fp32": 2e-4, "mixed": 1e-3}
PAD = 1
LENS, N1, LENS2, N2 = (5, 9, 12), 6, (3, 6, 1), 6          # the greedy scenario (SEED was chosen for exactly these)
SEED = 23                                                   # gap / bound = 14 on the CPU oracle (seeds 0 .. 39: 6 and 8 next, most below 1)
SAMPLED = dict(do_sample=True, top_k=20, repetition_penalty=1.2, no_repeat_ngram_size=2, seed=5)


def _lm(seed=6):
    return KosmosLanguage(vocab_size=502, dim=256, depth=2, ffn_dim=512, decoder_heads=4, _seed=seed, _perturb=0.1,
                          _max_positions=324).eval()


def _n_valid(row, eos):
    """A turn ends inclusively at an EOS, or at the budget."""
    row = row.tolist()
    return row.index(eos) + 1 if eos in row else len(row)


def _check_turn(forward, hist, new, out, logits, kw, eos, tol, prefix=0):
    """One turn of every row against the references.  ``hist``: per row the conversation's text ids before the turn, ``new`` the
    ids the turn brought in, ``forward(b, ids)`` the oracle's logits [T, V] over row b's whole sequence with text ids ``ids``.
    Returns the histories after the turn."""
    out, logits = out.cpu(), logits.cpu()
    prompts = [np.array(h + x, dtype=np.int64) for h, x in zip(hist, new)]
    starts = [prefix + len(p) for p in prompts]                              # the position the first new token takes
    cons = dict(eos_token_id=eos, no_repeat_ngram_size=kw.get("no_repeat_ngram_size", 0))
    _replay(out, logits, prompts, starts, kw, cons)
    after = []
    for b in range(out.shape[0]):
        nv = _n_valid(out[b], eos)
        ids = prompts[b].tolist() + out[b, :nv].tolist()
        ref = forward(b, ids[:-1])[starts[b] - 1:]
        e = rel_err(logits[b, :nv], ref)
        assert ref.shape[0] == nv and e < tol, (b, nv, e)
        after.append(ids)
    return after


def _pick_eos(plain):
    """An id row 0 emits early and the other rows never do: row 0 stops there, the others run to the budget."""
    plain = plain.cpu()
    others = set(plain[1:].flatten().tolist()) | {PAD}
    for g in range(1, plain.shape[1] - 1):
        if int(plain[0, g]) not in others and int(plain[0, g]) not in plain[0, :g].tolist():
            return int(plain[0, g]), g
    raise AssertionError(f"no id of row 0 is free of the other rows: {plain}")


@pytest.mark.parametrize("name,kw,chunk,prec,capacity", [("greedy", {}, None, "fp32", 64), ("greedy", {}, None, "mixed", None),
                                                         ("sampled", SAMPLED, None, "fp32", None), ("chunked", {}, 2, "fp32", 80)])
def test_language_session_turns_match_the_oracle_and_the_sampler_references(name, kw, chunk, prec, capacity):
    lm0 = _lm()
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = prec
    tol = TOL[prec]
    g = torch.Generator().manual_seed(31)
    tok = torch.randint(2, 502, (3, 12), generator=g)
    turns = [(torch.randint(2, 502, (3, 6), generator=g), [3, 6, 1]), (torch.randint(2, 502, (3, 4), generator=g), [4, 2, 3]),
             (torch.randint(2, 502, (3, 5), generator=g), [1, 5, 2])]
    n = 10

    def forward(b, ids):
        return O.kosmos_language_forward(w, torch.tensor(ids)[None], CFG)[0]
    eos, at = _pick_eos(lm.generate(tok.cuda(), n, prompt_lengths=list(LENS), **kw))
    common = dict(eos_token_id=eos, pad_token_id=PAD, output_logits=True, prefill_chunk=chunk, **kw)
    out, logits, sess = lm.generate(tok.cuda(), n, prompt_lengths=list(LENS), return_session=True, session_capacity=capacity, **common)
    assert isinstance(sess, Session) and sess.capacity == (322 if capacity is None else capacity)
    assert _n_valid(out[0].cpu(), eos) == at + 1 and all(_n_valid(out[b].cpu(), eos) == out.shape[1] for b in (1, 2))
    hist = _check_turn(forward, [[] for _ in LENS], [tok[b, :l].tolist() for b, l in enumerate(LENS)], out, logits, kw, eos, tol)
    assert sess.lengths == [len(h) for h in hist]
    # turn 2: ragged new tokens on the ragged cache (every row has a pending token)
    x, lens = turns[0]
    out, logits = sess.generate(x.cuda(), n, prompt_lengths=lens, **common)
    hist = _check_turn(forward, hist, [x[b, :l].tolist() for b, l in enumerate(lens)], out, logits, kw, eos, tol)
    assert sess.lengths == [len(h) for h in hist]
    # known tokens, nothing generated: afterwards no row has a pending token
    x, lens = turns[1]
    assert sess.append(x.cuda(), prompt_lengths=lens, prefill_chunk=chunk) is None
    hist = [h + x[b, :l].tolist() for b, (h, l) in enumerate(zip(hist, lens))]
    assert sess.lengths == [len(h) for h in hist]
    # turn 3
    x, lens = turns[2]
    out, logits = sess.generate(x.cuda(), n, prompt_lengths=lens, **common)
    hist = _check_turn(forward, hist, [x[b, :l].tolist() for b, l in enumerate(lens)], out, logits, kw, eos, tol)
    assert sess.lengths == [len(h) for h in hist]
    print(f"session ({name}, {prec}): lengths after three turns and an append {sess.lengths}")


@pytest.fixture(scope="module")
def greedy_runs():
    """The greedy fp32 scenario, once: turn 1 and turn 2 through a session, and the fresh generate() over the concatenation."""
    lm = _lm().to("cuda")
    lm.precision = "fp32"
    g = torch.Generator().manual_seed(SEED)
    tok = torch.randint(0, 502, (3, 12), generator=g)
    x2 = torch.randint(0, 502, (3, 6), generator=g)
    out1, lg1, sess = lm.generate(tok.cuda(), N1, prompt_lengths=list(LENS), output_logits=True, return_session=True)
    plain1 = lm.generate(tok.cuda(), N1, prompt_lengths=list(LENS))
    out2, lg2 = sess.generate(x2.cuda(), N2, prompt_lengths=list(LENS2), output_logits=True)
    rows = [torch.cat([tok[b, :LENS[b]], out1[b].cpu(), x2[b, :LENS2[b]]]) for b in range(3)]
    lens = [int(r.shape[0]) for r in rows]
    cat = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True, padding_value=7)
    fresh, lgf = lm.generate(cat.cuda(), N2, prompt_lengths=lens, output_logits=True)
    return dict(out1=out1.cpu(), plain1=plain1.cpu(), out2=out2.cpu(), fresh=fresh.cpu(), logits=[lg1.cpu(), lg2.cpu(), lgf.cpu()],
                lengths=sess.lengths, want_lengths=[n + N2 for n in lens])


def test_the_prompt_seed_leaves_a_wide_top_two_gap(greedy_runs):
    """Token equality between the session and the fresh run is only asserted because no pick is close: the smallest top-two logit
    gap of every run involved exceeds 10 x the fp32 tolerance x the logits' rms.  A property of SEED (chosen on the CPU oracle,
    where the same formula gives gap / bound = 14), not of the model."""
    for lg in greedy_runs["logits"]:
        top = lg.topk(2, -1).values
        gap, rms = float((top[..., 0] - top[..., 1]).min()), float(lg.pow(2).mean().sqrt())
        print(f"smallest top-two gap {gap:.3e}, 10 x tol x rms = {10 * 2e-4 * rms:.3e}")
        assert gap > 10 * 2e-4 * rms


def test_a_greedy_session_turn_equals_a_fresh_generate_over_the_concatenated_prompts(greedy_runs):
    r = greedy_runs
    assert torch.equal(r["out1"], r["plain1"])                               # asking for a session changes no token of the call
    assert r["out2"].shape == (3, N2) and torch.equal(r["out2"], r["fresh"])
    assert r["lengths"] == r["want_lengths"]
    e = float((r["logits"][1] - r["logits"][2]).abs().max()) / float(r["logits"][2].pow(2).mean().sqrt())
    print(f"session turn vs fresh generate: logits differ by {e:.3e} of their rms (tol {TOL['fp32']:.0e})")
    assert e < 2 * TOL["fp32"]                                               # both within tol of the oracle


@pytest.mark.parametrize("prec", ["fp32", "mixed"])
@pytest.mark.parametrize("alias", [True, False])
def test_kosmos_session_first_turn_with_images_then_a_text_turn(alias, prec):
    sw = Switches(u1_inplace_alias=alias)
    m0 = Kosmos._from_config(tiny_config(), seed=1, switches=sw, perturb=0.1).eval()
    w, cfg = oracle_weights(m0), oracle_cfg(m0.cfg)
    m = m0.to("cuda")
    m.precision = prec
    g = torch.Generator().manual_seed(5)
    tok = torch.randint(2, m.cfg.vocab, (2, 10), generator=g)
    img = torch.randn(2, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g)
    x2 = torch.randint(2, m.cfg.vocab, (2, 4), generator=g)
    n_img, n = m.cfg.perceiver.latents, 6
    lens, lens2 = [5, 10], [4, 2]

    def forward(b, ids):
        return O.kosmos_forward(w, torch.tensor(ids)[None], img[b:b + 1], cfg, oracle_switches(sw))[0]
    for kw in ({}, dict(do_sample=True, top_k=20, repetition_penalty=1.2, seed=9)):
        common = dict(output_logits=True, pad_token_id=PAD, **kw)
        out, logits, sess = m.generate(tok.cuda(), img.cuda(), n, prompt_lengths=lens, return_session=True, **common)
        hist = _check_turn(forward, [[], []], [tok[b, :l].tolist() for b, l in enumerate(lens)], out, logits, kw, None, TOL[prec],
                           prefix=n_img)
        assert sess.lengths == [n_img + len(h) for h in hist]
        out, logits = sess.generate(x2.cuda(), n, prompt_lengths=lens2, **common)
        hist = _check_turn(forward, hist, [x2[b, :l].tolist() for b, l in enumerate(lens2)], out, logits, kw, None, TOL[prec],
                           prefix=n_img)
        assert sess.lengths == [n_img + len(h) for h in hist] == [n_img + l + n + l2 + n for l, l2 in zip(lens, lens2)]


def test_a_turn_that_overruns_the_capacity_raises_before_any_launch_and_the_session_continues(monkeypatch):
    lm0 = _lm()
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = "fp32"
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(2, 502, (3, 12), generator=g)
    big, x = torch.randint(2, 502, (3, 20), generator=g), torch.randint(2, 502, (3, 4), generator=g)

    def forward(b, ids):
        return O.kosmos_language_forward(w, torch.tensor(ids)[None], CFG)[0]
    with pytest.raises(IndexError, match="exceed the 16-row position table / cache"):
        lm.generate(tok.cuda(), 6, return_session=True, session_capacity=16)  # 12 + 6 > 16
    out, logits, sess = lm.generate(tok.cuda(), 6, prompt_lengths=list(LENS), output_logits=True, return_session=True, session_capacity=40)
    hist = _check_turn(forward, [[] for _ in LENS], [tok[b, :l].tolist() for b, l in enumerate(LENS)], out, logits, {}, None, 2e-4)
    before = list(sess.lengths)
    assert before == [11, 15, 18]
    launched = []
    inner = lm.decoder._extend_ragged
    monkeypatch.setattr(lm.decoder, "_extend_ragged", lambda *a, **k: launched.append(1) or inner(*a, **k))
    with pytest.raises(IndexError, match="exceed the session's 40-row cache"):
        sess.generate(big.cuda(), 8)                                         # 17 cached + 21 + 8 = 46
    with pytest.raises(IndexError, match="exceed the session's 40-row cache"):
        sess.append(torch.cat([big, big], 1).cuda())                         # 17 + 41
    assert not launched and sess.lengths == before
    out, logits = sess.generate(x.cuda(), 8, prompt_lengths=[4, 1, 2], output_logits=True)   # 17 + 5 + 8 = 30 fits
    assert launched
    hist = _check_turn(forward, hist, [x[b, :l].tolist() for b, l in enumerate([4, 1, 2])], out, logits, {}, None, 2e-4)
    assert sess.lengths == [len(h) for h in hist] == [23, 24, 28]
    # an id outside the vocabulary: IndexError, and the session is where it was
    bad = x.clone()
    bad[1, 0] = 502
    with pytest.raises(IndexError):
        sess.generate(bad.cuda(), 2)
    assert sess.lengths == [23, 24, 28]
    out, logits = sess.generate(x.cuda(), 2, output_logits=True)
    hist = _check_turn(forward, hist, [x[b].tolist() for b in range(3)], out, logits, {}, None, 2e-4)
    assert sess.lengths == [len(h) for h in hist]
