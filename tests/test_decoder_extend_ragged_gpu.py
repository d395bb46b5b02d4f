"""Ragged extend: kx_decoder_extend_ragged under Decoder._extend_ragged — many rows appended to a filled cache in one pass, every
sequence at its own device-resident position.

The tiny LM of tests/test_decoder_extend_gpu.py (2 layers, dim 256, vocab 502, 324 positions).  Three prompts of lengths (5, 9, 12)
are prefilled right-padded; a ragged extend appends 7 rows per sequence, a second one 131 (past the 128-query block: the pair pass),
then single ragged steps follow.  Every row's logits are compared with the CPU oracle's full forward over that row's OWN
concatenated sequence, at that file's tolerances: fp32 2e-4, bf16 6e-2, f16c and mixed 1e-3."""
import pytest
import torch

from helpers import oracle_weights, rel_err
from kosmosx.generation import mask_padding
from kosmosx.model import KosmosLanguage
from oracle import kosmos_oracle as O

pytestmark = pytest.mark.gpu

CFG = O.DecoderCfg(layers=2, dim=256, ffn=512, heads=4, vocab=502, max_pos=324)
TOL = {"fp32": 2e-4, "bf16": 6e-2, "f16c": 1e-3, "mixed": 1e-3}
LENS, BLOCKS, STEPS = (5, 9, 12), (7, 131), 3


def _lm(seed=6):
    return KosmosLanguage(vocab_size=502, dim=256, depth=2, ffn_dim=512, decoder_heads=4, _seed=seed, _perturb=0.1,
                          _max_positions=324).eval()


@pytest.fixture(scope="module")
def ragged_ref():
    """(prompt [3, 12], the blocks [3, 7] and [3, 131], the step tokens [3, STEPS], per row the oracle's logits over the row's own
    sequence prompt[:len] | blocks | steps): computed once, shared, never written."""
    g = torch.Generator().manual_seed(11)
    prompt = torch.randint(0, 502, (3, max(LENS)), generator=g)
    blocks = [torch.randint(0, 502, (3, n), generator=g) for n in BLOCKS]
    steps = torch.randint(0, 502, (3, STEPS), generator=g)
    w = oracle_weights(_lm())
    refs = []
    for b, n in enumerate(LENS):
        seq = torch.cat([prompt[b, :n], *(blk[b] for blk in blocks), steps[b]])[None]
        refs.append(O.kosmos_language_forward(w, seq, CFG)[0])
    return prompt, blocks, steps, refs


def _run(lm, prec, ref, logits_of_second=True):
    """Prefill, the two ragged extends and the steps -> (state, [(what, row b, got logits, oracle rows)])."""
    prompt, blocks, steps, refs = ref
    dec = lm.decoder
    state, got = {}, []
    padded = mask_padding(prompt.cuda(), list(LENS))
    out = dec._forward_incremental(padded, state, None, prec)
    for b, n in enumerate(LENS):
        got.append(("prefill", b, out[b, :n], refs[b][:n]))
    pos = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    state.update(positions=pos, pos_max=max(LENS))
    at = list(LENS)
    for k, blk in enumerate(blocks):
        n = blk.shape[1]
        want = logits_of_second or k == 0
        out = dec._extend_ragged(blk.cuda(), state, pos, prec, output_logits=want)
        if want:
            assert out.shape == (3, n, 502) and out.dtype == torch.float32
            for b in range(3):
                got.append((f"extend {n}", b, out[b], refs[b][at[b]:at[b] + n]))
        else:
            assert out is None
        pos += n                                                             # (the caller moves the device positions)
        at = [a + n for a in at]
        assert state["pos_max"] == max(at)
    for j in range(STEPS):
        out = dec._forward_incremental(None, state, None, prec, next_token=steps[:, j].contiguous().cuda())
        for b in range(3):
            got.append((f"step {j}", b, out[b], refs[b][at[b]:at[b] + 1]))
        pos += 1
        at = [a + 1 for a in at]
    assert int(state["error"].item()) == 0
    return state, got, at


@pytest.mark.parametrize("prec", list(TOL))
def test_ragged_extends_then_steps_match_each_rows_own_full_forward(prec, ragged_ref):
    lm = _lm().to("cuda")
    lm.precision = prec
    state, got, at = _run(lm, prec, ragged_ref)
    worst = 0.0
    for what, b, out, want in got:
        e = rel_err(out, want)
        worst = max(worst, e)
        assert e < TOL[prec], (prec, what, b, e)
    print(f"ragged extend ({prec}): worst logits rel_err {worst:.3e} (tol {TOL[prec]:.0e})")
    assert at == [n + sum(BLOCKS) + STEPS for n in LENS]


def test_extend_without_logits_returns_none_and_fills_the_same_caches(ragged_ref):
    lm = _lm().to("cuda")
    lm.precision = "fp32"
    full, _, at = _run(lm, "fp32", ragged_ref)
    lean, _, _ = _run(lm, "fp32", ragged_ref, logits_of_second=False)
    for b, n in enumerate(at):                                               # every row a sequence really holds
        for c in ("kcache", "vcache"):
            e = rel_err(lean[c][:, b, :, :n], full[c][:, b, :, :n])
            assert e < TOL["fp32"], (c, b, e)


def test_the_refusals_leave_the_state_where_it_was(ragged_ref):
    prompt, blocks, _, refs = ragged_ref
    lm = _lm().to("cuda")
    lm.precision = "fp32"
    dec = lm.decoder
    state = {"max_len": 40}
    dec._forward_incremental(mask_padding(prompt.cuda(), list(LENS)), state, None, "fp32")
    with pytest.raises(ValueError, match="ragged incremental state"):        # a uniform state
        dec._extend_ragged(blocks[0].cuda(), state, torch.tensor(LENS, dtype=torch.int32, device="cuda"), "fp32")
    pos = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    state.update(positions=pos, pos_max=12)
    with pytest.raises(ValueError, match="ragged incremental state"):        # the public entry and _extend keep refusing a ragged state
        lm.extend(blocks[0].cuda(), state)
    with pytest.raises(IndexError, match="exceeds the table / cache"):       # 12 + 131 > 40
        dec._extend_ragged(blocks[1].cuda(), state, pos, "fp32")
    with pytest.raises(ValueError, match="batch size"):
        dec._extend_ragged(blocks[0][:2].cuda(), state, pos, "fp32")
    with pytest.raises(RuntimeError, match="precision changed"):
        dec._extend_ragged(blocks[0].cuda(), state, pos, "bf16")
    bad = blocks[0].clone()
    bad[1, 3] = 502
    with pytest.raises(IndexError):                                          # an id outside the vocabulary
        dec._extend_ragged(bad.cuda(), state, pos, "fp32")
    with pytest.raises(TypeError, match="seq_positions"):
        dec._extend_ragged(blocks[0].cuda(), state, pos.long(), "fp32")
    assert state["pos_max"] == 12 and pos.tolist() == list(LENS)
    out = dec._extend_ragged(blocks[0].cuda(), state, pos, "fp32")           # ... and a valid call still lands on the oracle
    for b, n in enumerate(LENS):
        assert rel_err(out[b], refs[b][n:n + 7]) < TOL["fp32"], b
    assert state["pos_max"] == 19 and int(state["error"].item()) == 0
