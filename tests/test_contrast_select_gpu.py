"""kx_contrast_candidates, kx_contrast_hidden and kx_contrast_select on the device against tests/contrast_ref.py.

The penalty is held to 2 * D * 2^-24 — twice the worst-case bound of an fp32 dot product of unit vectors — against float64 on the
same fp32 rows; the choice is demanded exactly (tests/test_contrast.py asserts the float64 gaps of these very cases on the CPU) and,
bit for bit, equal to the fp32 restatement of the score on the device's own probabilities and penalties."""
import numpy as np
import pytest
import torch

import contrast_ref as R
from kosmosx import ops
from kosmosx.model import KosmosLanguage

pytestmark = pytest.mark.gpu
PAD = 1


def _select(case, alpha=R.ALPHA, finished=None, eos=None, tokens=None):
    k, D, Ps, cap = case["k"], case["D"], case["Ps"], case["cap"]
    B = len(Ps)
    dev = "cuda"
    t = dict(u=torch.from_numpy(case["u"]).to(dev), prob=torch.from_numpy(case["prob"]).to(dev), history=torch.from_numpy(case["history"]).to(dev),
             hist_rows=torch.tensor(Ps, dtype=torch.int32, device=dev), hist_len=torch.full((B,), -7, dtype=torch.int32, device=dev),
             step_tokens=(torch.arange(B * k, dtype=torch.int64, device=dev) * 3 + 10) if tokens is None else tokens.to(dev),
             finished=torch.zeros(B, dtype=torch.uint8, device=dev) if finished is None else torch.tensor(finished, dtype=torch.uint8, device=dev),
             next_token=torch.full((B,), -5, dtype=torch.int64, device=dev), chosen=torch.full((B,), -5, dtype=torch.int32, device=dev),
             out_tokens=torch.full((B, 3), -5, dtype=torch.int64, device=dev), cand_penalty=torch.full((B, 3, k), -5.0, device=dev),
             chosen_trace=torch.full((B, 3), -5, dtype=torch.int32, device=dev), error_word=torch.zeros(1, dtype=torch.int32, device=dev))
    ops.contrast_select(t["u"], t["prob"], t["history"], hist_rows=t["hist_rows"], hist_len=t["hist_len"], alpha=alpha,
                        step_tokens=t["step_tokens"], finished=t["finished"], next_token=t["next_token"], chosen=t["chosen"],
                        scratch=ops.contrast_scratch(B, k, cap, dev), error_word=t["error_word"], eos_token_id=eos, pad_token_id=PAD,
                        out_tokens=t["out_tokens"], cand_penalty=t["cand_penalty"], chosen_trace=t["chosen_trace"], col=1)
    torch.cuda.synchronize()
    return {n: v.cpu().numpy() for n, v in t.items()}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: f"s{c[0]}-k{c[1]}-D{c[2]}-P{'_'.join(map(str, c[3]))}")
def test_penalty_choice_and_append(case):
    seed, k, D, Ps = case
    c = R.select_case(seed, k, D, Ps)
    pens, _, picks = R.case_reference(c)
    o = _select(c)
    assert int(o["error_word"][0]) == 0
    tol = 2 * D * 2.0 ** -24
    got = o["cand_penalty"][:, 1]
    err = np.abs(got.astype(np.float64) - pens).max()
    print(f"k={k} D={D} P={Ps}: penalty max|d| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    assert o["chosen"].tolist() == picks                                   # the float64 arg max (gaps > 1e-3: tests/test_contrast.py)
    for b, P in enumerate(Ps):
        j = int(o["chosen"][b])
        assert j == R.choose(R.scores_fp32(c["prob"][b * k:(b + 1) * k], got[b]))           # the fp32 restatement, bit for bit
        assert int(o["next_token"][b]) == (b * k + j) * 3 + 10 == int(o["out_tokens"][b, 1])
        assert int(o["chosen_trace"][b, 1]) == j and int(o["hist_len"][b]) == P + 1
        assert np.array_equal(o["history"][b, P].view(np.uint32), c["u"][b * k + j].view(np.uint32))
    keep = np.ones(c["history"].shape[:2], bool)
    keep[np.arange(len(Ps)), Ps] = False
    assert np.array_equal(o["history"][keep].view(np.uint32), c["history"][keep].view(np.uint32))     # no other history row changed
    assert (o["out_tokens"][:, [0, 2]] == -5).all() and (o["cand_penalty"][:, [0, 2]] == -5).all() and (o["chosen_trace"][:, [0, 2]] == -5).all()
    assert not o["finished"].any()


@pytest.mark.parametrize("D", [128, 2048])
def test_the_bits_do_not_depend_on_the_placement(D):
    """The same candidate and history rows as sequence 0 / slot 0..1 of a (B, k) = (1, 2) launch and as sequence 2 / slots 3..4 of a
    (3, 5) launch with a larger capacity: identical penalty bits."""
    a = R.select_case(11, 2, D, [257])
    big = R.select_case(12, 5, D, [65, 1000, 257], cap=1100)
    big["history"][2, :257] = a["history"][0, :257]
    big["u"][2 * 5 + 3:2 * 5 + 5] = a["u"]
    pa, pb = _select(a)["cand_penalty"][0, 1], _select(big)["cand_penalty"][2, 1, 3:5]
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    assert np.abs(pa.astype(np.float64) - R.penalty(a["u"], a["history"][0, :257])).max() <= 2 * D * 2.0 ** -24


def test_equal_scores_choose_the_lowest_index():
    c = R.select_case(5, 5, 128, [64, 65])
    for b in range(2):
        c["u"][b * 5 + 3] = c["u"][b * 5 + 1]
        c["prob"][b * 5:(b + 1) * 5] = [0.1, 0.3, 0.05, 0.3, 0.02]
    o = _select(c, alpha=0.0)                                              # alpha = 0: the score is the probability alone
    assert o["chosen"].tolist() == [1, 1]
    pen = o["cand_penalty"][:, 1]
    assert np.array_equal(pen[:, 1].view(np.uint32), pen[:, 3].view(np.uint32))
    c["prob"][0:5] = [0.3, 0.3, 0.3, 0.3, 0.3]
    c["u"][0:5] = c["u"][2]
    assert _select(c, alpha=0.7)["chosen"].tolist()[0] == 0                # every score equal, bit for bit


def test_a_nan_score_loses_to_every_number():
    c = R.select_case(6, 2, 128, [10])
    c["prob"][:] = [np.nan, 1e-6]
    assert _select(c)["chosen"].tolist() == [1]


def test_a_finished_row_writes_only_its_pad_and_the_eos_finishes_a_row():
    c = R.select_case(7, 2, 128, [63, 64, 65])
    _, _, picks = R.case_reference(c)
    eos = (2 * 2 + picks[2]) * 3 + 10                                      # what row 2 is about to emit
    o = _select(c, finished=[0, 1, 0], eos=eos)
    assert o["finished"].tolist() == [0, 1, 1]
    assert int(o["next_token"][1]) == PAD == int(o["out_tokens"][1, 1])
    assert int(o["chosen"][1]) == -5 and int(o["hist_len"][1]) == -7 and int(o["chosen_trace"][1, 1]) == -5
    assert (o["cand_penalty"][1] == -5).all() and np.array_equal(o["history"][1], c["history"][1])
    assert int(o["next_token"][2]) == eos and int(o["hist_len"][2]) == 66 and o["chosen"].tolist()[0] == picks[0]


def test_a_history_without_room_raises_the_error_bit_and_writes_nothing():
    c = R.select_case(8, 2, 128, [5, 9], cap=9)                             # row 1: P == cap, no row to append to (checked by the kernel)
    o = _select(c)
    assert int(o["error_word"][0]) == ops.H.KX_RAGGED_ERR_CACHE
    assert int(o["next_token"][1]) == -5 and int(o["chosen"][1]) == -5 and int(o["next_token"][0]) != -5


# ---- the candidates ----

@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_candidates_are_step_logprobs_top_k_of_the_addressed_row(k):
    B, V, kp = 3, 1031, 4
    g = torch.Generator().manual_seed(k)
    logits = (torch.randn(B * kp, V, generator=g) * 3).cuda()
    logits[5, 7] = logits[5, 900] = logits[5].max() + 1.0                  # equal values: the lowest id first
    chosen = torch.tensor([2, 1, 3], dtype=torch.int32, device="cuda")
    rows = torch.tensor([2, 5, 11], device="cuda")
    lp, top_lp, top_id = torch.zeros(B, 1, device="cuda"), torch.zeros(B, 1, k, device="cuda"), torch.zeros(B, 1, k, dtype=torch.int64, device="cuda")
    ops.step_logprobs(logits[rows].contiguous(), torch.zeros(B, dtype=torch.int64, device="cuda"), out=lp, col=0, top_n=k, top_out=top_lp, top_ids=top_id)
    st, pr = torch.full((B * k,), -1, dtype=torch.int64, device="cuda"), torch.zeros(B * k, device="cuda")
    cid, cpr = torch.full((B, 2, k), -1, dtype=torch.int64, device="cuda"), torch.zeros(B, 2, k, device="cuda")
    fin = torch.tensor([0, 0, 1], dtype=torch.uint8, device="cuda")
    ops.contrast_candidates(logits, k=k, step_tokens=st, prob=pr, chosen=chosen, k_prev=kp, finished=fin, cand_id=cid, cand_prob=cpr, col=1)
    assert torch.equal(st.view(B, k)[:2], top_id[:2, 0]) and torch.equal(cid[:2, 1], top_id[:2, 0])
    if k >= 2:
        assert st.view(B, k)[1, :2].tolist() == [7, 900]
    want = torch.exp(top_lp[:2, 0].double())
    assert ((pr.view(B, k)[:2].double() - want).abs() <= 4 * 2.0 ** -23 * want).all()       # 4 ulp through the expf
    assert torch.equal(cpr[:2, 1], pr.view(B, k)[:2])
    assert (st.view(B, k)[2] == -1).all() and (cid[2] == -1).all() and (cid[:, 0] == -1).all()       # a finished row writes nothing
    st2, pr2 = torch.zeros(B * kp * k, dtype=torch.int64, device="cuda"), torch.zeros(B * kp * k, device="cuda")
    ops.contrast_candidates(logits, k=k, step_tokens=st2, prob=pr2)        # without ``chosen``: row b
    assert torch.equal(st2.view(-1, k)[rows][:2], st.view(B, k)[:2]) and torch.equal(pr2.view(-1, k)[rows][:2], pr.view(B, k)[:2])


# ---- the unit hidden rows ----

def _check_unit_rows(u, res, g, b, eps):
    want = R.unit_rows(res, g, b, eps)
    model = np.abs(R.unit_rows_fp32(res, g, b, eps).astype(np.float64) - want).max()
    err = np.abs(u.astype(np.float64) - want).max()
    print(f"rows {res.shape}: max|d| = {err:.3e}, fp32 restatement {model:.3e}, tolerance {8 * model:.3e}")
    assert model > 0 and err <= 8 * model


@pytest.fixture(scope="module")
def lm():
    m = KosmosLanguage(vocab_size=102, dim=128, depth=2, ffn_dim=256, decoder_heads=2, _seed=3, _perturb=0.1, _max_positions=64).eval().to("cuda")
    m.precision = "fp32"
    return m


def _affine(lm, state):
    w = lm.decoder._pack(state["prec"])[0]
    ln = lm.decoder.layer_norm
    return w, ln.weight.detach().cpu().numpy(), ln.bias.detach().cpu().numpy(), float(w.eps)


@pytest.mark.parametrize("B,k", [(1, 2), (2, 3), (3, 6)])
def test_hidden_rows_of_a_step(lm, B, k):
    """M = 2 (the streaming step's residual pair), 6 (streaming, one stream) and 18 (tile GEMMs): the unit rows against float64 on the
    residual the launch returns, which is the step's own — the step's logits are its LayerNorm times the output projection."""
    T, M, D = 7, B * k, 128
    tok = torch.randint(0, 102, (B, T), generator=torch.Generator().manual_seed(B)).cuda()
    state = {"max_len": T + 3}
    lm.decoder._forward_incremental(tok, state, None, lm.precision)
    kc = state["kcache"]
    pos = torch.full((M,), T, dtype=torch.int32, device="cuda")
    state.update(positions=pos, pos_max=T)
    state["prefix"] = dict(ktail=torch.empty((2, M, 2, 1, 64), dtype=kc.dtype, device="cuda"), vtail=torch.empty((2, M, 2, 1, 64), dtype=kc.dtype, device="cuda"),
                           prefix_seq=(torch.arange(M, dtype=torch.int32, device="cuda") // k).to(torch.int32), prefix_len=pos)
    nxt = torch.randint(0, 102, (M,), generator=torch.Generator().manual_seed(M)).cuda()
    logits = lm.decoder._forward_incremental(None, state, None, lm.precision, next_token=nxt)[:, 0]
    w, g, b, eps = _affine(lm, state)
    u, res = torch.full((M, D), 9.0, device="cuda"), torch.zeros((M, D), device="cuda")
    ops.contrast_hidden(w, state["x_step"], u, workspace=state["step_ws"], prec=state["step_pid"], residual_out=res)
    assert int(state["error"].item()) == 0
    res_h, x_h = res.cpu().numpy(), state["x_step"].view(M, D).cpu().numpy()
    assert np.array_equal(res_h, x_h) == (M > 4)                           # up to four rows the stream is the pair x + xb
    _check_unit_rows(u.cpu().numpy(), res_h, g, b, eps)
    c = res_h.astype(np.float64) - res_h.astype(np.float64).mean(1, keepdims=True)
    h = c / np.sqrt((c * c).mean(1, keepdims=True) + eps) * g + b
    want = h @ lm.decoder.output_projection.weight.detach().cpu().numpy().astype(np.float64).T
    assert np.abs(logits.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max()            # (this residual is what the logits came from)


def test_hidden_rows_of_a_ragged_prefill(lm):
    B, T, D, cap = 3, 9, 128, 12
    tok = torch.randint(0, 102, (B, T), generator=torch.Generator().manual_seed(0)).cuda()
    state = {"max_len": cap, "keep_residual": True}
    lm.decoder._forward_incremental(tok, state, None, lm.precision)
    res = state["residual"]
    assert tuple(res.shape) == (B, T, D)
    w, g, b, eps = _affine(lm, state)
    lens = [9, 1, 4]
    out = torch.full((B, cap, D), 9.0, device="cuda")
    ops.contrast_hidden(w, res, out, lengths=torch.tensor(lens, dtype=torch.int32, device="cuda"))
    out_h, res_h = out.cpu().numpy(), res.cpu().numpy()
    for r, l in enumerate(lens):
        _check_unit_rows(out_h[r, :l], res_h[r, :l], g, b, eps)
        assert (out_h[r, l:] == 9.0).all()                                 # rows at or beyond a length stay untouched
    state2 = {"max_len": cap}
    lm.decoder._forward_incremental(tok, state2, None, lm.precision)
    assert "residual" not in state2                                        # kept on request only


def test_hidden_rows_at_full_width():
    """D = 2048 rows as they are (the prefill form needs no model: x is given)."""
    import ctypes as C
    x, g, b = R.hidden_rows(0, 18, 2048)
    w = ops.H.DecoderWeights()
    w.struct_bytes, w.layer_bytes = C.sizeof(ops.H.DecoderWeights), C.sizeof(ops.H.DecoderLayer)
    gt, bt = torch.from_numpy(g).cuda(), torch.from_numpy(b).cuda()
    w.dim, w.eps, w.ln_g, w.ln_b = 2048, R.EPS, gt.data_ptr(), bt.data_ptr()
    out = torch.zeros((2, 9, 2048), device="cuda")
    ops.contrast_hidden(w, torch.from_numpy(x).cuda().view(2, 9, 2048), out)
    _check_unit_rows(out.cpu().numpy().reshape(18, 2048), x, g, b, R.EPS)
