"""kx_sample_logits on the device against the CPU restatement of its contract (tests/sampling_ref.py).

Bounds (from the number formats, not from the kernel's output): eps_p = 1e-5 of the total mass for the top-p boundary
(fp32 exp of an fp32 argument with |x - max| < 20 is off by at most ~20 * 2^-24 = 1.2e-6 relative, the integer sum adds
less), eps_g = 1e-4 on the Gumbel score (the fp32 chain x - log(-log u): a few 1e-6), and at most 1 % of a test's draws
may need the eps_g escape."""
import numpy as np
import pytest
import torch

import sampling_ref as R

pytestmark = pytest.mark.gpu

EPS_P, EPS_G = 1e-5, 1e-4
SHAPES = [(1, 1, 1.0), (5, 7, 2.0), (16, 502, 3.0), (40, 1002, 1.0), (5, 32002, 2.0), (16, 64007, 1.0), (1, 64007, 3.0),
          (40, 502, 2.0), (1, 32002, 1.0)]


def _logits(B, V, s, seed, pad_cols=0):
    """randn * s with planted exact ties (at the maximum and below it), -inf entries, one NaN and, from five rows on, one
    all--inf row.  Returns the [B, V] view of a [B, V + pad_cols] tensor."""
    g = torch.Generator().manual_seed(seed)
    full = torch.randn(B, V + pad_cols, generator=g) * s
    full[:, V:] = 1e30                                           # beyond V: must never be read as a logit
    x = full[:, :V]
    if V >= 7:
        for b in range(B):
            top = float(x[b].max())
            if b % 2 == 0:
                x[b, 5], x[b, 2] = top + 1.0, top + 1.0          # tie at the maximum: index 2 wins under greedy
            x[b, 3] = x[b, 6] = float(x[b, 1])                   # tie below it
            x[b, 4] = -float("inf")
        x[0, 0] = float("nan")
        if V >= 100:
            x[:, 50:60] = -float("inf")
    if B >= 5:
        x[4] = -float("inf")
    return x


def _run(xd, **kw):
    from kosmosx import ops
    tok, kept, mask = ops.sample_logits(xd, return_debug=True, **kw)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), kept.cpu().numpy(), mask.cpu().numpy().astype(bool)


@pytest.mark.parametrize("B,V,s", SHAPES)
def test_greedy_is_the_reference_arg_max(B, V, s):
    x = _logits(B, V, s, seed=B * 7 + V, pad_cols=5 if V == 502 else 0)
    xd = x._base.cuda()[:, :V]                                   # V = 502: rows 5 columns apart from dense (ld > V)
    assert xd.stride(0) == V + (5 if V == 502 else 0)
    fin = torch.zeros(B, dtype=torch.uint8, device="cuda")
    for kw in (dict(do_sample=False), dict(do_sample=True, temperature=0.0, top_k=3, top_p=0.5)):
        fin.zero_()
        tok, kept, mask = _run(xd, finished=fin, pad_token_id=1, **kw)
        for b in range(B):
            ref = R.sample_row(x[b].numpy(), do_sample=False)
            assert tok[b] == ref["token"], (b, tok[b], ref["token"])
            assert bool(fin[b].item()) == ref["none"]
            assert np.array_equal(mask[b], ref["keep"]) and kept[b] == int(ref["keep"].sum())


@pytest.mark.parametrize("B,V,s", SHAPES)
@pytest.mark.parametrize("T,k,p", [(0.8, 50, 0.9), (1.0, 0, 0.95), (1.3, 50, 1.0), (0.7, 5, 0.5)])
def test_kept_set_and_drawn_token(B, V, s, T, k, p):
    x = _logits(B, V, s, seed=B * 11 + V, pad_cols=3 if V == 1002 else 0)
    xd = x._base.cuda()[:, :V]                                   # V = 1002: rows 3 columns apart from dense (ld > V), sampled
    assert xd.stride(0) == V + (3 if V == 1002 else 0)
    seq = torch.arange(100, 100 + B, dtype=torch.int64, device="cuda")
    tok, kept, mask = _run(xd, temperature=T, top_k=k, top_p=p, seed=17, position=23, sequence_ids=seq)
    used_eps = 0
    for b in range(B):
        ref = R.sample_row(x[b].numpy(), temperature=T, top_k=k, top_p=p, seed=17, position=23, sequence_id=100 + b)
        if ref["none"]:
            assert tok[b] == 1 and kept[b] == 0 and not mask[b].any()
            continue
        assert kept[b] == int(mask[b].sum())
        assert np.array_equal(mask[b] | ref["keepk"], ref["keepk"]), "kept a token top-k dropped"
        if p >= 1.0:
            assert np.array_equal(mask[b], ref["keepk"])          # counts are exact integers
            thr_ties = int((ref["x"] == ref["x"][ref["keepk"]].min()).sum())
            if 0 < k < V and thr_ties == 1:
                assert kept[b] == min(k, int((ref["x"] > -np.inf).sum()))
        else:
            p32 = float(np.float32(p))
            must = ref["keepk"] & (ref["ahead"] < p32 - EPS_P)
            never = ref["keepk"] & (ref["ahead"] > p32 + EPS_P)
            assert mask[b][must].all() and not mask[b][never].any()
            assert int((ref["keepk"] & ~must & ~never).sum()) <= 6, "the band hides more than 0-2 tokens and a planted tie"
        assert mask[b][tok[b]]
        used_eps += R.check_draw(int(tok[b]), ref, EPS_P, EPS_G, p) == "eps"
    assert used_eps <= 0.01 * B


def test_many_draws_use_the_escape_rarely():
    """1 % cap of the drawn-token rule over a population where 1 % is more than one draw: 64 positions x 40 rows."""
    from kosmosx import ops
    B, V = 40, 1002
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, V, generator=g) * 2
    xd = x.cuda()
    used = 0
    for pos in range(64):
        tok = ops.sample_logits(xd, temperature=0.8, top_k=50, top_p=0.9, seed=3, position=pos).cpu().numpy()
        for b in range(B):
            ref = R.sample_row(x[b].numpy(), temperature=0.8, top_k=50, top_p=0.9, seed=3, position=pos, sequence_id=b)
            used += R.check_draw(int(tok[b]), ref, EPS_P, EPS_G, 0.9) == "eps"
    assert used <= 0.01 * 64 * B, used


def test_repetition_penalty_and_history():
    from kosmosx import ops
    B, V = 5, 1002
    x = _logits(B, V, 2.0, seed=9)
    g = torch.Generator().manual_seed(1)
    hist = torch.zeros(B, 41, dtype=torch.int64)
    hist[:, :40] = torch.randint(0, V, (B, 40), generator=g)
    for b in range(B):
        hist[b, 0] = int(torch.nan_to_num(x[b], nan=-1e30).argmax())   # penalise the leader ...
        hist[b, 7] = hist[b, 0]                                        # ... once, although it occurs twice
    hd = hist.cuda()
    tok, kept, mask = _run(x.cuda(), temperature=0.9, top_k=20, top_p=0.9, repetition_penalty=1.7, seed=2, position=40,
                           history=hd, hist_len=40)
    for b in range(B):
        ref = R.sample_row(x[b].numpy(), temperature=0.9, top_k=20, top_p=0.9, repetition_penalty=1.7, seed=2, position=40,
                           sequence_id=b, history=hist[b, :40].numpy())
        R.check_draw(int(tok[b]), ref, EPS_P, EPS_G, 0.9)
        assert np.array_equal(mask[b] | ref["keepk"], ref["keepk"])
    assert np.array_equal(hd[:, 40].cpu().numpy(), tok)               # appended
    assert torch.equal(hd[:, :40].cpu(), hist[:, :40])
    # greedy: the leader at 4.0 against a runner-up at 3.0, r = 1.2: penalised once it still leads (3.33), twice it would not
    y = torch.zeros(1, 16)
    y[0, 3], y[0, 9] = 4.0, 3.0
    h = torch.tensor([[3, 3, 3, 0]], dtype=torch.int64).cuda()
    t = ops.sample_logits(y.cuda(), do_sample=False, repetition_penalty=1.2, history=h, hist_len=3)
    assert int(t[0]) == 3
    t = ops.sample_logits(y.cuda(), do_sample=False, repetition_penalty=1.5, history=h, hist_len=3)
    assert int(t[0]) == 9


def test_batch_invariance_and_reproducibility():
    from kosmosx import ops
    V = 32002
    x = _logits(7, V, 2.0, seed=3)
    xd = x.cuda()
    kw = dict(temperature=0.8, top_k=50, top_p=0.9, seed=99, position=130)
    seq = torch.tensor([10, 11, 12, 5, 14, 15, 16], dtype=torch.int64, device="cuda")
    t7, k7, m7 = _run(xd, sequence_ids=seq, **kw)
    t7b, k7b, m7b = _run(xd, sequence_ids=seq, **kw)
    assert np.array_equal(t7, t7b) and np.array_equal(k7, k7b) and np.array_equal(m7, m7b)
    t1, k1, m1 = _run(xd[3:4].clone(), sequence_ids=seq[3:4].clone(), **kw)
    assert t1[0] == t7[3] and k1[0] == k7[3] and np.array_equal(m1[0], m7[3])
    base, other_seed, other_pos = [], [], []
    row = xd[3:4].clone()
    for pos in range(64):
        base.append(int(ops.sample_logits(row, temperature=1.0, seed=1, position=pos)[0]))
        other_seed.append(int(ops.sample_logits(row, temperature=1.0, seed=2, position=pos)[0]))
        other_pos.append(int(ops.sample_logits(row, temperature=1.0, seed=1, position=pos + 64)[0]))
    assert base != other_seed and base != other_pos and len(set(base)) > 1


def test_distribution_on_the_device():
    """V = 64, one row repeated 65 536 times with distinct sequence ids, one launch; chi-square against the exact filtered
    softmax at significance 1e-6."""
    from kosmosx import ops
    V, N = 64, 65536
    row = torch.randn(V, generator=torch.Generator().manual_seed(4)) * 2
    T, k, p = 0.8, 40, 0.9
    x = R.scaled(row.numpy(), T)
    keep, ahead, _ = R.filter_row(x, k, p)
    assert (np.abs(ahead[np.isfinite(ahead)] - np.float32(p)) > 1e-3).all()       # nothing near the boundary: the set is exact
    e = np.where(keep, np.exp(x.astype(np.float64) - x.max()), 0.0)
    prob = e / e.sum()
    xd = row.cuda()[None].repeat(N, 1).contiguous()
    tok = ops.sample_logits(xd, temperature=T, top_k=k, top_p=p, seed=8, position=3,
                            sequence_ids=torch.arange(N, dtype=torch.int64, device="cuda")).cpu().numpy()
    counts = np.bincount(tok, minlength=V)
    assert counts[~keep].sum() == 0
    chi2 = float(((counts[keep] - N * prob[keep]) ** 2 / (N * prob[keep])).sum())
    assert int(keep.sum()) - 1 == 6                                               # seeded: the degrees of freedom are fixed
    assert chi2 < 38.2583, chi2                                                   # chi-square upper 1e-6 point, 6 dof


def test_stop_state():
    from kosmosx import ops
    B, V = 3, 502
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(6))
    xd = x.cuda()
    eos = int(x[0].argmax())
    assert eos != int(x[1].argmax()) and eos != int(x[2].argmax())
    fin = torch.zeros(B, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 4), -7, dtype=torch.int64, device="cuda")
    hist = torch.full((B, 6), -1, dtype=torch.int64, device="cuda")
    t0 = ops.sample_logits(xd, do_sample=False, finished=fin, eos_token_id=eos, pad_token_id=1, out_tokens=out, out_col=1,
                           history=hist, hist_len=2).clone()
    assert t0.tolist() == [int(x[b].argmax()) for b in range(B)] and fin.tolist() == [1, 0, 0]
    t1 = ops.sample_logits(xd, do_sample=False, finished=fin, eos_token_id=eos, pad_token_id=1, out_tokens=out, out_col=2,
                           history=hist, hist_len=3)
    assert t1.tolist() == [1, t0[1].item(), t0[2].item()] and fin.tolist() == [1, 0, 0]
    assert out[:, 1].tolist() == t0.tolist() and out[:, 2].tolist() == t1.tolist()
    assert out[:, 0].tolist() == [-7] * B and out[:, 3].tolist() == [-7] * B
    assert hist[:, 2].tolist() == t0.tolist() and hist[:, 3].tolist() == t1.tolist() and hist[:, 4].tolist() == [-1] * B
