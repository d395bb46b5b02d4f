"""min-p inside the sampler (kx_sample_logits_min_p) against tests/shape_ref.py: the kept set is an exact threshold compare, so
``keep_mask`` / ``kept_count`` must equal the reference's, and the token drawn must be the one the old entry point draws from the same
row with everything outside the min-p set banned.  Apart from the min_p = 1 case every x_i lies at least 1e-4 away from the
threshold x_max + log(min_p) (asserted below on the CPU), so the last bit of the host's log decides nothing."""
import numpy as np
import pytest
import torch

import sampling_ref as R
import shape_ref as SR
from kosmosx import _hip as H
from kosmosx import ops

pytestmark = pytest.mark.gpu

VS = [37, 1500, 64007]                                      # below one pass of the 1024 threads, above it, the product's vocabulary
B = 3


def _rows(V, seed, scale=3.0):
    return (np.random.default_rng(seed).standard_normal((B, V)) * scale).astype(np.float32)


def _clear_of_the_threshold(x, m):
    thr = float(x.max()) + float(SR.log_min_p(m))
    assert np.abs(x[x > -np.inf].astype(np.float64) - thr).min() >= 1e-4, "choose another row: an x_i sits on the min-p threshold"


def _debug(rows, **kw):
    dev = torch.device("cuda")
    tok, kept, mask = ops.sample_logits(torch.from_numpy(rows).to(dev), return_debug=True, **kw)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), kept.cpu().numpy(), mask.cpu().numpy().astype(bool)


def _check_keep(rows, *, min_p, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, history=None, clear=True):
    kw = dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, seed=11, position=5)
    hist = None
    if history is not None:
        hist = torch.tensor(np.concatenate([history, np.zeros((B, 1), dtype=np.int64)], axis=1), device="cuda")
        kw.update(repetition_penalty=repetition_penalty, history=hist, hist_len=history.shape[1])
    tok, kept, mask = _debug(rows, **kw)
    fewer = 0
    for b in range(rows.shape[0]):
        x, keep = SR.sample_keep(rows[b], temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p,
                                 repetition_penalty=repetition_penalty, history=None if history is None else history[b])
        if clear:
            _clear_of_the_threshold(x, min_p)
        assert np.array_equal(mask[b], keep), (b, np.nonzero(mask[b] != keep)[0][:8])
        assert kept[b] == keep.sum() and keep[tok[b]] and keep[int(np.argmax(x))]
        fewer += int(keep.sum() < R.filter_row(x, top_k, top_p)[0].sum())
    return fewer


@pytest.mark.parametrize("V", VS)
def test_min_p_alone(V):
    rows = _rows(V, seed=V)
    assert _check_keep(rows, min_p=0.1) == B                                # min-p binds in every row
    _check_keep(rows, min_p=0.02, temperature=0.7)
    _check_keep(rows, min_p=0.6, temperature=1.6)


@pytest.mark.parametrize("V", VS)
def test_min_p_with_top_k_and_with_top_p(V):
    rows = _rows(V, seed=V + 1)
    assert _check_keep(rows, min_p=0.2, top_k=min(20, V - 1)) > 0            # min-p cuts into what top-k kept
    assert _check_keep(rows, min_p=0.02, top_k=5) == 0                      # ... and here top-k is the tighter one
    assert _check_keep(rows, min_p=0.3, top_p=0.9) > 0
    assert _check_keep(rows, min_p=0.02, top_p=0.5) == 0
    _check_keep(rows, min_p=0.05, top_k=min(30, V - 1), top_p=0.8, temperature=0.9)


@pytest.mark.parametrize("V", VS)
def test_min_p_with_the_repetition_penalty(V):
    rows = _rows(V, seed=V + 2)
    history = np.stack([np.argsort(-rows[b])[:4] for b in range(B)]).astype(np.int64)   # the four most likely ids: the penalty moves the maximum
    assert _check_keep(rows, min_p=0.1, repetition_penalty=1.7, history=history) > 0
    _check_keep(rows, min_p=0.1, repetition_penalty=0.8, history=history, top_k=min(25, V - 1))


def test_the_transformers_order_top_p_before_min_p():
    """log([0.6, 0.3, 0.05, 0.05]), T = 1, top_p = 0.65, min_p = 0.1: top-p keeps {0, 1} (the mass ahead of token 1 is 0.6 < 0.65),
    min-p then keeps both (0.3 >= 0.06).  Min-p first would leave {0, 1} with token 0 at 0.667 >= 0.65 of the renormalised mass:
    token 0 alone."""
    row = np.log(np.array([[0.6, 0.3, 0.05, 0.05]])).astype(np.float32).repeat(B, axis=0)
    for b in range(B):
        _clear_of_the_threshold(R.scaled(row[b], 1.0), 0.1)
    _, kept, mask = _debug(row, top_p=0.65, min_p=0.1, seed=3)
    assert mask.tolist() == [[True, True, False, False]] * B and kept.tolist() == [2] * B
    _check_keep(row, min_p=0.1, top_p=0.65)


@pytest.mark.parametrize("V", [37, 1500])
def test_min_p_one_keeps_exactly_the_ties(V):
    rows = _rows(V, seed=V + 3)
    for b in range(B):
        top = rows[b].max()
        rows[b, [1 + b, V - 1 - b, V // 2]] = top                            # three more ties at the maximum
        rows[b, 0] = np.nextafter(top, np.float32(-np.inf))                  # one ulp below: not a tie
    _, kept, mask = _debug(rows, min_p=1.0, seed=5)
    for b in range(B):
        assert np.array_equal(mask[b], rows[b] == rows[b].max()) and kept[b] == 4 and not mask[b, 0]
    _check_keep(rows, min_p=1.0, clear=False)
    _check_keep(rows, min_p=1.0, temperature=0.7, top_k=2, clear=False)      # (ties at the top-k threshold are all kept, as ever)


def test_rows_with_plus_inf_logits():
    V = 300
    rows = _rows(V, seed=8)
    rows[0, [7, 250]] = np.inf
    rows[1, 0] = np.inf
    rows[1, 5] = -np.inf
    tok, kept, mask = _debug(rows, min_p=0.5, seed=9)
    assert np.nonzero(mask[0])[0].tolist() == [7, 250] and np.nonzero(mask[1])[0].tolist() == [0] and tok[1] == 0 and tok[0] in (7, 250)
    _check_keep(rows, min_p=0.5, clear=False)                                # (+inf ties: the threshold is +inf; row 2 is an ordinary row)
    _clear_of_the_threshold(R.scaled(rows[2], 1.0), 0.5)
    _check_keep(rows, min_p=0.5, top_p=0.9, top_k=40, clear=False)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("top_k", [0, 12])
def test_the_draw_equals_the_old_entry_point_on_the_banned_row(V, top_k):
    """top_p = 1: the token equals kx_sample_logits' on the same row with the ids outside the min-p set at -inf — same seed, position
    and sequence id — in the uniform and in the ragged form, and the ragged form advances ``positions``."""
    dev = torch.device("cuda")
    rows = _rows(V, seed=V + 4)
    m, T = 0.05, 0.9
    banned = rows.copy()
    sizes = []
    for b in range(B):
        x, keep = SR.sample_keep(rows[b], temperature=T, top_k=top_k, min_p=m)
        _clear_of_the_threshold(x, m)
        banned[b, ~keep] = -np.inf
        sizes.append(int(keep.sum()))
    assert min(sizes) >= 2                                                   # a real draw in every row
    seq = torch.tensor([4, 9, 2], dtype=torch.int64, device=dev)
    on, off = torch.from_numpy(rows).to(dev), torch.from_numpy(banned).to(dev)
    differ = 0
    for position in (3, 17, 40, 41):
        kw = dict(temperature=T, seed=77, sequence_ids=seq)
        got = ops.sample_logits(on, top_k=top_k, min_p=m, position=position, **kw)
        want = ops.sample_logits(off, position=position, **kw)
        assert torch.equal(got, want)
        differ += int(not torch.equal(got, ops.sample_logits(on, top_k=top_k, position=position, **kw)))
        pos = torch.tensor([position - 1, position + 5, position], dtype=torch.int32, device=dev)
        pos2 = pos.clone()
        got_r = ops.sample_logits(on, top_k=top_k, min_p=m, positions=pos, advance=1, **kw)
        want_r = ops.sample_logits(off, positions=pos2, advance=1, **kw)
        assert torch.equal(got_r, want_r) and got_r[0] == got[0]             # (row 0 drew at position - 1 + 1)
        assert pos.tolist() == [position, position + 6, position + 1] and torch.equal(pos, pos2)
        still = pos.clone()
        again = ops.sample_logits(on, top_k=top_k, min_p=m, positions=pos, advance=0, **kw)       # advance = 0: the positions stay
        assert torch.equal(again, ops.sample_logits(off, positions=pos2, advance=0, **kw)) and torch.equal(pos, still)
    if top_k == 0 and V > 37:
        assert differ > 0                                                    # without min-p some draw lands outside the set: the filter is real


def test_min_p_is_ignored_under_greedy():
    rows = _rows(1500, seed=6)
    dev = torch.device("cuda")
    t = torch.from_numpy(rows).to(dev)
    assert torch.equal(ops.sample_logits(t, do_sample=False, min_p=0.9), ops.sample_logits(t, do_sample=False))
    assert torch.equal(ops.sample_logits(t, temperature=0.0, min_p=0.9), torch.from_numpy(rows.argmax(1)).to(dev))


def test_min_p_zero_calls_the_old_entry_points(monkeypatch):
    dev = torch.device("cuda")
    t = torch.from_numpy(_rows(37, seed=1)).to(dev)
    real, called = H.load(), []

    class Spy:
        def __getattr__(self, name):
            if name.startswith("kx_sample_logits"):
                called.append(name)
            return getattr(real, name)
    monkeypatch.setattr(H, "load", lambda: Spy())
    pos = torch.tensor([1, 2, 3], dtype=torch.int32, device=dev)
    ops.sample_logits(t, seed=1)
    ops.sample_logits(t, seed=1, min_p=0.0)
    ops.sample_logits(t, seed=1, positions=pos, advance=1, min_p=0)
    assert called == ["kx_sample_logits", "kx_sample_logits", "kx_sample_logits_ragged"]
    ops.sample_logits(t, seed=1, min_p=0.25)
    ops.sample_logits(t, seed=1, positions=pos, advance=1, min_p=0.25)
    assert called[3:] == ["kx_sample_logits_min_p"] * 2
    with pytest.raises(ValueError, match="min_p"):
        ops.sample_logits(t, min_p=1.5)
