"""typical-p, epsilon and eta inside the sampler (kx_sample_logits_truncate) against tests/truncate_ref.py.

The kept set (``keep_mask`` / ``kept_count``) is compared with the float64 reference on the rows and cases that file shares with
tests/test_truncate.py, which asserts their band conditions on the CPU: up to V = 1500 the sets are EQUAL; above, every differing
element is unsure by the reference's rule (delta = 1e-4, eps_p = 1e-5) and at most 16 differ per row.  The token drawn must be the one
the old entry point draws from the same row with everything outside the new kept set banned."""
import functools

import numpy as np
import pytest
import torch

import truncate_ref as TR
from kosmosx import _hip as H
from kosmosx import ops

pytestmark = pytest.mark.gpu

VS = [5, 37, 502, 1500, 4099, 64007]
GROUPS = dict(alone=TR.ALONE, fronted=TR.FRONTED, together=TR.TOGETHER)


@functools.lru_cache(maxsize=None)
def _rows(V):
    r = TR.case_rows(V)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _reference(V, group, i):
    """The reference of one shared case, computed once."""
    return TR.case_keep(_rows(V), GROUPS[group][i])


def _debug(rows, **kw):
    tok, kept, mask = ops.sample_logits(torch.tensor(rows, device="cuda"), return_debug=True, **kw)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), kept.cpu().numpy(), mask.cpu().numpy().astype(bool)


def _launch_kw(rows, case):
    kw = dict(case, seed=11, position=5)
    if kw.pop("history", False):
        h = TR.case_history(rows)
        kw.update(history=torch.tensor(np.concatenate([h, np.zeros((len(rows), 1), dtype=np.int64)], axis=1), device="cuda"),
                  hist_len=h.shape[1])
    if "top_k" in kw:
        kw["top_k"] = min(kw["top_k"], rows.shape[1] - 1)
    return kw


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("group", list(GROUPS))
def test_the_kept_set_is_the_references(group, V):
    """Each filter alone, each behind top-k / top-p / min-p / the repetition penalty, and all three together."""
    rows = _rows(V)
    differing = 0
    for i, case in enumerate(GROUPS[group]):
        tok, kept, mask = _debug(rows, **_launch_kw(rows, case))
        for b, (x, keep, unsure, stages, s0) in enumerate(_reference(V, group, i)):
            diff = mask[b] != keep
            if V <= TR.EXACT_V:
                assert not diff.any(), (case, b, np.nonzero(diff)[0][:8])
            else:
                assert not (diff & ~unsure).any() and diff.sum() <= 16, (case, b, np.nonzero(diff & ~unsure)[0][:8], int(diff.sum()))
            differing += int(diff.sum())
            assert kept[b] == mask[b].sum() >= 1 and mask[b, tok[b]], (case, b)
            assert not (mask[b] & ~s0).any()                                 # never anything the earlier filters dropped
    print(f"{group} V={V}: {differing} differing elements, all unsure")


@pytest.mark.parametrize("V", [37, 1500, 64007])
@pytest.mark.parametrize("top_k", [0, 12])
def test_the_draw_equals_the_old_entry_point_on_the_banned_row(V, top_k):
    """top_p = 1: the token equals kx_sample_logits' on the same row with the ids outside the kept set (the launch's own keep_mask,
    which the test above holds to the reference) at -inf — same seed, position and sequence id — in the uniform and in the ragged
    form with advance 0 and 1, and the ragged form advances ``positions``."""
    dev = torch.device("cuda")
    rows = _rows(V)
    B = rows.shape[0]
    T = 0.9
    on = torch.from_numpy(rows.copy()).to(dev)
    seq = torch.tensor([4, 9, 2, 7, 1, 30, 5, 8][:B], dtype=torch.int64, device=dev)
    differ = 0
    for trunc in (dict(typical_p=0.9), dict(epsilon_cutoff=2e-3), dict(eta_cutoff=0.02), dict(typical_p=0.95, epsilon_cutoff=3e-4, eta_cutoff=2e-3)):
        kw = dict(temperature=T, seed=77, sequence_ids=seq)
        _, kept, mask = ops.sample_logits(on, top_k=top_k, position=3, return_debug=True, **kw, **trunc)
        off = on.masked_fill(mask == 0, float("-inf"))
        real = 0
        for position in (3, 17, 40):
            got = ops.sample_logits(on, top_k=top_k, position=position, **kw, **trunc)
            want = ops.sample_logits(off, position=position, **kw)
            assert torch.equal(got, want), (trunc, position)
            differ += int(not torch.equal(got, ops.sample_logits(on, top_k=top_k, position=position, **kw)))
            base = torch.arange(B, dtype=torch.int32, device=dev) * 3 + position
            base[0] = position - 1
            pos, pos2 = base.clone(), base.clone()
            got_r = ops.sample_logits(on, top_k=top_k, positions=pos, advance=1, **kw, **trunc)
            want_r = ops.sample_logits(off, positions=pos2, advance=1, **kw)
            assert torch.equal(got_r, want_r) and got_r[0] == got[0]         # (row 0 drew at position - 1 + 1)
            assert torch.equal(pos, base + 1) and torch.equal(pos, pos2)
            still = pos.clone()
            again = ops.sample_logits(on, top_k=top_k, positions=pos, advance=0, **kw, **trunc)   # advance = 0: the positions stay
            assert torch.equal(again, ops.sample_logits(off, positions=pos2, advance=0, **kw)) and torch.equal(pos, still)
            real += int((kept >= 2).sum())
        assert real > 0                                                      # a real draw in some row
    if top_k == 0 and V > 37:
        assert differ > 0                                                    # without the filters some draw lands outside the set


@pytest.mark.parametrize("V", [502, 4099])
def test_a_rows_result_does_not_depend_on_the_batch_or_on_its_index(V):
    rows = _rows(V)
    B = rows.shape[0]
    seq = torch.arange(100, 100 + B, dtype=torch.int64, device="cuda")
    kw = dict(typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3, top_k=min(200, V - 1), temperature=0.8, seed=5, position=9)
    tok, kept, mask = _debug(rows, sequence_ids=seq, **kw)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    tok_p, kept_p, mask_p = _debug(rows[perm], sequence_ids=seq[torch.from_numpy(perm).cuda()].contiguous(), **kw)
    assert np.array_equal(tok_p, tok[perm]) and np.array_equal(kept_p, kept[perm]) and np.array_equal(mask_p, mask[perm])
    for b in (0, 4, 7):
        t1, k1, m1 = _debug(rows[b:b + 1], sequence_ids=seq[b:b + 1].contiguous(), **kw)
        assert t1[0] == tok[b] and k1[0] == kept[b] and np.array_equal(m1[0], mask[b]), b
    again = _debug(rows, sequence_ids=seq, **kw)
    assert np.array_equal(again[0], tok) and np.array_equal(again[2], mask)  # two calls: identical


def test_typical_p_drops_the_arg_max_on_the_hand_made_row():
    """p = (0.6, 0.3, 0.05, 0.05): token 1 is the most typical one (tests/test_truncate.py spells the numbers out)."""
    row = np.log(np.array([[0.6, 0.3, 0.05, 0.05]])).astype(np.float32).repeat(3, axis=0)
    tok, kept, mask = _debug(row, typical_p=0.25, seed=3)
    assert mask.tolist() == [[False, True, False, False]] * 3 and kept.tolist() == [1] * 3 and tok.tolist() == [1] * 3
    _, kept, mask = _debug(row, typical_p=0.5, seed=3)
    assert mask.tolist() == [[True, True, False, False]] * 3 and kept.tolist() == [2] * 3
    _, kept, mask = _debug(row, typical_p=0.92, seed=3)
    assert mask.all() and kept.tolist() == [4] * 3                           # the ties at 0.05 stay together
    for t in (0.25, 0.5, 0.92):
        assert np.array_equal(mask_of(row, typical_p=t), np.stack([TR.sample_keep(r, typical_p=t)[1] for r in row]))


def mask_of(rows, **kw):
    return _debug(rows, seed=1, **kw)[2]


def test_eta_sees_what_epsilon_left():
    """p = (0.5, 0.3, 0.15, 0.04, 0.01), epsilon = 0.045, eta = 0.2: either alone leaves tokens 0-2; eta behind epsilon meets a
    lower entropy, its cut-off rises from 0.139 to 0.166 and token 2 (0.158 of what is left) goes as well."""
    row = np.log(np.array([[0.5, 0.3, 0.15, 0.04, 0.01]])).astype(np.float32).repeat(2, axis=0)
    assert mask_of(row, epsilon_cutoff=0.045).tolist() == [[True, True, True, False, False]] * 2
    assert mask_of(row, eta_cutoff=0.2).tolist() == [[True, True, True, False, False]] * 2
    assert mask_of(row, epsilon_cutoff=0.045, eta_cutoff=0.2).tolist() == [[True, True, False, False, False]] * 2
    assert mask_of(row, eta_cutoff=0.02).tolist() == [[True, True, True, True, False]] * 2
    assert mask_of(row, epsilon_cutoff=0.045, eta_cutoff=0.02).tolist() == [[True, True, True, False, False]] * 2
    # typical-p first: t = 0.5 leaves (0.5, 0.3) renormalised to (0.625, 0.375); epsilon at 0.4 then keeps the maximum alone
    assert mask_of(row, typical_p=0.5).tolist() == [[True, True, False, False, False]] * 2
    assert mask_of(row, typical_p=0.5, epsilon_cutoff=0.4).tolist() == [[True, False, False, False, False]] * 2
    assert mask_of(row, epsilon_cutoff=0.4).tolist() == [[True, False, False, False, False]] * 2
    assert mask_of(row, typical_p=0.5, epsilon_cutoff=0.35).tolist() == [[True, True, False, False, False]] * 2   # 0.375 >= 0.35, 0.3 was not


def test_the_arg_max_of_what_typical_p_left_survives_the_cut_offs():
    """p = (0.5, 0.22, 0.18, 0.1): H = 1.219 and |-log p - H| = 0.53, 0.30, 0.50, 1.08, so t = 0.3 leaves tokens 1 and 2 — not the
    row's arg max.  Renormalised they hold (0.55, 0.45): epsilon at 0.9 keeps only the maximum of what it was handed, token 1, and
    eta at 0.99 (cut-off min(0.99, 0.995 e^-0.688 = 0.50)) drops token 2 as well."""
    row = np.log(np.array([[0.5, 0.22, 0.18, 0.1]])).astype(np.float32)
    want = TR.sample_keep(row[0], typical_p=0.3)[1]
    assert want.tolist() == [False, True, True, False] and np.array_equal(mask_of(row, typical_p=0.3)[0], want)
    for kw in (dict(epsilon_cutoff=0.9), dict(eta_cutoff=0.99)):
        assert TR.sample_keep(row[0], typical_p=0.3, **kw)[1].tolist() == [False, True, False, False]
        tok, kept, mask = _debug(row, typical_p=0.3, seed=2, **kw)
        assert mask[0].tolist() == [False, True, False, False] and kept[0] == 1 and tok[0] == 1


def test_plus_inf_ties_underflow_and_rows_without_a_candidate():
    V = 300
    rows = np.array(_rows(502)[:5, :V])
    rows[0, [7, 250]] = np.inf
    rows[1, 0] = np.inf
    rows[1, 5] = -np.inf
    rows[2] = -200.0                                                         # everything but the maximum underflows 2^-40 relative to it
    rows[2, 33] = 0.0
    rows[3] = -np.inf                                                        # no candidate: a pad, and the row is finished
    finished = torch.tensor([0, 0, 0, 0, 1], dtype=torch.uint8, device="cuda")   # row 4 came in finished
    for kw in (dict(typical_p=0.5), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3), dict(typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=1e-3)):
        fin = finished.clone()
        tok, kept, mask = _debug(rows, seed=9, pad_token_id=299, finished=fin, **kw)
        assert np.nonzero(mask[0])[0].tolist() == [7, 250] and tok[0] in (7, 250), kw
        assert np.nonzero(mask[1])[0].tolist() == [0] and tok[1] == 0, kw
        assert np.nonzero(mask[2])[0].tolist() == [33] and tok[2] == 33 and kept[2] == 1, kw
        assert not mask[3].any() and kept[3] == 0 and tok[3] == 299, kw
        assert not mask[4].any() and kept[4] == 0 and tok[4] == 299, kw
        assert fin.tolist() == [0, 0, 0, 1, 1], kw
        for b in (0, 1, 2):
            assert np.array_equal(mask[b], TR.sample_keep(rows[b], **kw)[1]), (kw, b)


def test_greedy_ignores_all_three():
    rows = _rows(1500)
    t = torch.from_numpy(rows.copy()).cuda()
    kw = dict(typical_p=0.2, epsilon_cutoff=0.5, eta_cutoff=0.5)
    assert torch.equal(ops.sample_logits(t, do_sample=False, **kw), ops.sample_logits(t, do_sample=False))
    assert torch.equal(ops.sample_logits(t, temperature=0.0, **kw), torch.from_numpy(rows.argmax(1)).cuda())
    _, kept, mask = ops.sample_logits(t, do_sample=False, return_debug=True, **kw)
    assert bool(mask.all()) and kept.tolist() == [1500] * 8                  # greedy reports the candidates, as ever


def test_the_defaults_call_the_old_entry_points(monkeypatch):
    t = torch.from_numpy(_rows(37).copy()).cuda()
    real, called = H.load(), []

    class Spy:
        def __getattr__(self, name):
            if name.startswith("kx_sample_logits"):
                called.append(name)
            return getattr(real, name)
    monkeypatch.setattr(H, "load", lambda: Spy())
    pos = torch.arange(8, dtype=torch.int32, device="cuda")
    ops.sample_logits(t, seed=1)
    ops.sample_logits(t, seed=1, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0)
    ops.sample_logits(t, seed=1, positions=pos, advance=1, typical_p=1)
    ops.sample_logits(t, seed=1, min_p=0.25, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    assert called == ["kx_sample_logits", "kx_sample_logits", "kx_sample_logits_ragged", "kx_sample_logits_min_p"]
    for kw in (dict(typical_p=0.9), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3), dict(min_p=0.1, eta_cutoff=1e-3)):
        ops.sample_logits(t, seed=1, **kw)
        ops.sample_logits(t, seed=1, positions=pos, advance=1, **kw)
    assert called[4:] == ["kx_sample_logits_truncate"] * 8
    for kw in (dict(typical_p=0.0), dict(typical_p=1.5), dict(epsilon_cutoff=1.0), dict(eta_cutoff=-0.1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ops.sample_logits(t, **kw)
