"""kx_step_logprobs (csrc/kx_rowops.hip): the log-prob of the token a generation step drew and the row's top-n (log-prob, id) pairs,
one launch, one workgroup per row — against float64 (tests/logprob_ref.py) and, bit for bit, against kx_token_logprob.

V in {1, 5, 255, 256, 257, 1000, 64007} (below, at and above the 256 threads' stride; the real, odd vocabulary), B in {1, 3}, top_n in
{0, 1, 5, 16} (no selection and each of the kernel's three list sizes), a row pitch of V + 5 whose gap holds 1e30: a kernel that read
it would take it for the maximum.  Four kinds of row: normals x 8; integers in -3..3, the 3s placed so that ties fall inside one
thread (ids 256 apart), in neighbouring lanes and across waves; -inf at half the ids; -inf everywhere but one id."""
import functools

import pytest
import torch

import logprob_ref as R
from kosmosx import _hip as H
from kosmosx import ops
from test_logprobs import KX_ERR_INVALID_ARG, step_logprobs_refusals

pytestmark = pytest.mark.gpu

BOUND = 2e-5            # absolute, over float64: the project's bound for this arithmetic (tests/test_token_logprob_gpu.py)
VS = [1, 5, 255, 256, 257, 1000, 64007]
KINDS = ["normal", "integer", "half_inf", "one_finite"]
GAP, ROWS, N_MAX = 5, 3, 16
NINF = float("-inf")


def _row(kind, V, g):
    if kind == "normal":
        return torch.randn(V, generator=g) * 8
    if kind == "integer":
        r = torch.randint(-3, 3, (V,), generator=g).float()                 # -3..2, then the 3s by hand
        for i in (5, 6, 70, 200, 261, 517, V - 1):
            if 0 <= i < V:
                r[i] = 3.0
        return r
    r = torch.randn(V, generator=g) * 8
    if kind == "half_inf":
        r[torch.randperm(V, generator=g)[:V // 2]] = NINF
        return r
    keep = int(torch.randint(0, V, (1,), generator=g))
    out = torch.full((V,), NINF)
    out[keep] = r[keep]
    return out


@functools.lru_cache(maxsize=None)
def _case(V, kind):
    """-> (the [ROWS, V + GAP] block, tokens [ROWS], the float64 reference at top_n = 16); computed once and left unchanged."""
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + V)
    buf = torch.full((ROWS, V + GAP), 1e30)
    for b in range(ROWS):
        buf[b, :V] = _row(kind, V, g)
    tok = torch.randint(0, V, (ROWS,), generator=g)
    return buf, tok, R.step_ref(buf[:, :V], tok, N_MAX)


def _outputs(B, n, cols=3):
    """Sentinel-filled outputs of ``cols`` columns."""
    return (torch.full((B, cols), 777.0, device="cuda"), torch.full((B, cols, max(n, 1)), 555.0, device="cuda")[:, :, :n].contiguous(),
            torch.full((B, cols, max(n, 1)), -7, dtype=torch.int64, device="cuda")[:, :, :n].contiguous())


def _run(x, tok, n, col=1, skip=None):
    lp, tl, ti = _outputs(x.shape[0], n)
    ops.step_logprobs(x, tok, out=lp, col=col, skip=skip, top_n=n, top_out=tl if n else None, top_ids=ti if n else None)
    return lp, tl, ti


def _untouched(lp, tl, ti, col):
    other = [c for c in range(lp.shape[1]) if c != col]
    return (bool((lp[:, other] == 777.0).all()) and bool((tl[:, other] == 555.0).all()) and bool((ti[:, other] == -7).all()))


def _close(got, ref):
    """|got - ref| where the reference is finite; -inf exactly where it is -inf."""
    got = got.cpu().double()
    fin = torch.isfinite(ref)
    assert torch.equal(got[~fin], ref[~fin]), (got[~fin], ref[~fin])
    return float((got[fin] - ref[fin]).abs().max()) if bool(fin.any()) else 0.0


@pytest.mark.parametrize("n", [0, 1, 5, 16])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_step_logprobs_against_float64_and_token_logprob(V, B, n):
    worst = 0.0
    for kind in KINDS:
        buf, tok, (ref_lp, ref_tl, ref_ti) = _case(V, kind)
        x, t = buf[:B].cuda()[:, :V], tok[:B].cuda()                         # [B, V] view of the [B, V + GAP] block
        lp, tl, ti = _run(x, t, n)
        assert _untouched(lp, tl, ti, 1), kind
        assert torch.equal(ti[:, 1].cpu(), ref_ti[:B, :n]), (kind, ti[:, 1].cpu(), ref_ti[:B, :n])       # the ids, exactly
        # bit-equality with kx_token_logprob on the same row and id
        assert torch.equal(lp[:, 1], ops.token_logprob(x, t)), kind
        if n:
            ids = ti[:, 1].reshape(B * n)
            rows = torch.arange(B, dtype=torch.int32, device="cuda").repeat_interleave(n)
            same = ops.token_logprob(x, ids.contiguous(), row_index=rows)                                # (id -1: 0.0 there)
            live = ids >= 0
            assert torch.equal(tl[:, 1].reshape(B * n)[live], same[live]), kind
            assert bool((tl[:, 1].reshape(B * n)[~live] == NINF).all()), kind
        worst = max(worst, _close(lp[:, 1], ref_lp[:B]), _close(tl[:, 1], ref_tl[:B, :n]))
        lp2, tl2, ti2 = _run(x, t, n)                                                                    # two calls, identical bits
        assert torch.equal(lp2, lp) and torch.equal(ti2, ti) and torch.equal(tl2.view(torch.int32), tl.view(torch.int32)), kind
    print(f"step_logprobs V={V} B={B} top_n={n}: worst |err| {worst:.3e} (bound {BOUND:.0e})")
    assert worst <= BOUND


@pytest.mark.parametrize("n", [0, 5, 16])
@pytest.mark.parametrize("V", [5, 257, 64007])
def test_skipped_rows_and_tokens_out_of_range(V, n):
    buf, tok, (ref_lp, ref_tl, ref_ti) = _case(V, "normal")
    x = buf.cuda()[:, :V]
    skip = torch.tensor([0, 1, 0], dtype=torch.uint8, device="cuda")
    bad = torch.tensor([V, int(tok[1]), -1], device="cuda")                  # rows 0 and 2 live, their tokens outside [0, V)
    for col in (0, 2):
        lp, tl, ti = _run(x, bad, n, col=col, skip=skip)
        assert _untouched(lp, tl, ti, col)
        assert lp[:, col].tolist() == [0.0, 0.0, 0.0]                        # a bad token: 0.0; a skipped row: 0.0
        assert bool((tl[1, col] == 0.0).all()) and bool((ti[1, col] == -1).all())                       # skipped: zeros and -1
        assert torch.equal(ti[[0, 2], col].cpu(), ref_ti[[0, 2], :n])        # the live rows' alternatives are written all the same
        assert _close(tl[[0, 2], col], ref_tl[[0, 2], :n]) <= BOUND
    # skip given and all zero: what skip=None gives
    a, b = _run(x, tok.cuda(), n, skip=torch.zeros(3, dtype=torch.uint8, device="cuda")), _run(x, tok.cuda(), n)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # every row skipped: nothing of the logits is read (the block is NaN)
    lp, tl, ti = _run(torch.full((3, V), float("nan"), device="cuda"), tok.cuda(), n, skip=torch.ones(3, dtype=torch.uint8, device="cuda"))
    assert bool((lp[:, 1] == 0.0).all()) and bool((tl[:, 1] == 0.0).all()) and bool((ti[:, 1] == -1).all()) and _untouched(lp, tl, ti, 1)


@pytest.mark.parametrize("V", [257, 64007])
def test_a_row_gives_the_same_bits_at_any_row_index_and_batch(V):
    buf, tok, _ = _case(V, "integer")
    one, t = buf[:1].cuda()[:, :V], tok[:1].cuda()
    lp1, tl1, ti1 = _run(one, t, 16)
    x = buf[[1, 0, 0, 2, 0]].cuda()[:, :V]
    lp, tl, ti = _run(x, tok[[1, 0, 0, 2, 0]].cuda(), 16)
    for b in (1, 2, 4):
        assert torch.equal(lp[b], lp1[0]) and torch.equal(tl[b], tl1[0]) and torch.equal(ti[b], ti1[0])
    assert torch.equal(_run(one, t, 5)[2][0, 1], ti1[0, 1, :5])              # the shorter lists are prefixes of the longer
    assert torch.equal(_run(one, t, 1)[2][0, 1], ti1[0, 1, :1])


def test_a_nan_in_the_row_gives_nan_logprobs_and_ids_in_range():
    V = 257
    x = _case(V, "normal")[0][:2].cuda()[:, :V].contiguous()
    x[0, 100] = float("nan")
    lp, tl, ti = _run(x, torch.tensor([3, 3], device="cuda"), 5)
    assert bool(torch.isnan(lp[0, 1])) and bool(torch.isnan(tl[0, 1]).all())
    assert bool(((ti[0, 1] >= -1) & (ti[0, 1] < V)).all())
    assert bool(torch.isfinite(lp[1, 1])) and bool(torch.isfinite(tl[1, 1]).all())                      # the other row is its own


def test_refusals_launch_nothing():
    lib = H.load()
    H.prof_enable(True)
    try:
        for name, rc, msg in step_logprobs_refusals(lib):
            assert rc == KX_ERR_INVALID_ARG and "kx_step_logprobs" in msg and name in msg, (name, rc, msg)
        x, t = torch.zeros(2, 10, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
        lp, tl, ti = _outputs(2, 5)
        for exc, kw in ((TypeError, dict(logits=x.double())), (TypeError, dict(token=t.int())), (TypeError, dict(out=lp[:, :2])),
                        (ValueError, dict(col=3)), (ValueError, dict(top_n=17)), (TypeError, dict(top_ids=ti.int())),
                        (TypeError, dict(top_out=None)), (TypeError, dict(skip=torch.zeros(2, dtype=torch.bool, device="cuda"))),
                        (RuntimeError, dict(token=t.cpu()))):
            a = dict(logits=x, token=t, out=lp, col=1, skip=None, top_n=5, top_out=tl, top_ids=ti)
            a.update(kw)
            with pytest.raises(exc):
                ops.step_logprobs(a.pop("logits"), a.pop("token"), **a)
        torch.cuda.synchronize()
        assert H.prof_collect() == []
    finally:
        H.prof_enable(False)
    assert _untouched(lp, tl, ti, 99)                                        # nothing was written anywhere
