"""kx_token_logprob (csrc/kx_rowops.hip): out[r] = x[target[r]] - logsumexp(x) over x = logits[row_index[r], 0:V], one launch, no
softmax written — against float64 (tests/score_ref.py).

The inputs are the cross-entropy kernel's (tests/test_train_kernels_gpu.py, CE_CASES: the two kernels share their device code): V in
{1, 255, 257, 1002, 64007}, logits near 1e4, and a row pitch of 1008 whose columns past V hold the row's maximum."""
import pytest
import torch

import score_ref as R
from kosmosx import ops
from test_train_kernels_gpu import CE_CASES, _ce_inputs

pytestmark = pytest.mark.gpu

BOUND = 2e-5            # absolute, over float64: the project's row-loss bound for this arithmetic (measured there at 7.6e-6 worst)
# measured here (MI355X), worst case over the table: 7.2e-6 (many_rows_low: log-probs near -100, where half an fp32 ulp is 3.8e-6),
# 3.3e-6 at vocab_64007_wide, below 1.1e-6 everywhere else


def _case(name):
    """logits [rows, ld], V, and 2 * rows + 3 outputs whose row_index repeats and permutes the rows."""
    buf, _ = _ce_inputs(name)
    rows, V = CE_CASES[name][:2]
    g = torch.Generator().manual_seed(rows + V)
    n = 2 * rows + 3
    idx = torch.cat([torch.randperm(rows, generator=g), torch.randint(0, rows, (n - rows,), generator=g)]).to(torch.int32)
    tgt = torch.randint(0, V, (n,), generator=g)
    tgt[0], tgt[1] = 0, V - 1
    return buf, V, idx, tgt


@pytest.mark.parametrize("name", list(CE_CASES))
def test_token_logprob_against_float64(name):
    buf, V, idx, tgt = _case(name)
    ref = R.token_logprob_ref(buf, tgt, idx, vocab=V)
    logits = buf.cuda()
    got = ops.token_logprob(logits, tgt.cuda(), row_index=idx.cuda(), vocab=V)
    assert got.dtype == torch.float32 and got.shape == tgt.shape and bool(torch.isfinite(got).all())
    e = float((got.cpu().double() - ref).abs().max())
    print(f"token_logprob {name}: worst |err| {e:.3e} (bound {BOUND:.0e})")
    assert e <= BOUND
    assert torch.equal(ops.token_logprob(logits, tgt.cuda(), row_index=idx.cuda(), vocab=V), got)        # two calls, identical bits
    # no row_index: row r; and the logits[:, :V] view the step hands over (a row pitch, unit column stride)
    rows = buf.shape[0]
    got2 = ops.token_logprob(logits[:, :V], tgt[:rows].cuda())
    e2 = float((got2.cpu().double() - R.token_logprob_ref(buf, tgt[:rows], vocab=V)).abs().max())
    assert e2 <= BOUND


def test_out_of_range_target_and_row_index_give_exactly_zero():
    buf, V, idx, tgt = _case("V_257")
    rows = buf.shape[0]
    tgt, idx = tgt.clone(), idx.clone()
    tgt[2], tgt[3], tgt[4] = V, -1, 1 << 40
    idx[5], idx[6] = rows, -1
    got = ops.token_logprob(buf.cuda(), tgt.cuda(), row_index=idx.cuda(), vocab=V).cpu()
    assert got[2:7].tolist() == [0.0] * 5
    ref = R.token_logprob_ref(buf, tgt, idx, vocab=V)
    assert float((got.double() - ref).abs().max()) <= BOUND and bool((got[7:] < 0).all())


def test_minus_infinity_and_nan():
    buf, V, idx, tgt = _case("V_255")
    buf = buf.clone()
    buf[0, 7] = float("-inf")
    buf[1, 200] = float("nan")
    idx = torch.tensor([0, 0, 1, 2], dtype=torch.int32)
    tgt = torch.tensor([7, 8, 3, 3])
    got = ops.token_logprob(buf.cuda(), tgt.cuda(), row_index=idx.cuda(), vocab=V).cpu()
    assert got[0].item() == float("-inf")                        # a -inf target logit
    assert abs(got[1].item() - R.token_logprob_ref(buf, tgt, idx, vocab=V)[1].item()) <= BOUND   # ... leaves the row's other entries alone
    assert got[2].item() != got[2].item()                        # a NaN in the row
    assert bool(torch.isfinite(got[3]))


def test_the_wrapper_checks_its_arguments():
    x = torch.zeros(4, 10, device="cuda")
    t = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError):
        ops.token_logprob(x.double(), t)
    with pytest.raises(TypeError):
        ops.token_logprob(x, t.int())
    with pytest.raises(ValueError):
        ops.token_logprob(x, t[:3].contiguous())
    with pytest.raises(TypeError):
        ops.token_logprob(x, t, row_index=torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="ld"):
        ops.token_logprob(x, t, vocab=11)
