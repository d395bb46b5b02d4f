"""Per-row presence / frequency penalties (kx_shape_logits_rows) on the GPU, bit for bit: against one-row kx_shape_logits launches
with the row's scalars, and against tests/shape_ref.py evaluated row by row.  uint32 compare of the logits, equality of the counts."""
import numpy as np
import pytest
import torch

import shape_ref as SR
from kosmosx import ops

pytestmark = pytest.mark.gpu

B = 4
FREQ = [0.0, 0.37, -0.25, 1.5]                                # row 0: no penalty at all; row 2: a negative one
PRES = [0.0, 0.0, 0.6, -0.125]
STEPS = 3


def _case(V):
    g = np.random.default_rng(V)
    logits = [(g.standard_normal((B, V)) * 3).astype(np.float32) for _ in range(STEPS)]
    for x in logits:
        x[g.random((B, V)) < 0.05] = -np.inf
        x[0, V // 2] = np.nan
    # the tokens "emitted": the slice edges and a repeat, so that counts above 1 and both slices of V = 4099 are met
    toks = np.array([[V - 1, V - 1, 0], [V // 2, V // 2, 3], [5, 5, V - 1], [min(4095, V - 2), min(4096, V - 1), 0]], dtype=np.int64)
    bias = [[(1, 0.5), (V - 1, -2.0)], [], [(0, float("-inf"))], [(V // 2, 1.25)]]
    return logits, toks, bias


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("with_bias", [False, True], ids=["penalties", "penalties+bias"])
@pytest.mark.parametrize("V", [37, 4099])
def test_every_row_equals_its_own_scalar_launch_and_the_reference(V, with_bias):
    dev = "cuda"
    logits, toks, bias = _case(V)
    table = ops.BiasTable(bias, dev) if with_bias else None
    f_rows, p_rows = torch.tensor(FREQ, device=dev), torch.tensor(PRES, device=dev)
    counts = torch.zeros((B, V), dtype=torch.int32, device=dev)
    alone = [torch.zeros((1, V), dtype=torch.int32, device=dev) for _ in range(B)]
    ref_counts = np.zeros((B, V), dtype=np.int32)
    finished = torch.tensor([0, 0, 0, 0], dtype=torch.uint8, device=dev)
    for g in range(STEPS):
        last = torch.tensor(toks[:, g - 1], device=dev) if g else None
        if g == 2:
            finished[1] = 1                                   # a finished row keeps its logits and its counts
        rows = torch.tensor(logits[g], device=dev)
        ops.shape_logits(rows, bias=table, counts=counts, last_token=last, finished=finished, frequency_rows=f_rows, presence_rows=p_rows)
        for b in range(B):
            one = torch.tensor(logits[g][b:b + 1], device=dev)
            ops.shape_logits(one, bias=ops.BiasTable(bias[b:b + 1], dev) if with_bias else None, counts=alone[b],
                             last_token=None if last is None else last[b:b + 1].contiguous(), finished=finished[b:b + 1].contiguous(),
                             frequency_penalty=FREQ[b], presence_penalty=PRES[b])
            assert np.array_equal(_bits(rows[b]), _bits(one[0])), (g, b)
            assert torch.equal(counts[b], alone[b][0]), (g, b)
            want, ref_counts[b] = SR.shape_row(logits[g][b], ref_counts[b], bias=bias[b] if with_bias else (), frequency=FREQ[b],
                                               presence=PRES[b], last_token=None if g == 0 else int(toks[b, g - 1]),
                                               finished=bool(finished[b]))
            assert np.array_equal(_bits(rows[b]), want.view(np.uint32)), (g, b)
            assert np.array_equal(counts[b].cpu().numpy(), ref_counts[b]), (g, b)
    assert counts.max() == 2 and counts[1].sum() == 1         # a repeat was counted twice; the finished row stopped counting
    assert not np.array_equal(_bits(rows[3]), logits[STEPS - 1][3].view(np.uint32))               # the penalties are real


def test_one_array_alone_takes_the_scalar_for_the_other():
    V, dev = 4099, "cuda"
    logits, toks, _ = _case(V)
    last = torch.tensor(toks[:, 0], device=dev)
    f_rows, p_rows = torch.tensor(FREQ, device=dev), torch.tensor(PRES, device=dev)
    for kw, f, p in ((dict(frequency_rows=f_rows, presence_penalty=0.3), FREQ, [0.3] * B),
                     (dict(presence_rows=p_rows, frequency_penalty=-0.7), [-0.7] * B, PRES)):
        rows, counts = torch.tensor(logits[0], device=dev), torch.zeros((B, V), dtype=torch.int32, device=dev)
        ops.shape_logits(rows, counts=counts, last_token=last, **kw)
        for b in range(B):
            want, c = SR.shape_row(logits[0][b], np.zeros(V, dtype=np.int32), frequency=f[b], presence=p[b], last_token=int(toks[b, 0]))
            assert np.array_equal(_bits(rows[b]), want.view(np.uint32)) and np.array_equal(counts[b].cpu().numpy(), c), (sorted(kw), b)


def test_without_the_arrays_the_old_entry_point_is_called_and_the_arrays_are_checked(monkeypatch):
    V, dev = 37, "cuda"
    logits, toks, _ = _case(V)
    real, names = ops.H.load(), []

    class Spy:
        def __getattr__(self, name):
            names.append(name)
            return getattr(real, name)
    monkeypatch.setattr(ops.H, "load", lambda: Spy())
    rows, counts = torch.tensor(logits[0], device=dev), torch.zeros((B, V), dtype=torch.int32, device=dev)
    ops.shape_logits(rows, counts=counts, frequency_penalty=0.5, frequency_rows=None, presence_rows=None)
    assert names == ["kx_shape_logits"]
    ops.shape_logits(rows, counts=counts, frequency_rows=torch.tensor(FREQ, device=dev))
    assert names == ["kx_shape_logits", "kx_shape_logits_rows"]
    # both arrays NULL at the C level is the old launch too
    a, b = torch.tensor(logits[1], device=dev), torch.tensor(logits[1], device=dev)
    ca, cb = counts.clone(), counts.clone()
    last = torch.tensor(toks[:, 0], device=dev)
    args = ops.H.ShapeArgs()
    for t, c, fn in ((a, ca, real.kx_shape_logits), (b, cb, None)):
        args.logits, args.ld, args.B, args.V, args.counts = t.data_ptr(), V, B, V, c.data_ptr()
        args.frequency, args.presence, args.last_token = 0.25, -0.5, last.data_ptr()
        import ctypes as C
        rc = fn(C.byref(args), None) if fn else real.kx_shape_logits_rows(C.byref(args), None, None, None)
        assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a), _bits(b)) and torch.equal(ca, cb)
    with pytest.raises(RuntimeError, match="counts"):
        ops.shape_logits(rows, bias=ops.BiasTable([[(0, 1.0)]] * B, dev), frequency_rows=torch.tensor(FREQ, device=dev))
    with pytest.raises(ValueError, match="frequency_rows"):
        ops.shape_logits(rows, counts=counts, frequency_rows=torch.tensor(FREQ[:2], device=dev))
    with pytest.raises(TypeError, match="presence_rows"):
        ops.shape_logits(rows, counts=counts, presence_rows=torch.tensor(PRES, device=dev, dtype=torch.float64))
