"""kx_guidance_logits on the GPU, the kernel alone.

Bit-exact: lc and lu are taken on the device with ops.token_logprob (row_index = the row, target = 0..V-1); tests/guidance_ref.py's
guided_row_f32 over them must equal the kernel's output bit for bit.  Float64: elementwise
    |out - guided_row_f64| <= (|s| + |1 - s|) * 2e-5 + 2^-22 * (|lu| + |s * (lc - lu)|)
— the first term is the project's own bound for this log-prob arithmetic (tests/test_token_logprob_gpu.py) carried through the
combine out = (1 - s) * lu + s * lc, the second the three fp32 roundings.  A NumPy restatement of the arithmetic with the same
lane-strided summation stays below 0.26 of this bound on a CPU at every V below, at logit scales 1, 4 and 10 and all five s; the
device's worst ratio is printed.
Shapes: V at the 256-lane stride and at the edges of the 8 x 256 unrolled loop, one large value of each vocabulary kind; one and
three pairs; the three row pitches all different and > V on some cases; in place and out of place."""
import numpy as np
import pytest
import torch

import guidance_ref as GR
from kosmosx import ops

pytestmark = pytest.mark.gpu

VS = [1, 5, 255, 256, 257, 2047, 2048, 2049, 4097, 32002, 64007]
SCALES = [0.0, -0.5, 1.5, 3.0, 7.5]
SENTINEL = np.float32(12345.5)
WORST = {"ratio": 0.0}


def _buf(B, V, pad, seed=None):
    """fp32 [B, V + pad] on the host: randn * 4 in the row (or zeros), a sentinel nobody may touch behind it."""
    full = np.zeros((B, V + pad), dtype=np.float32)
    if seed is not None:
        full[:, :V] = (np.random.default_rng(seed).standard_normal((B, V)) * 4).astype(np.float32)
    full[:, V:] = SENTINEL
    return full


def _logprobs(view):
    """Device log-probs of every id of every row of the fp32 [B, V] view (any row pitch), as kx_token_logprob gives them."""
    B, V = view.shape
    dev = view.device
    tgt = torch.arange(V, dtype=torch.int64, device=dev).repeat(B)
    idx = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(V)
    return ops.token_logprob(view, tgt, row_index=idx).view(B, V).cpu().numpy()


def _same_bits(got, want):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad[0].size == 0, (bad[0][:5], bad[1][:5], got[bad][:5], want[bad][:5])


def _launch(c_host, u_host, V, s, *, o_host=None, finished=None, positions=None, advance=0):
    """One launch on device copies.  o_host None: in place.  Returns (cond buffer, uncond buffer, out buffer, positions) as numpy,
    whole buffers, padding included."""
    dev = torch.device("cuda")
    c, u = torch.from_numpy(c_host.copy()).to(dev), torch.from_numpy(u_host.copy()).to(dev)
    o = c if o_host is None else torch.from_numpy(o_host.copy()).to(dev)
    fin = None if finished is None else torch.tensor(finished, dtype=torch.uint8, device=dev)
    pos = None if positions is None else torch.tensor(positions, dtype=torch.int32, device=dev)
    ret = ops.guidance_logits(c[:, :V], u[:, :V], scale=s, out=None if o_host is None else o[:, :V], finished=fin, positions=pos,
                              advance=advance)
    torch.cuda.synchronize()
    assert ret.data_ptr() == o.data_ptr()
    return c.cpu().numpy(), u.cpu().numpy(), o.cpu().numpy(), (None if pos is None else pos.cpu().numpy())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_the_guided_rows_match_the_reference_bit_for_bit_and_the_float64_bound(B, V):
    dev = torch.device("cuda")
    pads = (3, 7, 5) if (V + B) % 2 else (0, 0, 0)                          # three different row pitches > V, or contiguous rows
    c_host, u_host = _buf(B, V, pads[0], seed=3 * V + B), _buf(B, V, pads[1], seed=5 * V + B + 1)
    lc = _logprobs(torch.from_numpy(c_host).to(dev)[:, :V])
    lu = _logprobs(torch.from_numpy(u_host).to(dev)[:, :V])
    lc64, lu64 = GR.log_softmax_f64(c_host[:, :V]), GR.log_softmax_f64(u_host[:, :V])
    for k, s in enumerate(SCALES):
        in_place = (k + V) % 2 == 0
        o_host = None if in_place else _buf(B, V, pads[2])
        c_after, u_after, o_after, _ = _launch(c_host, u_host, V, s, o_host=o_host)
        want = (c_host if in_place else o_host).copy()
        want[:, :V] = GR.guided_row_f32(lc, lu, s)
        _same_bits(o_after, want)                                           # the rows and the padding behind them
        _same_bits(u_after, u_host)                                         # the inputs are read only
        if not in_place:
            _same_bits(c_after, c_host)
        ref = GR.guided_row_f64(c_host[:, :V], u_host[:, :V], s)
        bound = (abs(s) + abs(1 - s)) * 2e-5 + 2.0 ** -22 * (np.abs(lu64) + np.abs(s * (lc64 - lu64)))
        ratio = float((np.abs(o_after[:, :V].astype(np.float64) - ref) / bound).max())
        WORST["ratio"] = max(WORST["ratio"], ratio)
        print(f"V={V} B={B} s={s}: worst |out - f64| / bound = {ratio:.3f} (so far {WORST['ratio']:.3f})")
        assert ratio <= 1.0, (V, B, s, ratio)


def _special_rows(V=300):
    c, u = _buf(3, V, 4, seed=21), _buf(3, V, 6, seed=22)
    c[0, [3, 50]] = -np.inf                                                 # cond only: 3; both: 50
    u[0, [7, 50]] = -np.inf                                                 # uncond only: 7
    c[1, 11] = np.nan                                                       # a NaN in the conditional row
    u[2, 13] = np.nan                                                       # ... and in the unconditional one
    return c, u, V


@pytest.mark.parametrize("s", [1.5, -0.5, 0.0])
def test_minus_inf_and_nan_inputs_give_minus_inf_there(s):
    c, u, V = _special_rows()
    dev = torch.device("cuda")
    lc, lu = _logprobs(torch.from_numpy(c).to(dev)[:, :V]), _logprobs(torch.from_numpy(u).to(dev)[:, :V])
    _, _, got, _ = _launch(c, u, V, s, o_host=_buf(3, V, 5))
    for b, i in ((0, 3), (0, 7), (0, 50), (1, 11), (2, 13)):
        assert got[b, i] == -np.inf, (b, i, got[b, i])
    want = _buf(3, V, 5)
    want[:, :V] = GR.guided_row_f32(lc, lu, s)                              # a reference over the same rows
    _same_bits(got, want)
    others = np.ones(V, bool)
    others[[3, 7, 50]] = False
    assert np.isfinite(got[0, :V][others]).all()                            # a -inf logit takes out its own id alone
    assert not np.isnan(got).any()


def test_a_finished_pair_is_untouched_and_every_position_advances():
    V = 2049
    c, u = _buf(3, V, 2, seed=31), _buf(3, V, 9, seed=32)
    u[1, :V] = np.nan                                                       # (a finished pair's inputs are not even read)
    dev = torch.device("cuda")
    lc, lu = _logprobs(torch.from_numpy(c).to(dev)[:, :V]), _logprobs(torch.from_numpy(u).to(dev)[:, :V])
    want = c.copy()
    want[[0, 2], :V] = GR.guided_row_f32(lc, lu, 3.0)[[0, 2]]
    for o_host in (None, _buf(3, V, 5)):
        _, u_after, got, pos = _launch(c, u, V, 3.0, o_host=o_host, finished=[0, 1, 0], positions=[10, 20, 2147483000], advance=1)
        if o_host is None:
            _same_bits(got, want)                                           # in place: row 1 keeps the conditional logits
        else:
            _same_bits(got[1], o_host[1])                                   # out of place: row 1 of out is not written
            _same_bits(got[[0, 2]], np.concatenate([want[[0, 2], :V], o_host[[0, 2], V:]], axis=1))
        assert pos.tolist() == [11, 21, 2147483001]                         # finished ones included
        assert np.array_equal(u_after.view(np.uint32), u.view(np.uint32))
    _, _, _, pos = _launch(c, u, V, 3.0, finished=[0, 1, 0], positions=[10, 20, 30], advance=0)
    assert pos.tolist() == [10, 20, 30]                                     # advance = 0: nothing moves
    _, _, got, pos = _launch(c, u, V, 3.0, finished=[0, 1, 0], positions=None, advance=1)
    assert pos is None
    _same_bits(got, want)                                                   # positions = NULL: the rows all the same


@pytest.mark.parametrize("V", [257, 64007])
def test_a_pair_does_not_depend_on_the_batch_or_on_its_index_and_two_calls_agree(V):
    c, u = _buf(3, V, 3, seed=41 + V), _buf(3, V, 0, seed=42 + V)
    _, _, all3, _ = _launch(c, u, V, 1.5, o_host=_buf(3, V, 1))
    _, _, again, _ = _launch(c, u, V, 1.5, o_host=_buf(3, V, 1))
    _same_bits(all3, again)
    for b in range(3):
        _, _, alone, _ = _launch(c[b:b + 1], u[b:b + 1], V, 1.5)
        _same_bits(alone[:, :V], all3[b:b + 1, :V])
    order = [2, 0, 1]
    _, _, moved, _ = _launch(c[order], u[order], V, 1.5)
    _same_bits(moved[:, :V], all3[order, :V])


@pytest.mark.parametrize("V", [5, 2049, 32002])
def test_equal_rows_give_the_log_softmax_exactly(V):
    dev = torch.device("cuda")
    c = _buf(2, V, 3, seed=51 + V)
    lc = _logprobs(torch.from_numpy(c).to(dev)[:, :V])
    for s in SCALES + [-1e30]:
        _, _, got, _ = _launch(c, c, V, s, o_host=_buf(2, V, 6))
        _same_bits(got[:, :V], lc)
    t = torch.from_numpy(c.copy()).to(dev)
    out = torch.empty((2, V), dtype=torch.float32, device=dev)
    ops.guidance_logits(t[:, :V], t[:, :V], scale=2.5, out=out)             # the very same tensor as both inputs
    _same_bits(out.cpu().numpy(), lc)


def test_the_wrapper_and_the_library_refuse_bad_tensors():
    dev = torch.device("cuda")
    c, u = torch.zeros((2, 10), device=dev), torch.zeros((2, 10), device=dev)
    with pytest.raises(RuntimeError, match="out overlaps uncond"):
        ops.guidance_logits(c, u, scale=1.5, out=u)
    with pytest.raises(RuntimeError, match="out overlaps uncond"):
        ops.guidance_logits(c, c, scale=1.5)                                # in place over a row that is also the unconditional one
    with pytest.raises(RuntimeError, match="scale"):
        ops.guidance_logits(c, u, scale=float("nan"))
    with pytest.raises(RuntimeError, match="advance"):
        ops.guidance_logits(c, u, scale=1.5, positions=torch.zeros(2, dtype=torch.int32, device=dev), advance=2)
    with pytest.raises(ValueError, match="uncond"):
        ops.guidance_logits(c, torch.zeros((2, 9), device=dev), scale=1.5)
    with pytest.raises(TypeError, match="positions"):
        ops.guidance_logits(c, u, scale=1.5, positions=torch.zeros(2, dtype=torch.int64, device=dev), advance=1)
    with pytest.raises(ValueError, match="finished"):
        ops.guidance_logits(c, u, scale=1.5, finished=torch.zeros(3, dtype=torch.uint8, device=dev))
    with pytest.raises(TypeError, match="cond"):
        ops.guidance_logits(c.double(), u, scale=1.5)
    assert not c.any() and not u.any()                                      # nothing was launched
