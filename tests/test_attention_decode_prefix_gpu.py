"""The PREFIX form of attn_decode_kernel (kx_attention_decode_prefix, csrc/kx_attention.hip): rows that read a shared, read-only
prefix cache first and a private tail cache after it.

The contract is bit equality with kx_attention_decode_ragged on a private cache assembled from the prefix and tail rows
(tests/prefix_ref.py::assemble): same slots, key order and arithmetic, only the address a key is loaded from differs.  On top of it the
float64 reference at the bound tests/test_attention_decode_gpu.py holds this arithmetic to, the caches (the prefix caches untouched,
one tail row written) and the guard.  tests/test_prefix_ref.py shows on the CPU that these inputs reject kernels that index the
tail wrongly, read the wrong prefix sequence, read key t from the tail or stop the prefix one key early.

Cases: P on both sides of the 128-key (fp32) and 256-key (bf16) first rounds and P = 0, tail fills 0 (the first step) to 40, five
rows over two prefix sequences ([1, 0, 1, 1, 0]); 2 heads of 64, Tmax = 320, Ttail = 48."""
import pytest
import torch

import decode_ref as DR
import prefix_ref as R
from kosmosx import _hip
from kosmosx import ops

pytestmark = pytest.mark.gpu

BOUND = 2e-5
# measured worst rel_err over CASES (MI355X): fp32 cache 1.94e-6 (P = 128, fill 0), bf16 cache 2.10e-6 (P = 257, fill 40) — a tenth
# of the bound and the level of the ragged kernel over its own positions (2.0e-6): it is the same arithmetic
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
ERR_CACHE = _hip.KX_RAGGED_ERR_CACHE


def _prefix(inp, words=None, **kw):
    """One prefix launch on device copies -> (out, kprefix, vprefix, ktail, vtail after, error word) on the CPU."""
    qkv, kp, vp, kt, vt, pos, seq, plen = inp
    if words is not None:
        pos, seq, plen = words
    dev = [x.cuda() for x in (kp, vp, kt, vt)]
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = ops.attention_decode_prefix(qkv.cuda(), *dev, pos.cuda(), seq.cuda(), plen.cuda(), err, **kw)
    torch.cuda.synchronize()
    return (out.cpu(), *(x.cpu() for x in dev), int(err.item()))


def _ragged(inp, **kw):
    """The ragged launch on the assembled private caches -> (out, kcache, vcache after, error word) on the CPU."""
    qkv, kp, vp, kt, vt, pos, seq, plen = inp
    kd, vd = R.assemble(kp, kt, pos, seq, plen).cuda(), R.assemble(vp, vt, pos, seq, plen).cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = ops.attention_decode(qkv.cuda(), kd, vd, positions=pos.cuda(), error_word=err, **kw)
    torch.cuda.synchronize()
    return out.cpu(), kd.cpu(), vd.cpu(), int(err.item())


def _same(a, b):
    return a.dtype == b.dtype and torch.equal(DR.bits(a) if a.is_floating_point() else a, DR.bits(b) if b.is_floating_point() else b)


def _check_bits(inp, **kw):
    """Prefix launch == ragged launch on the assembled cache: outputs, the appended row; the prefix caches and every other tail row
    untouched.  Returns the prefix launch's output."""
    qkv, kp, vp, kt, vt, pos, seq, plen = inp
    out, kp1, vp1, kt1, vt1, word = _prefix(inp, **kw)
    ref, kr, vr, word_r = _ragged(inp, **kw)
    assert word == 0 and word_r == 0
    assert _same(out, ref)
    assert _same(kp1, kp) and _same(vp1, vp)                                  # const: bitwise untouched
    for r in range(R.M):
        t, P = int(pos[r]), int(plen[r])
        assert _same(kt1[r, :, t - P], kr[r, :, t]) and _same(vt1[r, :, t - P], vr[r, :, t]), r      # the ragged launch's cache row t
        keep = torch.arange(kt.shape[2]) != t - P
        assert _same(kt1[r][:, keep], kt[r][:, keep]) and _same(vt1[r][:, keep], vt[r][:, keep]), r
    return out


@pytest.mark.parametrize("P", R.PREFIXES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_of_the_ragged_launch_and_float64(dtype, P):
    worst = (0.0, -1)
    for i, fill in enumerate(R.FILLS):
        inp = R.prefix_inputs(P, fill, dtype, seed=100 + R.CASES.index((P, fill)))
        st_p, st_r = (torch.zeros(R.M, R.HH, 2, device="cuda") for _ in range(2))
        out = _check_bits(inp)
        _prefix(inp, stats_out=st_p)
        _ragged(inp, stats_out=st_r)
        assert _same(st_p.cpu(), st_r.cpu())
        ref, kt_ref, vt_ref = R.prefix_attention_ref(*inp, nan_to_num=dtype == torch.float32)
        assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        _, _, _, kt1, vt1, _ = _prefix(inp)
        assert _same(kt1, kt_ref) and _same(vt1, vt_ref)                      # the reference's own statement of the append
        e = DR.rel_err64(out, ref)
        worst = max(worst, (e, fill))
        assert e < BOUND, (P, fill, e)
    print(f"prefix decode attention, {dtype} cache, P = {P}: worst rel_err {worst[0]:.3e} at fill {worst[1]} (bound {BOUND:.0e})")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rows_of_one_sequence_with_different_prefix_lengths(dtype):
    """Rows that name the same prefix sequence with different P and different fills, P = 0 among them."""
    inp = R.prefix_inputs([130, 256, 0, 129, 17], [3, 0, 40, 16, 47], dtype, seed=77)
    out = _check_bits(inp)
    ref, _, _ = R.prefix_attention_ref(*inp, nan_to_num=dtype == torch.float32)
    # (the prefix rows between a row's P and its sequence's largest P are finite here: what shows a read past P is the float64 value)
    assert DR.rel_err64(out, ref) < BOUND


@pytest.mark.parametrize("dtype,forms", [(torch.float32, ("f32", "f16c", "f16p")), (torch.bfloat16, ("f32", "bf16"))], ids=IDS)
def test_output_forms(dtype, forms):
    """KX_F32, KX_BF16, KX_F16C and KX_F16P: each the ragged launch's bits."""
    for P, fill in ((129, 17), (0, 5)):
        inp = R.prefix_inputs(P, fill, dtype, seed=300 + P)
        for form in forms:
            _check_bits(inp, out_dtype=form)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_major_layout_gives_the_bits_of_the_default_layout(dtype):
    """Tuning key 9 = 1 lays out both caches as [sequences, T, H, 64]: the default layout's output and statistics, the appended row
    at [r, t - P, h, :], nothing else moved."""
    lib = _hip.load()
    inp = R.prefix_inputs(257, 16, dtype, seed=400)
    qkv, kp, vp, kt, vt, pos, seq, plen = inp
    st0, st1 = (torch.zeros(R.M, R.HH, 2, device="cuda") for _ in range(2))
    out0, _, _, kt0, vt0, _ = _prefix(inp, stats_out=st0)
    rm = (qkv, *(x.transpose(1, 2).contiguous() for x in (kp, vp, kt, vt)), pos, seq, plen)
    lib.kx_set_tuning(9, 1)
    try:
        out1, kp1, vp1, kt1, vt1, word = _prefix(rm, stats_out=st1, layout="row_major")
    finally:
        lib.kx_set_tuning(9, 0)
    assert word == 0 and _same(out1, out0) and _same(st1.cpu(), st0.cpu())
    assert _same(kp1, rm[1]) and _same(vp1, rm[2])
    assert _same(kt1, kt0.transpose(1, 2).contiguous()) and _same(vt1, vt0.transpose(1, 2).contiguous())
    with pytest.raises(ValueError):
        _prefix(inp, layout="row_major")                                       # [Bp, H, Tmax, 64] is not [Bp, Tmax, H, 64]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_guard_rejects_a_row_and_leaves_the_others(dtype):
    """prefix_seq = Bp, t < P, t - P = Ttail, P > Tmax and a negative word: the kernel's own check rejects the row before any
    address is formed from the word — it writes no output, no statistics and no tail row and sets KX_RAGGED_ERR_CACHE; the other
    rows keep the bits of the clean launch."""
    inp = R.prefix_inputs(129, 17, dtype, seed=500)
    qkv, kp, vp, kt, vt, pos, seq, plen = inp
    st0 = torch.full((R.M, R.HH, 2), -7.0, device="cuda")
    clean, _, _, kt0, vt0, word = _prefix(inp, stats_out=st0)
    assert word == 0
    for row, (t, c, P) in ((0, (146, R.BP, 129)), (1, (128, 0, 129)), (2, (129 + R.TTAIL, 1, 129)), (3, (R.TMAX + 5, 1, R.TMAX + 1)),
                           (4, (146, -1, 129)), (1, (-1, 0, -1)), (3, (1 << 30, 1, -(1 << 30)))):
        words = [w.clone() for w in (pos, seq, plen)]
        words[0][row], words[1][row], words[2][row] = t, c, P
        st1 = torch.full((R.M, R.HH, 2), -7.0, device="cuda")
        out, kp1, vp1, kt1, vt1, word = _prefix(inp, words=words, stats_out=st1)
        assert word == ERR_CACHE, (row, t, c, P)
        others = [r for r in range(R.M) if r != row]
        assert bool((out[row] == 0).all()) and bool((st1[row] == -7.0).all())                    # (the wrapper's rows start as zeros)
        assert _same(kt1[row], kt[row]) and _same(vt1[row], vt[row])                             # no tail row
        assert _same(out[others], clean[others]) and _same(st1.cpu()[others], st0.cpu()[others])
        assert _same(kt1[others], kt0[others]) and _same(vt1[others], vt0[others])
        assert _same(kp1, kp) and _same(vp1, vp)


def test_the_wrapper_checks_shapes_and_dtypes():
    qkv, kp, vp, kt, vt, pos, seq, plen = (x.cuda() for x in R.prefix_inputs(5, 3, torch.float32, seed=1))
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError, match="prefix_seq"):
        ops.attention_decode_prefix(qkv, kp, vp, kt, vt, pos, seq.long(), plen, err)
    with pytest.raises(TypeError, match="prefix_len"):
        ops.attention_decode_prefix(qkv, kp, vp, kt, vt, pos, seq, plen[:3].contiguous(), err)
    with pytest.raises(TypeError, match="dtype"):
        ops.attention_decode_prefix(qkv, kp.bfloat16(), vp.bfloat16(), kt, vt, pos, seq, plen, err)
    with pytest.raises(ValueError, match="prefix caches"):
        ops.attention_decode_prefix(qkv, kp[:, :1].contiguous(), vp[:, :1].contiguous(), kt, vt, pos, seq, plen, err)
