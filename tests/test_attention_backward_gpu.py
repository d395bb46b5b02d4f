"""The attention backward kernels (kx_attention_backward, kx_attention_backward_dropout, kx_attention_backward_dropout_bf16,
csrc/kx_backward.hip) against the float64 reference of tests/attention_bwd_ref.py.

tests/test_attention_bwd_ref.py shows on the CPU that these inputs and bounds accept a right kernel and reject kernels that drop
or double a row of a tile, start or end the causal walk a tile off, leave a wave's rows unwritten, mix up heads, batch rows, tile
buffers or mask bits; the bounds and their derivation are in the docstring of attention_bwd_ref.py.  Every comparison below goes
through attention_bwd_ref's dq_ratio / dk_ratio / dv_ratio and verdict, the code the CPU file runs its mutants through.

Every launch goes through ctypes on the library itself (the wrapper cannot express strides), is handed out = fp32(O) and
lse = fp32(lse) of the REFERENCE (so a failure is the backward's own), masks drawn on the CPU (train_ref.keep_mask, not
kx_dropout_mask), NaN-filled gradients and a NaN guard behind delta.

The entry points' dispatch and the configurations (attention_bwd_ref.CONFIGS) that launch each branch, causal and unmasked:
  kx_attention_backward, KX_PREC_F32            attn_bwd_dkv_mfma_kernel + attn_bwd_dq_mfma_kernel        fp32
  kx_attention_backward, KX_PREC_F32, key 2 = 1  attn_bwd_kernel<0>, <1>                                   fp32-valu
  kx_attention_backward, KX_PREC_BF16           attn_bwd_dkv_bf16_kernel + attn_bwd_dq_bf16_kernel<float> bf16p/f32
                                                ... <bf16_t>                                              bf16p/bf16
  kx_attention_backward_dropout                 attn_bwd_kernel<0>, <1> with the mask                      valu-drop
  kx_attention_backward_dropout_bf16            attn_bwd_*_bf16_kernel<float, DROP> / <bf16_t, DROP>       bf16-drop/f32, bf16-drop/bf16
  attn_delta_kernel                             every launch
B = 2, H = 3 unless stated: an odd head count and a second batch row, different inputs for every (b, h)."""
import pytest
import torch

import attention_bwd_ref as BR
from kosmosx import _hip

pytestmark = pytest.mark.gpu

MASKS = [True, False]
MASK_IDS = ["causal", "unmasked"]
GUARD = 64                                                # poisoned floats behind delta


def _poison(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _raw(entry, q, k, v, out, dout, lse, dq, dk, dv, delta, causal, *, prec=None, p=0.0, seed=BR.SEED, site=BR.SITE,
         row_stride=None, dq_ptr=None):
    """One call of an entry point on DEVICE views q / k / v / dq / dk / dv [B, T, H, 64] (any batch and row strides, the same for
    all six) and out / dout [B, T, H*64] -> the status.  prec, row_stride and dq_ptr override what the views imply."""
    lib = _hip.load()
    Bc, T, Hc, _ = q.shape
    for x in (k, v, dq, dk, dv):
        assert x.stride() == q.stride() and x.shape == q.shape
    assert q.stride(2) == 64 and q.stride(3) == 1 and out.stride() == dout.stride() and out.stride(2) == 1
    assert q.dtype == k.dtype == v.dtype and q.dtype in (torch.float32, torch.bfloat16)
    assert all(x.dtype == torch.float32 for x in (dq, dk, dv, out, dout, lse, delta))
    qkv_dt = _hip.KX_BF16 if q.dtype == torch.bfloat16 else _hip.KX_F32
    strides = (Bc, Hc, T, q.stride(1) if row_stride is None else row_stride, q.stride(0), out.stride(1), out.stride(0))
    mask = _hip.KX_ATTN_CAUSAL if causal else _hip.KX_ATTN_FULL
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = (out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dq.data_ptr() if dq_ptr is None else dq_ptr, dk.data_ptr(),
            dv.data_ptr(), delta.data_ptr())
    if entry == "plain":
        rc = lib.kx_attention_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), qkv_dt, *ptrs, *strides, mask, prec, stream)
    elif entry == "valu-drop":
        assert qkv_dt == _hip.KX_F32
        rc = lib.kx_attention_backward_dropout(q.data_ptr(), k.data_ptr(), v.data_ptr(), *ptrs, *strides, mask, float(p), seed,
                                               site, stream)
    else:
        rc = lib.kx_attention_backward_dropout_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), qkv_dt, *ptrs, *strides, mask,
                                                    float(p), seed, site, stream)
    torch.cuda.synchronize()
    return rc


def _launch(name, q, k, v, dO, R, causal, p=0.0, entry=None, key2=None):
    """One dense launch of configuration `name` on CPU tensors [B, T, H, 64] and the reference's out and lse -> (dq, dk, dv) on the
    CPU.  Checks on the way: the status, delta against the reference, the guard behind delta.  `entry` / `key2` launch the same
    data through another entry point or kernel variant."""
    cfg = BR.CONFIGS[name]
    entry = cfg.entry if entry is None else entry
    Bc, T, Hc, _ = q.shape
    qd, kd, vd = (x.to(cfg.store).cuda().contiguous() for x in (q, k, v))
    dout = dO.float().reshape(Bc, T, Hc * 64).cuda().contiguous()
    out, lse = R.out.float().cuda().contiguous(), R.lse.float().cuda().contiguous()
    dq, dk, dv = _poison(Bc, T, Hc, 64), _poison(Bc, T, Hc, 64), _poison(Bc, T, Hc, 64)
    delta = _poison(Bc * Hc * T + GUARD)
    lib = _hip.load()
    lib.kx_set_tuning(2, cfg.key2 if key2 is None else key2)
    try:
        prec = _hip.KX_PREC_F32 if cfg.fmt is None else _hip.KX_PREC_BF16
        rc = _raw(entry, qd, kd, vd, out, dout, lse, dq, dk, dv, delta, causal, prec=prec, p=p)
    finally:
        lib.kx_set_tuning(2, 0)
    assert rc == 0, (name, _hip.last_error())
    dl = delta.cpu()
    assert bool(torch.isnan(dl[Bc * Hc * T:]).all()), "delta: written past B H T"
    terms = (dO.double() * R.out.reshape(Bc, T, Hc, 64)).permute(0, 2, 1, 3)                            # [B, H, T, 64]
    tol = 66 * 2.0 ** -24 * terms.abs().sum(-1) + 1e-30                  # the fp32 O, 64 products, a sum of them in any order
    want = terms.sum(-1)
    assert bool(((dl[:Bc * Hc * T].double().reshape(Bc, Hc, T) - want).abs() <= tol).all()), "delta"
    return dq.cpu(), dk.cpu(), dv.cpu()


def _label(test, name, causal):
    return f"{test}, {name}, {'causal' if causal else 'unmasked'}"


@pytest.mark.parametrize("causal", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("name", list(BR.CONFIGS))
def test_pair_probe(name, causal):
    """Probes A and B of attention_bwd_ref.probe_inputs on every shape of the configuration, dropout included: every score 0,
    P = 1 / n_i, each (query, key) pair and each keep bit alone in an element of dV and of dQ (A) or dK (B) — one pair more or
    less, or one wrong bit, is more than two bounds (tests/test_attention_bwd_ref.py).  dq, dk and dv are inside their bounds; dK
    of probe A and dQ of probe B are exactly zero (their bound is zero).
    Measured on an MI355X: worst error / bound, causal | unmasked: fp32 and fp32-valu 0.046 (A, T = 321, dq) | 0.022;
    valu-drop 0.063 | 0.063 (T = 1); bf16p/f32 and bf16p/bf16 0.496 (A, T = 193, dq) | 0.497 (A, T = 128, dq); bf16-drop/f32 and
    bf16-drop/bf16 0.495 (A, T = 131, dq) | 0.492 (A, T = 257, dq) — where the float64 restatement sits, to the digit: one bf16 rounding
    of a single term; the zero blocks are zero on every shape."""
    got = []
    for Bc, Hc, T, p in BR.shapes(name):
        for kind in ("A", "B"):
            q, k, v, dO, R = BR.case(kind, Bc, Hc, T, BR.CONFIGS[name].values, causal, p)
            dq, dk, dv = _launch(name, q, k, v, dO, R, causal, p)
            zero = dk if kind == "A" else dq
            assert float(zero.abs().max()) == 0.0, (kind, T, p)
            got += BR.grad_ratios(name, dq, dk, dv, R, (kind, T, p))
    BR.verdict(got, _label("pair probe", name, causal))


@pytest.mark.parametrize("causal", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("name", list(BR.CONFIGS))
def test_parity(name, causal):
    """Random inputs (q = randn * 0.35, k, v, dO = randn; bf16-exact for the configurations with bf16 products) on every shape and
    on (B, H, T) = (1, 9, 257) (the bf16 grids are head-fastest and tuned for H % 8 == 0): dq, dk, dv inside the elementwise bounds.
    Measured on an MI355X: worst error / bound, causal | unmasked: fp32 0.32 (T = 79, dv) | 0.34 (T = 191, dq); fp32-valu
    0.34 (T = 513, dq) | 0.39 (T = 130, dk); valu-drop 0.36 (T = 257, dv) | 0.35 (T = 131, dv); bf16p/f32 and bf16p/bf16 0.47 (T = 63,
    dk) | 0.44 (T = 130, dq); bf16-drop/f32 and bf16-drop/bf16 0.46 ((1, 9, 257), dv) | 0.47 (T = 63, dq)."""
    got = []
    for Bc, Hc, T, p in BR.shapes(name) + [BR.wide_shape(name)]:
        q, k, v, dO, R = BR.case("random", Bc, Hc, T, BR.CONFIGS[name].values, causal, p)
        got += BR.grad_ratios(name, *_launch(name, q, k, v, dO, R, causal, p), R, (Bc, Hc, T, p))
    BR.verdict(got, _label("parity", name, causal))


@pytest.mark.parametrize("name", BR.PLAIN)
def test_spikes(name):
    """A key k = c q[query] holding about half of its query's softmax weight, random dO: P is neither flat nor one-hot and |lse| a
    few units.  Causal T = 193: (query, key) = (192, 0) and (192, 191) — the one query of the last tile against the first tile and
    its own diagonal; (130, 64) and (70, 64) — a key at a tile start, two tiles and no tile before its query; unmasked T = 129:
    (128, 128), the diagonal pair of a last tile of one row.
    Measured on an MI355X: worst error / bound fp32 0.29 at (192, 0), fp32-valu 0.34, bf16p/f32 and bf16p/bf16 0.49, all three at
    (192, 191), all in dv."""
    got = []
    for i, (T, causal, query, key) in enumerate(BR.SPIKES):
        q, k, v, dO, R, w = BR.spike_case(BR.CONFIGS[name].values, i)
        assert all(0.3 <= x <= 0.7 for x in w), (i, w)
        got += BR.grad_ratios(name, *_launch(name, q, k, v, dO, R, causal), R, (T, query, key))
    BR.verdict(got, f"spikes, {name}")


def _unrounded(T, causal, p):
    """fp32 q, k, v that are NOT bf16-exact, a bf16-exact dO (delta is summed from the fp32 dO: a rounding of dO inside the passes
    alone is no part of the reference), and the reference of the bf16-rounded values (what the kernel is to multiply)."""
    q, k, v, dO = BR.random_inputs(BR.B, BR.H, T, torch.float32, seed=4000 + T)
    assert not torch.equal(q.to(torch.bfloat16).float(), q)
    dO = dO.to(torch.bfloat16).float()
    return q, k, v, dO, BR.Reference(q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16), dO, causal,
                                     BR.keep_scale(BR.B, BR.H, T, p))


@pytest.mark.parametrize("causal", MASKS, ids=MASK_IDS)
def test_rounding_on_the_way_in(causal):
    """KX_PREC_BF16 on fp32 q / k / v that are not bf16-exact against the same launch on q.to(bfloat16) rows as stored: dq, dk and
    dv bit-identical (the fp32 rows are rounded to nearest even on the way in, nothing else differs), for the plain and the
    dropout entry point; and inside the bounds of the reference on the rounded values.
    Measured on an MI355X: bit-identical; worst error / bound 0.45 causal (T = 130, p = 0.25, dq), 0.42 unmasked (T = 65, p = 0.25, dq)."""
    got = []
    for T in (65, 130):
        for f32name, b16name, p in (("bf16p/f32", "bf16p/bf16", 0.0), ("bf16-drop/f32", "bf16-drop/bf16", BR.P_DROP)):
            q, k, v, dO, R = _unrounded(T, causal, p)
            a = _launch(f32name, q, k, v, dO, R, causal, p)
            b = _launch(b16name, q, k, v, dO, R, causal, p)           # (_launch stores q / k / v in the configuration's dtype)
            for x, y, what in zip(a, b, ("dq", "dk", "dv")):
                assert torch.equal(BR.bits(x), BR.bits(y)), (T, f32name, what)
            got += BR.grad_ratios(f32name, *a, R, (T, p))
    BR.verdict(got, _label("rounding on the way in", "bf16", causal))


@pytest.mark.parametrize("causal", MASKS, ids=MASK_IDS)
def test_dropout_p0_is_the_plain_launch(causal):
    """Both dropout entry points at p = 0 against the plain launches that run the same kernels (tuning key 2 = 1 for the VALU one,
    KX_PREC_BF16 for the other, either storage dtype): bit-identical dq, dk, dv.
    Measured on an MI355X: bit-identical on all shapes."""
    for T in (5, 65, 130, 257):
        for drop, plain, key2 in (("valu-drop", "fp32-valu", 1), ("bf16-drop/f32", "bf16p/f32", 0), ("bf16-drop/bf16", "bf16p/bf16", 0)):
            q, k, v, dO, R = BR.case("random", BR.B, BR.H, T, BR.CONFIGS[drop].values, causal)
            a = _launch(drop, q, k, v, dO, R, causal, 0.0)
            b = _launch(plain, q, k, v, dO, R, causal)
            for x, y, what in zip(a, b, ("dq", "dk", "dv")):
                assert torch.equal(BR.bits(x), BR.bits(y)), (T, drop, what)


@pytest.mark.parametrize("causal", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("name", list(BR.CONFIGS))
def test_each_head_alone(name, causal):
    """(B, H, T) = (1, 9, 257): every head's dq, dk and dv equal, bit for bit, a B = H = 1 launch on that head's slices (the
    dropout entry points at p = 0, where no mask index depends on H).
    Measured on an MI355X: bit-identical for all nine heads."""
    Bc, Hc, T, _ = BR.wide_shape(name)
    q, k, v, dO, R = BR.case("random", Bc, Hc, T, BR.CONFIGS[name].values, causal)
    whole = _launch(name, q, k, v, dO, R, causal, 0.0)
    for h in range(Hc):
        one = lambda x: x[:, :, h:h + 1].contiguous()                                  # noqa: E731
        Rh = BR.Reference(one(q), one(k), one(v), one(dO), causal)
        part = _launch(name, one(q), one(k), one(v), one(dO), Rh, causal, 0.0)
        assert torch.equal(BR.bits(Rh.out.float()), BR.bits(R.out.reshape(Bc, T, Hc, 64)[:, :, h].float()))    # the same out handed in
        assert torch.equal(BR.bits(Rh.lse.float()), BR.bits(R.lse[:, h:h + 1].float()))
        for x, y, what in zip(whole, part, ("dq", "dk", "dv")):
            assert torch.equal(BR.bits(x[:, :, h:h + 1]), BR.bits(y)), (h, what)


@pytest.mark.parametrize("name", list(BR.CONFIGS))
def test_same_launch_twice(name):
    """No pass uses atomics and every mask is a function of (seed, site, index): a launch run twice is bit-identical.
    Measured on an MI355X: bit-identical."""
    for T, causal in ((130, True), (65, False)):
        p = 0.0 if BR.CONFIGS[name].entry == "plain" else BR.P_DROP
        q, k, v, dO, R = BR.case("random", BR.B, BR.H, T, BR.CONFIGS[name].values, causal, p)
        a, b = _launch(name, q, k, v, dO, R, causal, p), _launch(name, q, k, v, dO, R, causal, p)
        for x, y in zip(a, b):
            assert torch.equal(BR.bits(x), BR.bits(y)), (T, name)


@pytest.mark.parametrize("name", ["fp32", "bf16p/bf16", "bf16-drop/f32"])
def test_strided_rows_and_untouched_neighbours(name):
    """Nothing dense.  q, k, v = columns 0 .. D, D + 32 .. 2D + 32 and 2D + 64 .. 3D + 64 of a NaN-filled fused [B, T, 3D + 64] buffer
    whose batch stride is padded by 128 elements; dq, dk, dv the same columns of an fp32 NaN buffer with the same element strides;
    out and dout rows 2 .. 2 + T, columns 32 .. 32 + D of NaN-filled [B, T + 3, D + 64] buffers (row stride D + 64); a NaN guard behind
    delta.  A read outside the slices shows as NaN in a gradient; the gradients are inside their bounds, and every element of the
    gradient buffer outside the written columns, and the guard, keep their bits.  Causal T = 130 and unmasked T = 65.
    Measured on an MI355X: worst error / bound fp32 0.23 (T = 130, dv), bf16p/bf16 0.45 (T = 130, dq), bf16-drop/f32 0.44 (T = 65,
    dv); no element outside the slices changed."""
    cfg = BR.CONFIGS[name]
    Bc, Hc = BR.B, BR.H
    D = Hc * 64
    got = []
    for T, causal in ((130, True), (65, False)):
        p = 0.0 if cfg.entry == "plain" else BR.P_DROP
        q, k, v, dO, R = BR.case("random", Bc, Hc, T, cfg.values, causal, p)
        row, batch = 3 * D + 64, T * (3 * D + 64) + 128
        cols = [(0, D), (D + 32, 2 * D + 32), (2 * D + 64, 3 * D + 64)]

        def fused(dtype):
            flat = torch.full((Bc * batch,), float("nan"), dtype=dtype, device="cuda")
            buf = flat.as_strided((Bc, T, row), (batch, row, 1))
            return flat, [buf[:, :, a:b].unflatten(2, (Hc, 64)) for a, b in cols]

        _, (qv, kv, vv) = fused(cfg.store)
        for dst, src in ((qv, q), (kv, k), (vv, v)):
            dst.copy_(src.to(cfg.store).cuda())
        gflat, (dqv, dkv, dvv) = fused(torch.float32)
        obuf, dobuf = _poison(Bc, T + 3, D + 64), _poison(Bc, T + 3, D + 64)
        ov, dov = obuf[:, 2:2 + T, 32:32 + D], dobuf[:, 2:2 + T, 32:32 + D]
        ov.copy_(R.out.float().cuda()), dov.copy_(dO.float().reshape(Bc, T, D).cuda())
        lse, delta = R.lse.float().cuda().contiguous(), _poison(Bc * Hc * T + GUARD)
        before = BR.bits(gflat.cpu()).clone()
        prec = _hip.KX_PREC_F32 if cfg.fmt is None else _hip.KX_PREC_BF16
        assert _raw(cfg.entry, qv, kv, vv, ov, dov, lse, dqv, dkv, dvv, delta, causal, prec=prec, p=p) == 0, _hip.last_error()
        got += BR.grad_ratios(name, dqv.cpu(), dkv.cpu(), dvv.cpu(), R, (T, causal))
        assert bool(torch.isnan(delta.cpu()[Bc * Hc * T:]).all()) and bool(torch.isfinite(delta.cpu()[:Bc * Hc * T]).all())
        after = BR.bits(gflat.cpu()).clone()
        for x in (before, after):                                # blank the written slices, compare everything else
            view = x.as_strided((Bc, T, row), (batch, row, 1))
            for a, b in cols:
                view[:, :, a:b] = 0
        assert torch.equal(before, after), (T, name)
    BR.verdict(got, f"strided rows, {name}")


def test_refusals_launch_nothing():
    """Every refused call returns the documented error and leaves dq, dk, dv AND delta poisoned (no kernel ran, the delta kernel
    included): bf16 q / k / v with KX_PREC_F32; an unknown prec; a row stride that is no multiple of 4; a misaligned dq; p = 1 on both
    dropout entry points.
    Measured on an MI355X: all eleven calls refused with their message, the four buffers still poisoned.  (Before the precision
    check of kx_attention_backward moved above its first launch, the unknown-prec call had already written delta.)"""
    T, causal = 65, True
    q, k, v, dO, R = BR.case("random", BR.B, BR.H, T, torch.bfloat16, causal)
    Bc, Hc = BR.B, BR.H
    out, lse = R.out.float().cuda().contiguous(), R.lse.float().cuda().contiguous()
    dout = dO.float().reshape(Bc, T, Hc * 64).cuda().contiguous()
    f32s, b16s = [x.float().cuda().contiguous() for x in (q, k, v)], [x.cuda().contiguous() for x in (q, k, v)]
    F32, BF16 = _hip.KX_PREC_F32, _hip.KX_PREC_BF16
    cases = [("plain", b16s, dict(prec=F32), "bf16 with bf16 products"),
             ("plain", f32s, dict(prec=9), "products in fp32 or bf16"),
             ("plain", b16s, dict(prec=9), "bf16 with bf16 products"),
             ("plain", f32s, dict(prec=F32, row_stride=Hc * 64 + 2), "16-byte alignment"),
             ("valu-drop", f32s, dict(p=0.25, row_stride=Hc * 64 + 2), "16-byte alignment"),
             ("bf16-drop", b16s, dict(p=0.25, row_stride=Hc * 64 + 2), "16-byte alignment"),
             ("plain", f32s, dict(prec=BF16, dq_ptr=4), "16-byte alignment"),
             ("valu-drop", f32s, dict(p=0.25, dq_ptr=4), "16-byte alignment"),
             ("bf16-drop", f32s, dict(p=0.25, dq_ptr=4), "16-byte alignment"),
             ("valu-drop", f32s, dict(p=1.0), "dropout_p outside"),
             ("bf16-drop", b16s, dict(p=1.0), "dropout_p outside")]
    for entry, (qd, kd, vd), kw, message in cases:
        dk, dv = _poison(Bc, T, Hc, 64), _poison(Bc, T, Hc, 64)
        dq_room = _poison(Bc * T * Hc * 64 + 16)
        dq = dq_room[:Bc * T * Hc * 64].view(Bc, T, Hc, 64)
        if "dq_ptr" in kw:
            kw = dict(kw, dq_ptr=dq.data_ptr() + kw["dq_ptr"])                        # 4 bytes on: room for it, but not 16-byte aligned
        delta = _poison(Bc * Hc * T + GUARD)
        rc = _raw(entry, qd, kd, vd, out, dout, lse, dq, dk, dv, delta, causal, **kw)
        assert rc != 0 and message in _hip.last_error(), (entry, kw, rc, _hip.last_error())
        for x in (dq_room, dk, dv, delta):
            assert bool(torch.isnan(x.cpu()).all()), (entry, kw)
