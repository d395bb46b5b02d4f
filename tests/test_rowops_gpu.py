"""The forward-path row kernels (csrc/kx_rowops.hip: kx_layernorm, kx_gelu_layernorm, kx_row_stats_finalize, kx_embed_splice,
kx_token_range) and the two embedding kernels of csrc/kx_sample.hip (kx_embed_step, kx_step_prepare) against the restatements of
tests/rowops_ref.py, which tests/test_rowops_ref.py checks on the CPU.

LayerNorm: KX_TUNE_LN_VARIANT forces each of the two kernels at every width, so every instantiation is launched: the wave-per-row
kernel layernorm_kernel<OUT, NV> (NV = 4 up to 1024 columns, 8 up to 2048, 16 up to 4096, 32 above) and the workgroup-per-row kernel
layernorm_block_kernel<OUT>, each in the five output formats.  Two assertions per case:
  1. the fp32 output is within rowops_ref.ln_tol(class) of the float64 reference (a bound derived there from torch's fp32 CPU error);
  2. every 16-bit or operand-format output EQUALS the host packer applied to the fp32 output of the same kernel at the same shape.
The embedding kernels add fp32 rows in a documented order: equality.  No case provokes a fault: ids outside the table are clamped
before anything is read through them, a position outside the tables makes kx_step_prepare return before it reads or writes the row,
and the launchers refuse the rest on the host.

Measured on the MI355X (worst over widths, rows and both kernels / bound): LayerNorm baseline 7.5e-7 / 2e-5, offset 4.7e-4 / 2.2e-3,
spike 9.9e-6 / 6e-5, saturating 5.9e-2 / 3.6e-1, pre_add 8.7e-7 / 2e-5, integer-constant rows exactly beta; LayerNorm(gelu) 1.3e-6 /
2.6e-5; finalize mean 4.3e-6 / 4.8e-5 (offset) and 8e-8 / 2e-5, rstd 1.1e-7 / 2e-5.  Every test prints its figures before it asserts."""
import contextlib

import pytest
import torch

import rowops_ref as R
from kosmosx import _hip
from kosmosx import grad_ops
from kosmosx import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
# kx_layernorm's dispatch on KX_TUNE_LN_VARIANT: 0 = the shipped rule (wave kernel up to 2048 columns, block kernel above), 1 = the
# block kernel at every width, any other value = the wave kernel at every width (2 is used here)
LN_SHIPPED, LN_BLOCK, LN_WAVE = 0, 1, 2
VARIANTS = {"wave": LN_WAVE, "block": LN_BLOCK}
SENTINEL = 0xA5


@contextlib.contextmanager
def ln_variant(value):
    lib = _hip.load()
    assert lib.kx_set_tuning(_hip.KX_TUNE_LN_VARIANT, value) == 0
    try:
        yield
    finally:
        lib.kx_set_tuning(_hip.KX_TUNE_LN_VARIANT, LN_SHIPPED)


def _dev(t):
    return None if t is None else t.to(DEV)


def _ln(inp, rows, fmt="f32", out=None, **remap):
    """kx_layernorm on the first `rows` rows of an input set, in one output format -> the output on the CPU."""
    kw = {"f32": {}, "bf16": {"out_dtype": torch.bfloat16}, "f16": {"out_dtype": torch.float16}, "bf16x3": {"x3": True},
          "f16c": {"f16c": True}}[fmt]
    y = ops.layernorm(inp["x"][:rows].contiguous().to(DEV), _dev(inp["gamma"]), _dev(inp["beta"]), R.EPS, pre_add=_dev(inp["pre_add"]),
                      out=out, **kw, **remap)
    torch.cuda.synchronize()
    return y.cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(R.as_bytes(a), R.as_bytes(b))


# ---- kx_layernorm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", R.LN_COLS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_layernorm_fp32_against_float64(variant, cols):
    worst = {}
    with ln_variant(VARIANTS[variant]):
        for cls in R.LN_CLASSES:
            inp, ref = R.ln_inputs(cls, cols), R.ln_reference(cls, cols)
            for rows in R.LN_ROWS:
                y = _ln(inp, rows)
                assert y.dtype == torch.float32 and y.shape == (rows, cols) and bool(torch.isfinite(y).all())
                err = float((y.double() - ref[:rows]).abs().max())
                worst[cls] = max(worst.get(cls, 0.0), err)
                if cls == "intconst":      # exact sum, exact mean, centred values all zero: anything but beta is a wrong divisor or lane
                    assert _same_bits(y, inp["beta"][None].expand(rows, cols).contiguous()), (cls, rows)
                assert err <= R.ln_tol(cls), (cls, rows, err, R.ln_tol(cls))
    print(f"layernorm {variant} cols={cols}: " + ", ".join(f"{c} {e:.2e}/{R.ln_tol(c):.1e}" for c, e in worst.items()))


@pytest.mark.parametrize("cols", R.LN_COLS)
def test_layernorm_shipped_rule_is_one_of_the_two_kernels(cols):
    """Under the default the bits are the wave kernel's up to 2048 columns and the block kernel's above."""
    for cls in ("baseline", "offset", "pre_add"):
        inp = R.ln_inputs(cls, cols)
        y = _ln(inp, 7)
        assert float((y.double() - R.ln_reference(cls, cols)).abs().max()) <= R.ln_tol(cls)
        with ln_variant(LN_WAVE if cols <= 2048 else LN_BLOCK):
            same = _ln(inp, 7)
        assert _same_bits(y, same), cls


@pytest.mark.parametrize("fmt", R.FORMATS[1:])
@pytest.mark.parametrize("cols", R.LN_COLS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_layernorm_formats_are_the_packed_fp32_output(variant, cols, fmt):
    with ln_variant(VARIANTS[variant]):
        for cls, row_list in (("baseline", R.LN_ROWS), ("pre_add", R.LN_ROWS), ("null_both", [6]), ("spike", [7])):
            inp = R.ln_inputs(cls, cols)
            for rows in row_list:
                y32, yf = _ln(inp, rows), _ln(inp, rows, fmt)
                assert _same_bits(yf, R.PACKERS[fmt](y32)), (cls, rows)


@pytest.mark.parametrize("cols", R.LN_COLS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_layernorm_saturating_outputs_clamp(variant, cols):
    """Outputs beyond +-65504 and +-448: the fp16 parts saturate (no infinity), both e4m3 parts clamp, in both kernels."""
    inp = R.ln_inputs("saturating", cols)
    with ln_variant(VARIANTS[variant]):
        y32 = _ln(inp, 7)
        err = float((y32.double() - R.ln_reference("saturating", cols)).abs().max())
        print(f"layernorm {variant} cols={cols}: saturating {err:.2e}/{R.ln_tol('saturating'):.1e}")
        assert err <= R.ln_tol("saturating")
        assert float(y32.max()) > 65504 and float(y32.min()) < -65504
        out = {fmt: _ln(inp, 7, fmt) for fmt in R.FORMATS[1:]}
    for fmt, y in out.items():
        assert _same_bits(y, R.PACKERS[fmt](y32)), fmt
    h = out["f16"].float()
    assert bool(torch.isfinite(h).all()) and float(h.max()) == 65504.0 and float(h.min()) == -65504.0
    hc, e, r = ops.unpack_f16c_rows(out["f16c"], cols)
    assert torch.equal(hc, h)
    assert float(e.max()) == 448.0 and float(e.min()) == -448.0 and float(r.max()) == 448.0 and float(r.min()) == -448.0
    assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(r).all())
    assert bool(torch.isfinite(out["bf16x3"].float()).all())


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("cols", [4, 260, 2052, 4100])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_layernorm_row_remap_in_every_format(variant, cols, fmt):
    """6 rows in groups of 3 into a 10-row buffer (stride 5, offset 1), with pre_add: the named rows hold the packed fp32 result at the
    format's own row pitch, rows 0, 4, 5 and 9 keep the sentinel byte for byte."""
    rows, rpg, ogs, oro, total = 6, 3, 5, 1, 10
    inp = R.ln_inputs("pre_add", cols)
    width, dtype = {"f32": (cols, torch.float32), "bf16": (cols, torch.bfloat16), "f16": (cols, torch.float16),
                    "bf16x3": (3 * cols, torch.bfloat16), "f16c": (4 * cols, torch.uint8)}[fmt]
    buf = torch.full((total, width * dtype.itemsize), SENTINEL, dtype=torch.uint8, device=DEV).view(dtype)
    assert buf.shape == (total, width)
    with ln_variant(VARIANTS[variant]):
        y32 = _ln(inp, rows)
        got = _ln(inp, rows, fmt, out=buf, rows_per_group=rpg, out_group_stride=ogs, out_row_offset=oro)
    assert float((y32.double() - R.ln_reference("pre_add", cols)[:rows]).abs().max()) <= R.ln_tol("pre_add")
    packed = y32 if fmt == "f32" else R.PACKERS[fmt](y32)
    want, untouched = R.remap_rows(R.as_bytes(packed), rpg, ogs, oro, total)
    assert untouched.tolist() == [True, False, False, False, True, True, False, False, False, True]
    want[untouched] = SENTINEL
    assert torch.equal(R.as_bytes(got), want)


def test_layernorm_variant_is_back_at_the_shipped_rule():
    """Every test above restores the knob in a finally; a wide row under the default takes the block kernel again."""
    inp = R.ln_inputs("baseline", 4100)
    y = _ln(inp, 6)
    with ln_variant(LN_BLOCK):
        blk = _ln(inp, 6)
    with ln_variant(LN_WAVE):
        wav = _ln(inp, 6)
    assert _same_bits(y, blk)
    narrow = R.ln_inputs("baseline", 1028)
    with ln_variant(LN_WAVE):
        wav_n = _ln(narrow, 6)
    assert _same_bits(_ln(narrow, 6), wav_n)
    for t in (wav, blk):
        assert float((t.double() - R.ln_reference("baseline", 4100)[:6]).abs().max()) <= R.ln_tol("baseline")


# ---- kx_gelu_layernorm ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", R.GELU_ROWS)
@pytest.mark.parametrize("cols", R.GELU_COLS)
def test_gelu_layernorm_against_float64(cols, rows):
    """cols <= 1024: layernorm_kernel<*, 4, true>; <= 2048: <*, 8, true>; above: layernorm_block_kernel<*, true>."""
    i = R.gelu_inputs(cols)
    pre, gamma, beta = i["pre"][:rows].contiguous().to(DEV), i["gamma"].to(DEV), i["beta"].to(DEV)
    y = grad_ops.gelu_layernorm(pre, gamma, beta, R.EPS).cpu()
    y16 = grad_ops.gelu_layernorm(pre, gamma, beta, R.EPS, out_dtype=torch.bfloat16).cpu()
    err = float((y.double() - R.gelu_reference(cols)[:rows]).abs().max())
    print(f"gelu_layernorm cols={cols} rows={rows}: {err:.2e}/{R.gelu_tol():.1e}")
    assert y.dtype == torch.float32 and err <= R.gelu_tol()
    assert _same_bits(y16, R.pack_bf16(y))


# ---- kx_row_stats_finalize ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", R.FIN_CLASSES)
@pytest.mark.parametrize("nseg,seg", R.FIN_SHAPES)
def test_row_stats_finalize_on_synthetic_partials(nseg, seg, cls):
    p = R.fin_partials(cls, nseg, seg)
    mean, rstd = R.row_stats_finalize_ref(p, seg, R.EPS)
    tol_m, tol_r = R.fin_tol(cls)
    for rows in (1, 6, 7):
        out = ops.row_stats_finalize(p[:rows].contiguous().to(DEV), seg, R.EPS).cpu().double()
        em = float((out[:, 0] - mean[:rows]).abs().max())
        er = float(((out[:, 1] - rstd[:rows]) / rstd[:rows]).abs().max())
        print(f"finalize {cls} nseg={nseg} seg={seg} rows={rows}: mean {em:.2e}/{tol_m:.1e}, rstd {er:.2e}/{tol_r:.1e}")
        assert out.shape == (rows, 2) and em <= tol_m and er <= tol_r, (rows, em, er)


# ---- kx_embed_splice ------------------------------------------------------------------------------------------------------------
VOCAB, MAX_POS = 37, 32


def _tables(d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(VOCAB, d, generator=g), torch.randn(MAX_POS, d, generator=g), g


@pytest.mark.parametrize("pos_offset", [0, 7])
@pytest.mark.parametrize("alias", [True, False], ids=["u1", "no_u1"])
@pytest.mark.parametrize("Tt,n_img,splice_at", [(5, 3, 0), (5, 3, 5), (5, 3, 2), (0, 4, 0), (1, 0, 0)])
@pytest.mark.parametrize("d", [4, 260, 2048])
def test_embed_splice_equals_the_reference_order(d, Tt, n_img, splice_at, alias, pos_offset):
    emb, pos, g = _tables(d, 100 + d)
    B = 2
    tok = torch.randint(0, VOCAB, (B, Tt), generator=g) if Tt else None
    img = torch.randn(B, n_img, d, generator=g) if n_img else None
    want = R.embed_splice_ref(tok, emb, pos, img, alias, splice_at, pos_offset)
    got = ops.embed_splice(_dev(tok), emb.to(DEV), pos.to(DEV), _dev(img), alias, splice_at, pos_offset)
    assert got.shape == (B, Tt + n_img, d) and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("d", [4, 2048])
def test_embed_splice_clamps_ids_outside_the_table(d):
    emb, pos, g = _tables(d, 200 + d)
    tok = torch.tensor([[-1, VOCAB, 3, -2 ** 63], [2 ** 63 - 1, 0, VOCAB - 1, 5]])
    img = torch.randn(2, 2, d, generator=g)
    for im, s in ((None, 0), (img, 1)):
        got = ops.embed_splice(tok.to(DEV), emb.to(DEV), pos.to(DEV), _dev(im), True, s, 3).cpu()
        assert torch.equal(got, R.embed_splice_ref(tok, emb, pos, im, True, s, 3))
    assert torch.equal(got[0, 0], (emb[0] + pos[5]) + pos[5]) and torch.equal(got[0, 3], (emb[VOCAB - 1] + pos[6]) + pos[8])


def test_embed_splice_position_overflow_with_an_offset():
    """pos_offset + Tt + n_img + 2 <= max_pos: with 7 cached positions and 3 image rows a 32-row table admits 20 text tokens."""
    emb, pos, g = _tables(8, 300)
    img = torch.randn(1, 3, 8, generator=g)
    fits = torch.randint(0, VOCAB, (1, 20), generator=g)
    got = ops.embed_splice(fits.to(DEV), emb.to(DEV), pos.to(DEV), img.to(DEV), True, 2, 7)
    assert torch.equal(got.cpu(), R.embed_splice_ref(fits, emb, pos, img, True, 2, 7))
    over = torch.randint(0, VOCAB, (1, 21), generator=g)
    with pytest.raises(IndexError):
        R.embed_splice_ref(over, emb, pos, img, True, 2, 7)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.embed_splice(over.to(DEV), emb.to(DEV), pos.to(DEV), img.to(DEV), True, 2, 7)


# ---- kx_embed_step and kx_step_prepare ------------------------------------------------------------------------------------------
XPOS_LEN = 27           # shorter than the position table: t == XPOS_LEN is inside pos (t + 2 < MAX_POS) and outside the XPos tables


@pytest.mark.parametrize("pos_shift", [0, 3])
@pytest.mark.parametrize("d", [4, 2048])
def test_embed_step_equals_the_reference_order(d, pos_shift):
    emb, pos, g = _tables(d, 400 + d)
    tok = torch.tensor([5, -1, VOCAB, 0, VOCAB - 1, 17])
    for t in (pos_shift, 11, MAX_POS - 3):                                  # the first valid position, one inside, the last valid one
        a, b = (t - pos_shift, t) if pos_shift else (t, -1)
        got = ops.embed_step(tok.to(DEV), emb.to(DEV), pos.to(DEV), a, b)
        assert torch.equal(got.cpu(), R.embed_step_ref(tok, emb, pos, a, b)), t
    for a, b in ((MAX_POS - 2, -1), (0, MAX_POS - 2), (-1, 2)):             # t + 2 == max_pos in either slot, and one below the shift
        with pytest.raises(IndexError):
            R.embed_step_ref(tok, emb, pos, a, b)
        with pytest.raises(RuntimeError, match="out of range"):
            ops.embed_step(tok.to(DEV), emb.to(DEV), pos.to(DEV), a, b)


@pytest.mark.parametrize("with_tables", [True, False], ids=["xpos", "no_xpos"])
@pytest.mark.parametrize("pos_shift", [0, 3])
@pytest.mark.parametrize("d", [4, 2048])
def test_step_prepare_equals_the_reference_and_leaves_rejected_rows(d, pos_shift, with_tables):
    emb, pos, g = _tables(d, 500 + d)
    tables = [torch.randn(XPOS_LEN, 32, generator=g) for _ in range(4)] if with_tables else None
    last = (XPOS_LEN if with_tables else MAX_POS - 2) - 1
    #            first valid, last valid, below the shift, t + 2 == max_pos, t == xpos_len, one inside, far outside
    positions = [pos_shift, last, pos_shift - 1, MAX_POS - 2, XPOS_LEN, 11, 10 ** 6]
    rejected = [False, False, True, True, with_tables, False, True]
    tok = torch.tensor([5, VOCAB, 9, 1, 2, -1, 3])
    p = torch.tensor(positions, dtype=torch.int32)
    x0 = torch.full((len(positions), d), 7.0)
    xr0 = torch.full((4, len(positions), 32), 7.0) if with_tables else None
    want_x, want_xr, want_word = R.step_prepare_ref(tok, emb, pos, p, tables, pos_shift, x0, xr0)
    assert want_word == _hip.KX_RAGGED_ERR_TABLE == R.ERR_TABLE
    for b, rej in enumerate(rejected):
        assert bool((want_x[b] == 7.0).all()) == rej
    dt = None if tables is None else [t.to(DEV) for t in tables]
    x, xr, err = ops.step_prepare(tok.to(DEV), emb.to(DEV), pos.to(DEV), p.to(DEV), dt, pos_shift=pos_shift, out=x0.to(DEV),
                                  xpos_rows=_dev(xr0))
    torch.cuda.synchronize()
    assert int(err.item()) == _hip.KX_RAGGED_ERR_TABLE
    assert torch.equal(x.cpu(), want_x)                                      # valid rows written, rejected rows still the sentinel
    if with_tables:
        assert torch.equal(xr.cpu(), want_xr)
        for b, rej in enumerate(rejected):
            assert bool((xr[:, b] == 7.0).all()) == rej
    else:
        assert xr is None
    # the error word is sticky: a clean launch on the same word leaves the bit, and writes every row
    good = [b for b, rej in enumerate(rejected) if not rej]
    x1, xr1, err1 = ops.step_prepare(tok[good].to(DEV), emb.to(DEV), pos.to(DEV), p[good].contiguous().to(DEV), dt, pos_shift=pos_shift,
                                     error_word=err)
    assert int(err1.item()) == _hip.KX_RAGGED_ERR_TABLE and torch.equal(x1.cpu(), want_x[good])
    fresh = ops.step_prepare(tok[good].to(DEV), emb.to(DEV), pos.to(DEV), p[good].contiguous().to(DEV), dt, pos_shift=pos_shift)
    assert int(fresh[2].item()) == 0 and torch.equal(fresh[0].cpu(), want_x[good])
    if with_tables:
        assert torch.equal(xr1.cpu(), want_xr[:, good]) and torch.equal(fresh[1].cpu(), want_xr[:, good])


# ---- kx_token_range -------------------------------------------------------------------------------------------------------------
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
RANGE_N = [1, 63, 64, 65, 256, 257, 1024 * 256 + 3]        # the last: 1024 workgroups of 256, so three threads take a second element


def _range(tokens, out=None):
    got = ops.token_range(tokens.to(DEV), out)
    torch.cuda.synchronize()
    return tuple(int(v) for v in got.cpu().tolist())


@pytest.mark.parametrize("n", RANGE_N)
def test_token_range_against_python_min_max(n):
    g = torch.Generator().manual_seed(n)
    t = torch.randint(-1000, 1000, (n,), generator=g)
    assert R.token_range_ref(t) == (int(t.min()), int(t.max()))
    assert _range(t) == R.token_range_ref(t)
    # values that differ only above bit 31, or only in the sign of the upper half: a 32-bit shuffle or an unsigned compare shows
    wide = t * (2 ** 33 + 1) - 5
    assert _range(wide) == R.token_range_ref(wide)
    neg = -(t.abs()) - 2 ** 40
    assert _range(neg) == R.token_range_ref(neg)
    # the extremes anywhere, then in the last wave
    for lo_at, hi_at in ((0, n // 2), (n - 1, max(n - 2, 0)), (max(n - 64, 0), n - 1)):
        e = t.clone()
        e[hi_at] = I64_MAX
        e[lo_at] = I64_MIN if lo_at != hi_at else e[lo_at]
        assert _range(e) == R.token_range_ref(e), (lo_at, hi_at)


def test_token_range_minimum_and_maximum_in_one_lane():
    """One thread, and one lane position of two waves, hold both extremes; every other element lies strictly between."""
    n = RANGE_N[-1]
    t = torch.randint(-1000, 1000, (n,), generator=torch.Generator().manual_seed(9))
    t[1], t[1 + 1024 * 256] = I64_MIN, I64_MAX                              # the grid-stride loop brings both to thread 1 of workgroup 0
    assert _range(t) == (I64_MIN, I64_MAX)
    t[1], t[1 + 1024 * 256] = -(2 ** 40), 2 ** 40
    assert _range(t) == (-(2 ** 40), 2 ** 40)
    s = torch.randint(-1000, 1000, (256,), generator=torch.Generator().manual_seed(10))
    s[5], s[5 + 64] = -5000, 5000                                           # lane 5 of wave 0 and of wave 1
    assert _range(s) == (-5000, 5000)
    one = torch.tensor([I64_MIN])
    assert _range(one) == (I64_MIN, I64_MIN) and _range(-(one + 1)) == (I64_MAX, I64_MAX)


def test_token_range_launcher_reinitialises_the_result():
    out = torch.empty(2, dtype=torch.int64, device=DEV)
    wide = torch.tensor([-7, 3, 900, I64_MIN, I64_MAX])
    assert _range(wide, out) == (I64_MIN, I64_MAX)
    narrow = torch.tensor([4, 6, 5])
    assert _range(narrow, out) == (4, 6)                                     # not the minimum / maximum left by the first call
    assert _range(torch.tensor([-9]), out) == (-9, -9)
