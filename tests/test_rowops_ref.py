"""rowops_ref.py checked on the CPU: every reference against something independent of it, the host packers against the project's two
torch packers bit for bit, the conditions the assertions of test_rowops_gpu.py rest on, on that test's inputs, and every pinned
tolerance against a re-measured fp32 CPU baseline."""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import rowops_ref as R
from kosmosx import _hip
from kosmosx import ops
from oracle import kosmos_oracle as O
from test_ops_gpu import _split3


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_the_bindings_tuning_key_mirrors_the_library():
    """test_rowops_gpu.py selects the LayerNorm kernel through _hip.KX_TUNE_LN_VARIANT: the number is the enum's."""
    plan = (Path(__file__).resolve().parent.parent / "kosmos-x_amd" / "csrc" / "kx_gemm_plan.h").read_text()
    assert int(re.search(r"\bKX_TUNE_LN_VARIANT\s*=\s*(\d+)", plan).group(1)) == _hip.KX_TUNE_LN_VARIANT


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [4, 260, 2052])
def test_layernorm_ref_matches_torch_float64(cols):
    g = _g(cols)
    x, pa = torch.randn(5, cols, generator=g) * 3 + 0.7, torch.randn(cols, generator=g)
    w, b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    eps = R._eps32(1e-5)
    for gamma, beta, pre in [(w, b, None), (None, b, None), (w, None, None), (None, None, None), (w, b, pa)]:
        xin = x.double() if pre is None else x.double() + pre.double()
        want = F.layer_norm(xin, (cols,), None if gamma is None else gamma.double(), None if beta is None else beta.double(), eps)
        got = R.layernorm_ref(x, gamma, beta, 1e-5, pre)
        assert got.dtype == torch.float64 and float((got - want).abs().max()) < 1e-13


def test_gelu_layernorm_ref_is_layernorm_of_the_rounded_activation():
    i = R.gelu_inputs(1028)
    act64 = F.gelu(i["pre"].double())
    got = R.gelu_layernorm_ref(i["pre"], i["gamma"], i["beta"])
    want = F.layer_norm(act64.float().double(), (1028,), i["gamma"].double(), i["beta"].double(), R._eps32(1e-5))
    assert float((got - want).abs().max()) < 1e-13
    # the rounding is there: the un-rounded float64 activation gives another (close) answer
    unrounded = F.layer_norm(act64, (1028,), i["gamma"].double(), i["beta"].double(), R._eps32(1e-5))
    d = float((got - unrounded).abs().max())
    assert 0 < d < 1e-6
    assert float(i["pre"].min()) < -5.9 and float(i["pre"].max()) > 5.9


def test_remap_rows_against_a_loop():
    y = torch.arange(6 * 3, dtype=torch.float32).reshape(6, 3) + 1
    out, untouched = R.remap_rows(y, 3, 5, 1, 10)
    want, mask = torch.zeros(10, 3), [True] * 10
    for row in range(6):
        orow = (row // 3) * 5 + 1 + row % 3
        want[orow] = y[row]
        mask[orow] = False
    assert torch.equal(out, want) and untouched.tolist() == mask
    assert untouched.tolist() == [True, False, False, False, True, True, False, False, False, True]
    ident, none = R.remap_rows(y, 6, 0, 0, 6)
    assert torch.equal(ident, y) and not bool(none.any())


# ---- operand formats ------------------------------------------------------------------------------------------------------------
def _format_inputs():
    g = _g(3)
    rnd = torch.randn(6, 64, generator=g) * torch.tensor([1e-4, 1e-2, 1.0, 30.0, 3e3, 3e5])[:, None]
    edges = torch.tensor([0.0, -0.0, 448.0, -448.0, 449.0, 464.0, 480.0, 1e4, -1e4, 65504.0, -65504.0, 65520.0, 65536.0, 1e5, -1e5, 3e38,
                          2.0 ** -6, 2.0 ** -7, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -10, 2.5 * 2.0 ** -9, 0.9 * 2.0 ** -6, 17.0, 18.0, 19.0,
                          20.0, 22.0, 26.0, 30.0, 31.0, 511.75, 512.25, 1023.75, 2.0 ** -24, 3.0e-8, 6.1e-5, -6.1e-5, 1.0009765625,
                          1.00048828125, 1.001953125, 1.005859375, 0.1, -0.1] + [0.0] * 20).reshape(1, 64)
    return torch.cat([rnd, edges, -edges], dim=0)


def test_e4m3_packer_is_the_format():
    """Every one of the 254 finite codes decodes (by the definition) to a value the packer maps back to that code, ties go to the
    even mantissa, and the clamp is at +-448."""
    codes = [c for c in range(256) if c & 0x7F != 0x7F]
    vals = []
    for c in codes:
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        v = (m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
        vals.append(-v if s else v)
    t = torch.tensor(vals, dtype=torch.float32).reshape(1, -1)
    assert R.pack_e4m3(t).reshape(-1).tolist() == codes
    assert torch.equal(R.pack_e4m3(t), t.to(torch.float8_e4m3fn).view(torch.uint8))
    assert max(vals) == 448.0
    ties = torch.tensor([[17.0, 19.0, 1.0625, 1.1875, 2.0 ** -10, 3 * 2.0 ** -10, 1e9, -1e9]])
    assert R.pack_e4m3(ties).reshape(-1).tolist() == R.pack_e4m3(torch.tensor([[16.0, 20.0, 1.0, 1.25, 0.0, 2.0 ** -8, 448.0, -448.0]])
                                                                 ).reshape(-1).tolist()


def test_packers_agree_bit_for_bit_with_the_projects_torch_packers():
    x = _format_inputs()
    assert bool((x.abs() > 65504).any()) and bool(((x.abs() > 448) & (x.abs() < 65504)).any())
    assert torch.equal(R.as_bytes(R.pack_bf16(x)), R.as_bytes(x.to(torch.bfloat16)))
    assert torch.equal(R.as_bytes(R.pack_f16(x)), R.as_bytes(x.clamp(-65504.0, 65504.0).to(torch.float16)))
    assert bool(torch.isfinite(R.pack_f16(x).float()).all())
    assert torch.equal(R.as_bytes(R.pack_bf16x3(x)), R.as_bytes(_split3(x, "hhl")))
    got, want = R.pack_f16c(x), ops.pack_f16c_rows(x)
    assert got.dtype == torch.uint8 and got.shape == (x.shape[0], 4 * x.shape[1]) and torch.equal(got, want)
    K = x.shape[1]
    # both e4m3 clamps are exercised by these inputs: the value part and the residual part hold +-448 (0x7E / 0xFE)
    for part in (got[:, 2 * K:3 * K], got[:, 3 * K:]):
        assert bool((part == 0x7E).any()) and bool((part == 0xFE).any())
    h, e, r = ops.unpack_f16c_rows(got, K)
    assert float(h.abs().max()) == 65504.0 and float(e.abs().max()) == 448.0 and float(r.abs().max()) == 448.0


# ---- the GPU test's LayerNorm inputs and tolerances ----------------------------------------------------------------------------
def test_layernorm_input_classes_are_what_they_claim():
    for cols in R.LN_COLS:
        i = R.ln_inputs("intconst", cols)
        x = i["x"]
        assert torch.equal(x, (torch.arange(7.0) + 3)[:, None].expand(7, cols))
        s = x.sum(-1)                                                       # fp32: the sums are exact, so the mean is
        assert torch.equal(s, (torch.arange(7.0) + 3) * cols) and torch.equal(s / cols, x[:, 0])
        assert torch.equal(R.ln_reference("intconst", cols), i["beta"].double()[None].expand(7, cols))
        off = R.ln_inputs("offset", cols)["x"].double()
        assert bool(((off.mean(-1) - 300.0 * torch.arange(1, 8)).abs() < 2).all())
        sp = R.ln_inputs("spike", cols)["x"]
        assert bool((sp[:, cols - 2] == 1e4).all()) and cols - 2 >= cols - 4 and int((sp == 1e4).sum()) == 7
        for cls, gam, bet, pa in [("null_gamma", False, True, False), ("null_beta", True, False, False),
                                  ("null_both", False, False, False), ("pre_add", True, True, True)]:
            j = R.ln_inputs(cls, cols)
            assert (j["gamma"] is not None, j["beta"] is not None, j["pre_add"] is not None) == (gam, bet, pa)
        # saturating: the reference output passes +-65504 and lies between 448 and 65504 on both sides; the fp16 residual
        # (v - fp16(v)) * 2^11 passes +-448 as well, at a saturated fp16 part and at an unsaturated one
        y = R.ln_reference("saturating", cols)
        assert float(y.max()) > 65504 * 1.01 and float(y.min()) < -65504 * 1.01, cols
        mid = y[:, 1::2]
        assert bool(((mid > 448 * 1.01) & (mid < 65504)).any()) and bool(((mid < -448 * 1.01) & (mid > -65504)).any()), cols
        rows = R.pack_f16c(y.float())
        for part in (rows[:, 2 * cols:3 * cols], rows[:, 3 * cols:]):
            assert bool((part == 0x7E).any()) and bool((part == 0xFE).any()), cols


def test_layernorm_tolerances_are_tied_to_the_fp32_cpu_baseline():
    for cls, pinned in R.LN_CPU_ERR.items():
        m = R.ln_cpu_fp32_error(cls)
        print(f"LayerNorm {cls}: torch fp32 CPU max|err| {m:.3e}, pinned {pinned:.3e}, kernel bound {R.ln_tol(cls):.3e}")
        assert m <= pinned <= 4 * m, (cls, m, pinned)
        assert R.ln_tol(cls) == R.LN_TOL_FACTOR * pinned
    assert R.LN_TOL_FACTOR == 4.0 and R.ln_tol("intconst") == 0.0
    for cls in ("baseline", "null_gamma", "null_beta", "null_both", "pre_add"):    # the project's bound holds for the CPU operator too
        m = R.ln_cpu_fp32_error(cls)
        print(f"LayerNorm {cls}: torch fp32 CPU max|err| {m:.3e}, bound {R.ln_tol(cls):.1e}")
        assert R.ln_tol(cls) == 2e-5 and m < 2e-5
    m = R.gelu_cpu_fp32_error()
    print(f"LayerNorm(gelu): torch fp32 CPU max|err| {m:.3e}, pinned {R.GELU_CPU_ERR:.3e}, kernel bound {R.gelu_tol():.3e}")
    assert m <= R.GELU_CPU_ERR <= 4 * m
    assert R.gelu_tol() == max(2e-5, 4 * R.GELU_CPU_ERR)


# ---- row statistics -------------------------------------------------------------------------------------------------------------
def finalize_fp32(partials, seg_size, eps=1e-5):
    """kx_row_stats_finalize's formula in fp32 by torch on the CPU: the baseline of the kernel's tolerance."""
    p = partials.float()
    n = torch.tensor(float(seg_size)) * float(p.shape[1])
    mean = p[..., 0].sum(-1) / n
    d = p[..., 0] / float(seg_size) - mean[:, None]
    var = (p[..., 1] + float(seg_size) * d * d).sum(-1) / n
    return mean, torch.rsqrt(var + eps)


@pytest.mark.parametrize("nseg,seg", R.FIN_SHAPES)
def test_finalize_ref_of_exact_partials_is_the_rows_mean_and_variance(nseg, seg):
    g = _g(nseg)
    x = torch.randn(5, nseg * seg, generator=g) * 3 + 20
    p = R.make_partials(x, seg)
    assert p.dtype == torch.float32 and p.shape == (5, nseg, 2)
    mean, rstd = R.row_stats_finalize_ref(p, seg, 1e-5)
    xd = x.double()
    assert float((mean - xd.mean(-1)).abs().max()) < 1e-6 * 20          # the partials were rounded once to fp32 (2^-24 relative)
    want = 1.0 / torch.sqrt(xd.var(-1, unbiased=False) + R._eps32(1e-5))
    assert float(((rstd - want) / want).abs().max()) < 1e-6


def test_finalize_tolerances_are_tied_to_the_fp32_cpu_baseline():
    for cls in R.FIN_CLASSES:
        em = er = 0.0
        for nseg, seg in R.FIN_SHAPES:
            p = R.fin_partials(cls, nseg, seg)
            mean, rstd = R.row_stats_finalize_ref(p, seg)
            m32, r32 = finalize_fp32(p, seg)
            em = max(em, float((m32.double() - mean).abs().max()))
            er = max(er, float(((r32.double() - rstd) / rstd).abs().max()))
        pm, pr = R.FIN_CPU_ERR[cls]
        print(f"finalize {cls}: fp32 CPU mean err {em:.3e} (pinned {pm:.3e}), rstd rel err {er:.3e} (pinned {pr:.3e}), bounds {R.fin_tol(cls)}")
        assert em <= pm <= 4 * em or (em == 0.0 and pm == 0.0), (cls, em, pm)
        assert er <= pr <= 4 * er, (cls, er, pr)
        assert R.fin_tol(cls) == (max(2e-5, 4 * pm), max(2e-5, 4 * pr))
    off = R.fin_partials("offset", 128, 64).double()                        # the class is what it claims: seg * d^2 dominates M2
    d = off[..., 0] / 64 - (off[..., 0].sum(-1) / (128 * 64))[:, None]
    assert float((64 * d * d).sum()) > 20 * float(off[..., 1].sum())


# ---- embedding assembly ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alias", [True, False])
def test_embed_references_against_the_oracle(alias):
    g = _g(2)
    B, Tt, n, d, V, P = 3, 10, 8, 64, 302, 64
    tok = torch.randint(0, V, (B, Tt), generator=g)
    emb, pos = torch.randn(V, d, generator=g), torch.randn(P, d, generator=g)
    img = torch.randn(B, n, d, generator=g)
    cfg = O.DecoderCfg(vocab=V, max_pos=P, dim=d)
    x, e = O.forward_embedding_tokens({"embed.weight": emb, "embed_positions.weight": pos}, tok, cfg)
    first = x if alias else e
    want = 1.0 * torch.cat([first[:, 0:2], img, first[:, 2:]], dim=1) + pos[O.positions_for(Tt + n)][None]
    assert torch.equal(R.embed_splice_ref(tok, emb, pos, img, alias, 2), want)
    assert torch.equal(R.embed_splice_ref(tok, emb, pos), x)                # text only: one position add
    # one decode step is one row of the same assembly: text index tt, spliced index t = tt + n
    for tt in (2, Tt - 1):
        t = tt + n
        a, b = (tt, t) if alias else (t, -1)
        assert torch.equal(R.embed_step_ref(tok[:, tt], emb, pos, a, b), want[:, t])
        x0, xr0 = torch.full((B, d), 7.0), None
        got, _, word = R.step_prepare_ref(tok[:, tt], emb, pos, torch.full((B,), t), None, n if alias else 0, x0, xr0)
        assert word == 0 and torch.equal(got, want[:, t])
    assert torch.equal(R.embed_step_ref(tok[:, 1], emb, pos, 1), x[:, 1])
    # the position-overflow condition is the oracle's
    long_tok = torch.zeros(1, P - 1, dtype=torch.long)
    with pytest.raises(IndexError):
        O.forward_embedding_tokens({"embed.weight": emb, "embed_positions.weight": pos}, long_tok, cfg)
    with pytest.raises(IndexError):
        R.embed_splice_ref(long_tok, emb, pos)
    R.embed_splice_ref(long_tok[:, :P - 2], emb, pos)
    with pytest.raises(IndexError):
        R.embed_splice_ref(long_tok[:, :P - 9], emb, pos, pos_offset=8)
    R.embed_splice_ref(long_tok[:, :P - 10], emb, pos, pos_offset=8)


def test_embed_references_clamp_ids_shift_positions_and_leave_rejected_rows():
    g = _g(4)
    V, d, P = 11, 8, 20
    emb, pos = torch.randn(V, d, generator=g), torch.randn(P, d, generator=g)
    tok = torch.tensor([[-1, V, 3]])
    out = R.embed_splice_ref(tok, emb, pos, pos_offset=5)
    assert torch.equal(out[0, 0], emb[0] + pos[7]) and torch.equal(out[0, 1], emb[V - 1] + pos[8]) and torch.equal(out[0, 2], emb[3] + pos[9])
    img = torch.randn(1, 2, d, generator=g)
    for s in (0, 3):                                        # the image rows first, or last
        o = R.embed_splice_ref(tok, emb, pos, img, True, s, 1)
        txt = [2, 3, 4] if s == 0 else [0, 1, 2]
        for k, t in enumerate(txt):
            assert torch.equal(o[0, t], (emb[tok[0, k].clamp(0, V - 1)] + pos[3 + k]) + pos[3 + t])
        for k in range(2):
            assert torch.equal(o[0, s + k], img[0, k] + pos[3 + s + k])
    assert torch.equal(R.embed_splice_ref(None, emb, pos, img, True, 0, 0)[0], img[0] + pos[2:4])
    tables = [torch.randn(9, 32, generator=g) for _ in range(4)]
    positions = torch.tensor([2, 1, 17, 18, 9, 8])          # pos_shift 2: 1 is below it; 18 + 2 == P; 9 == xpos_len; 17 >= xpos_len
    x0, xr0 = torch.full((6, d), 7.0), torch.full((4, 6, 32), 7.0)
    toks = torch.tensor([0, 1, 2, 3, 4, V + 5])
    x, xr, word = R.step_prepare_ref(toks, emb, pos, positions, tables, 2, x0, xr0)
    assert word == R.ERR_TABLE and bool((x0 == 7).all())
    for b in (1, 2, 3, 4):
        assert bool((x[b] == 7).all()) and bool((xr[:, b] == 7).all())
    assert torch.equal(x[0], (emb[0] + pos[2]) + pos[4]) and torch.equal(x[5], (emb[V - 1] + pos[8]) + pos[10])
    assert all(torch.equal(xr[k, 5], tables[k][8]) for k in range(4))
    x, xr, word = R.step_prepare_ref(toks, emb, pos, positions, None, 2, x0, None, error_word=0)
    assert xr is None and word == R.ERR_TABLE and not bool((x[2] == 7).any()) and bool((x[3] == 7).all())
    assert R.step_prepare_ref(toks[:1], emb, pos, positions[:1], None, 2, x0[:1], None, error_word=R.ERR_TABLE)[2] == R.ERR_TABLE


def test_token_range_ref():
    lo, hi = -2 ** 63, 2 ** 63 - 1
    t = torch.tensor([[5, -3, hi], [lo, 0, 7]])
    assert R.token_range_ref(t) == (lo, hi) == (int(t.min()), int(t.max()))
    assert R.token_range_ref(torch.tensor([4])) == (4, 4)
