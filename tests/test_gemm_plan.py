"""kx_gemm's launch plan, pinned without a GPU.  kx_gemm_describe prints the plan kx_gemm would execute (one pure host function
of the arguments, a snapshot of the tuning table and the CU count: csrc/kx_gemm_plan.h); tests/golden/gemm_plan.json holds, per
case of tools/gemm_plan_sweep.py, the launches a kernel trace of the parent commit (recorded in the file) showed on the MI355X.
The description must name the same kernels with the same template arguments, grid and block.  The file's `lds` is a property of
the compiled kernel (static + dynamic bytes as the trace reports them; the planner passes no dynamic LDS), kept as a record only."""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "gemm_plan.json").read_text())


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from kosmosx import _hip
    return _hip.load()


@pytest.fixture(scope="module")
def described(lib):
    """name -> the sweep's description record at the golden file's CU count (computed once, shared)."""
    sys.path.insert(0, str(ROOT / "tools"))
    import gemm_plan_sweep as S
    return {r["name"]: r for r in S.describe_all(GOLDEN["cu_count"])}


def _without_lds(launches):
    return [{k: v for k, v in rec.items() if k != "lds"} for rec in launches]


def _golden_launches(ids):
    from kosmosx import ops
    return ops.parse_gemm_description("\n".join(GOLDEN["launches"][i] for i in ids))[0]


def test_every_golden_case_is_described_as_the_parent_launched_it(described):
    assert len(GOLDEN["cases"]) > 1000 and GOLDEN["cu_count"] == 256
    for name, want in GOLDEN["cases"].items():
        got = described[name]
        if isinstance(want, str):
            assert want.startswith("refused: ") and want[len("refused: "):] in got.get("refused", ""), (name, want, got)
        else:
            assert "launches" in got, (name, got)
            assert _without_lds(got["launches"]) == _without_lds(_golden_launches(want)), (name, got["launches"], want)


def test_the_sweep_covers_every_instantiation_class(described):
    """Over the GOLDEN file (so a thinned sweep fails): every EPI value, each NST, the pair split, the in-launch reduce, both
    reduce kernels at both widths; over the descriptions of the same cases: every KX_K_GEMM_* kind."""
    seen = {"tile_epi": set(), "nst": set(), "p5_epi": set(), "ks2": set(), "coop": set(), "bal": set(), "phased": set(), "reduce": set(),
            "family": set()}
    used = sorted({i for v in GOLDEN["cases"].values() if not isinstance(v, str) for i in v})
    assert used == list(range(len(GOLDEN["launches"])))
    for rec in _golden_launches(used):
        a = rec.get("args", [])
        seen["family"].add(rec["kernel"])
        if rec["kernel"] == "gemm_kernel":
            seen["tile_epi"].add(a[4]); seen["nst"].add(a[5]); seen["coop"].add(a[6])
        elif rec["kernel"] == "gemm_kernel_p5":
            seen["p5_epi"].add(a[3]); seen["ks2"].add(a[4]); seen["bal"].add(a[5])
        elif rec["kernel"] == "gemm_kernel_p3":
            seen["phased"].add(a[2])
        elif rec["kernel"].startswith("splitk"):
            seen["reduce"].add((rec["kernel"], a[-1] if rec["kernel"].endswith("rows_kernel") else ""))
    assert seen["tile_epi"] == {"0", "1"} and seen["nst"] == {"2", "4", "8"} and seen["coop"] == {"false", "true"}
    assert seen["p5_epi"] == {"0", "1", "4", "5", "6", "7", "8", "9"}
    assert seen["ks2"] == {"false", "true"} and seen["bal"] == {"false", "true"} and seen["phased"] == {"false", "true"}
    assert seen["reduce"] == {("splitk_reduce_kernel", ""), ("splitk_reduce_rows_kernel", "2"), ("splitk_reduce_rows_kernel", "8")}
    assert seen["family"] == {"gemm_kernel", "gemm_kernel_p3", "gemm_kernel_p5", "gemv_fused", "kx_row_stats_finalize",
                              "splitk_reduce_kernel", "splitk_reduce_rows_kernel"}
    # the row-owning reduce behind a KX_F16C main kernel (the batch-1 residual GEMMs in f16c), and KX_F16HL outputs: on the lean XPos
    # tile store, on the generic loops, and on the skinny shape where the split is withdrawn (no reduce kernel writes the pieces)
    def launches(name):
        return _golden_launches(GOLDEN["cases"][name])
    for name in ("decoder.out_proj/B1/f16c", "decoder.fc2/B1/f16c", "vit.out_proj/B1/f16c", "vit.fc2/B4/f16c", "rows_reduce/f16c/N8192"):
        main, red = launches(name)
        assert (main["kernel"], main["args"][0], red["kernel"]) == ("gemm_kernel", "f16c_t", "splitk_reduce_rows_kernel"), (name, main, red)
    hilo = {n: launches(n) for n in GOLDEN["cases"] if n.startswith("f16c/hilo/")}
    assert len(hilo) == 12 and all(len(v) == 1 for v in hilo.values())
    assert hilo["f16c/hilo/3648/t0"][0]["args"][2:4] == ["192", "8"] and hilo["f16c/hilo/4092/t512"][0]["args"][2:4] == ["256", "0"]
    assert hilo["f16c/hilo/114/t0"][0]["kernel"] == "gemm_kernel" and hilo["f16c/hilo/114/t0"][0]["grid"] == [192, 1]
    assert [r["grid"][1] for r in launches("splitk7/f16c/t64")[:1]] == [7] and len(launches("splitk1/bf16/t0")) == 1     # forced / off
    assert sum(n.startswith("f16c/corr/") for n in GOLDEN["cases"]) == 3 * (4 * 7 + 1)
    from kosmosx import _hip
    kinds = {_hip.KERNEL_KINDS[r["plan"]["kind"]] for r in described.values() if "plan" in r}
    assert kinds == {k for k in _hip.KERNEL_KINDS if k.startswith("gemm_")}


def _qkv_args(_hip):
    g = _hip.GemmArgs()
    g.A = g.W = g.C = g.bias = 1 << 20
    g.M, g.N, g.K, g.lda, g.ldw, g.ldc = 3648, 6144, 2048, 2048, 2048, 6144
    g.cdt, g.prec = _hip.KX_BF16, _hip.KX_PREC_BF16
    return g


def _describe(lib, g, cus=256):
    buf = C.create_string_buffer(4096)
    assert lib.kx_gemm_describe(C.byref(g), cus, buf, len(buf)) == 0
    return buf.value.decode()


def test_describing_twice_gives_the_same_text_and_a_tuning_value_changes_it(lib):
    from kosmosx import _hip
    g = _qkv_args(_hip)
    first = _describe(lib, g)
    assert first == _describe(lib, g)
    assert first.splitlines()[0] == "gemm_kernel_p5<bf16_t, 0, 192, 1, false, true> grid=256x1 block=512"
    assert first.splitlines()[-1].startswith("plan tile=384 kind=11 ") and len(first.splitlines()) == 2
    lib.kx_set_tuning(18, 1)                # the throughput objective: 256-row tiles where the rules chose 192-row ones
    try:
        changed = _describe(lib, g)
    finally:
        lib.kx_set_tuning(18, 0)
    assert changed.splitlines()[0] == "gemm_kernel_p5<bf16_t, 0, 256, 1, false, true> grid=256x1 block=512"
    assert _describe(lib, g) == first
    assert _describe(lib, g, cus=0) == first                 # no device here: the CU count defaults to 256
    assert "persistent=304" in _describe(lib, g, cus=304)    # the count is an input of the plan
    small = C.create_string_buffer(16)
    assert lib.kx_gemm_describe(C.byref(g), 256, small, len(small)) == 1 and "bytes" in _hip.last_error()


def test_refusals_carry_the_same_code_and_message_from_both_entry_points(lib):
    """The refusals tests/test_abi.py exercises on kx_gemm, and one of each later phase of the planner."""
    from kosmosx import _hip
    buf = C.create_string_buffer(4096)
    assert lib.kx_gemm(None, None) == 1
    msg = _hip.last_error()
    assert lib.kx_gemm_describe(None, 0, buf, len(buf)) == 1 and _hip.last_error() == msg and "null" in msg

    def both(g, code, needle):
        assert lib.kx_gemm(C.byref(g), None) == code
        m1 = _hip.last_error()
        assert lib.kx_gemm_describe(C.byref(g), 0, buf, len(buf)) == code
        assert _hip.last_error() == m1 and needle in m1, (m1, _hip.last_error())
    g = _hip.GemmArgs()
    g.A = g.W = g.C = 256
    g.M, g.N, g.K, g.lda, g.ldw, g.ldc = 4, 8, 100, 100, 100, 8
    both(g, 1, "multiple of")
    g = _hip.GemmArgs()
    g.A = g.W = g.C = g.row_stats = 256
    g.M, g.N, g.K, g.lda, g.ldw, g.ldc = 4, 64, 64, 64, 64, 64
    both(g, 1, "together")                                   # row_stats without colsum
    g = _qkv_args(_hip)
    g.tile = 1024
    both(g, 1, "pair split")                                 # the tile phase
    g.tile = 7
    both(g, 4, "unknown tile variant 7")                     # the instantiation phase: KX_ERR_UNSUPPORTED
    g.tile, g.ln_out = 0, 1 << 20
    both(g, 1, "split-K row reduce")                         # the split-K phase
