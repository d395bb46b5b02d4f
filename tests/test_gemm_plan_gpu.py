"""What kx_gemm_describe says a call will launch is what the call launches: for six calls — each the smallest shape that still
takes its path — the in-process launch record (kx_prof_enable / kx_prof_collect) around ONE launch carries the KX_K_* kind and
the M, N, K the description names, and the description shows the path (pair split taken / not taken, row-owning reduce, 8-stage
ring, 192-row tiles)."""
import pytest
import torch

from kosmosx import _hip as H
from kosmosx import ops
from kosmosx.model import _operand_f16c

pytestmark = pytest.mark.gpu
DEV = "cuda"

#        name                  kind    M     N     K     what the description must show
CASES = [("pair_split_bf16", "bf16", 3584, 2048, 4096, dict(kernel="gemm_kernel_p5", pairk=1, args={2: "256", 4: "true"})),   # 14 x 8 tiles, 64 K-tiles
         ("pair_split_f16c", "f16c", 3584, 2048, 2048, dict(kernel="gemm_kernel_p5", pairk=1, args={2: "256", 4: "true"})),
         ("pair_not_taken_bf16", "bf16", 3584, 2048, 2048, dict(kernel="gemm_kernel_p3", pairk=0, args={2: "true"})),           # 32 K-tiles: too few
         ("splitk_row_reduce", "bf16", 114, 2048, 2048, dict(kernel="gemm_kernel", pairk=0, args={1: "64", 5: "4"}, reduce="splitk_reduce_rows_kernel")),
         ("ring8", "bf16", 114, 6144, 2048, dict(kernel="gemm_kernel", pairk=0, args={1: "64", 5: "8"})),                        # 192 tiles, one per CU
         ("tile_192", "bf16", 3648, 6144, 2048, dict(kernel="gemm_kernel_p5", pairk=0, args={2: "192", 4: "false"}))]


@pytest.mark.parametrize("name,kind,M,N,K,want", CASES, ids=[c[0] for c in CASES])
def test_the_launch_record_matches_the_description(name, kind, M, N, K, want):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.04).to(DEV)
    kw = dict(bias=torch.randn(N, generator=g).to(DEV), splitk_ws=torch.empty(32 << 20, dtype=torch.uint8, device=DEV))
    if name.startswith("pair"):
        kw.update(residual=torch.randn(M, N, generator=g).to(DEV), pair_ws=ops.pair_scratch())
    if name == "splitk_row_reduce":
        kw.update(residual=torch.randn(M, N, generator=g).to(DEV),
                  ln_out=(torch.ones(N, device=DEV), torch.zeros(N, device=DEV), 1e-5, torch.bfloat16))
    if kind == "f16c":
        fn, args = ops.gemm_f16c, (ops.pack_f16c_rows(x), _operand_f16c(w), N, K)
    else:
        fn, args = ops.gemm, (x.to(torch.bfloat16), w.to(torch.bfloat16))
    launches, plan = ops.gemm_describe(*args, **kw)
    main = [rec for rec in launches if rec["kernel"].startswith("gemm_kernel")]
    assert len(main) == 1 and main[0]["kernel"] == want["kernel"] and plan["pairk"] == want["pairk"], (launches, plan)
    assert all(main[0]["args"][i] == v for i, v in want["args"].items()), main[0]
    assert (launches[-1]["kernel"] == want["reduce"]) if "reduce" in want else (launches[-1] is main[0]), launches
    torch.cuda.synchronize()
    H.prof_enable(True)
    try:
        fn(*args, **kw)
        torch.cuda.synchronize()
        recs = [r for r in H.prof_collect() if r[0].startswith("gemm_")]
    finally:
        H.prof_enable(False)
    assert len(recs) == 1, recs
    assert recs[0][:4] == (H.KERNEL_KINDS[plan["kind"]], M, N, K), (recs, plan)
    assert ops.pair_split_errors() == 0
