"""kx_beam_step and kx_kv_cache_gather at kernel level against the CPU restatement (beam_ref): every batch row of every case is
replayed through beam_ref.step from the same state and compared under the rule of beam_ref.check_step."""
import numpy as np
import pytest
import torch

import beam_ref as BR
from kosmosx import _hip as H
from kosmosx import ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 2), (2, 1, 4, 8), (3, 4, 4, 502), (2, 8, 8, 1002), (1, 16, 16, 502), (1, 4, 4, 32002), (2, 2, 2, 64007)]
PAD = 1


def _gauss(B, Win, V, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B * Win, V)) * scale).astype(np.float32)
    s = np.zeros(B * Win, np.float32) if Win == 1 else -(rng.random(B * Win) * 8).astype(np.float32)
    return x, s


def _run(B, Win, W, V, g, x, s, pools=None, dones=None, eos=None, early=False, alpha=1.0, ld=None):
    """One launch of the step on the device -> per batch row dict(token, parent, score, pool, done) as numpy, and src_row."""
    dev = "cuda"
    ld = V if ld is None else ld
    buf = torch.full((B * Win, ld), 7.0, dtype=torch.float32)               # the columns past V are never read
    buf[:, :V] = torch.from_numpy(x)
    logits = buf.to(dev)[:, :V]
    pools = pools or [[] for _ in range(B)]
    ps = torch.full((B, W), float("-inf"))
    pe, pp, pc = torch.zeros((B, W), dtype=torch.int32), torch.zeros((B, W), dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b, pool in enumerate(pools):
        pc[b] = len(pool)
        for k, p in enumerate(pool):
            ps[b, k], pe[b, k], pp[b, k] = p["score"], p["end"], p["parent"]
    pool = tuple(t.to(dev) for t in (ps, pe, pp, pc))
    done = torch.tensor([int(d) for d in (dones or [False] * B)], dtype=torch.uint8, device=dev)
    out = dict(scores_out=torch.full((B * W,), 99.0, device=dev), next_token=torch.full((B * W,), -7, dtype=torch.int64, device=dev),
               parent=torch.full((B * W,), -7, dtype=torch.int32, device=dev), src_row=torch.full((B * W,), -7, dtype=torch.int32, device=dev))
    scratch = torch.empty(B * Win * 2 * W, dtype=torch.int64, device=dev)
    ops.beam_step(logits, torch.from_numpy(s).to(dev), num_beams=W, step=g, pool=pool, done=done, scratch=scratch,
                  length_penalty=alpha, early_stopping=early, eos_token_id=eos, pad_token_id=PAD, **out)
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy().reshape(B, W) for k, v in out.items()}
    pl = [t.cpu().numpy() for t in pool]
    dn = done.cpu().numpy()
    rows = [dict(token=o["next_token"][b], parent=o["parent"][b], score=o["scores_out"][b], done=dn[b],
                 pool=(pl[0][b], pl[1][b], pl[2][b], pl[3][b])) for b in range(B)]
    assert (o["src_row"] == np.arange(B)[:, None] * Win + o["parent"]).all()                 # what the cache gather reads
    raw = [o["next_token"], o["parent"], o["scores_out"], o["src_row"], *pl, dn]
    return rows, raw


def _ref(B, Win, W, V, g, x, s, pools=None, dones=None, eos=None, early=False, alpha=1.0):
    pools = pools or [[] for _ in range(B)]
    dones = dones or [False] * B
    return [BR.step(x[b * Win:(b + 1) * Win], s[b * Win:(b + 1) * Win], pools[b], g, W=W, eos=eos, pad=PAD, alpha=alpha, early=early,
                    done=dones[b]) for b in range(B)]


def _check(B, Win, W, V, g, x, s, **kw):
    ld = kw.pop("ld", None)
    got, raw = _run(B, Win, W, V, g, x, s, ld=ld, **kw)
    ref = _ref(B, Win, W, V, g, x, s, **kw)
    tally = BR.Tally()
    for b in range(B):
        BR.check_step(got[b], ref[b], tally, msg=f"row {b}")
    tally.check()
    return got, ref, raw


@pytest.mark.parametrize("B,Win,W,V", SHAPES)
def test_step_against_the_reference(B, Win, W, V):
    g = 0 if Win == 1 else 5
    x, s = _gauss(B, Win, V, seed=V + W)
    ld = V + 5 if V == 502 and W == 4 else V
    _, ref, raw = _check(B, Win, W, V, g, x, s, ld=ld, alpha=0.8)
    assert all(np.isfinite(r["score"]).all() for r in ref)                  # V >= 2W finite candidates: every slot is filled
    # EOS = the reference's best token of row 0: it enters the pool
    eos = int(ref[0]["token"][0])
    _, ref2, raw2 = _check(B, Win, W, V, g, x, s, ld=ld, eos=eos, alpha=0.8)
    assert len(ref2[0]["pool"]) >= 1 and eos not in ref2[0]["token"]
    # two runs, bit for bit (scores compared as bits)
    _, raw3 = _run(B, Win, W, V, g, x, s, ld=ld, eos=eos, alpha=0.8)
    for a, b in zip(raw2, raw3):
        assert a.tobytes() == b.tobytes()


def test_non_finite_logits_and_dead_beams():
    B, Win, W, V, g = 3, 4, 4, 502, 2
    x, s = _gauss(B, Win, V, seed=1)
    x[0, ::3] = -np.inf
    x[1, 5:400] = np.nan
    x[2, :] = -np.inf                                                       # a row with no candidate at all
    x[3, 7] = np.inf                                                        # clamped to FLT_MAX: lse = FLT_MAX, its lp = 0
    x[5, 100] = -0.0
    s[6] = -np.inf                                                          # one input beam at -inf: offers nothing
    x[8:12, :] = np.nan
    x[8, 3], x[8, 9], x[9, 4] = 0.5, 0.25, 1.0                              # batch row 2: three finite candidates in all
    s[3] = -0.5
    got, ref, _ = _check(B, Win, W, V, g, x, s)
    assert (3, 7) in list(zip(ref[0]["parent"], ref[0]["token"]))           # the +inf entry is a candidate at c = s_j
    assert 2 not in ref[0]["parent"] and 2 not in ref[1]["parent"]          # the empty row and the dead beam parent nothing
    assert ref[2]["token"][3] == PAD and ref[2]["score"][3] == -np.inf and ref[2]["parent"][3] == 3   # an unfilled slot
    for b in range(B):
        assert [int(t) for t in got[b]["token"]] == ref[b]["token"]
        for p, t, c in zip(got[b]["parent"], got[b]["token"], got[b]["score"]):
            if c > -np.inf:                                                 # nothing NaN or -inf was selected
                assert x[b * Win + p, t] > -np.inf


@pytest.mark.parametrize("Win,W,V", [(1, 4, 8), (4, 4, 502), (2, 2, 64007)])
def test_all_equal_logits_select_the_lowest_flat_indices(Win, W, V):
    """Equal logits and equal input scores: every candidate ties exactly, the best 2W are flat indices 0 .. 2W-1 — equality."""
    B = 2
    x = np.full((B * Win, V), 0.5, np.float32)
    s = np.full(B * Win, -1.25 if Win > 1 else 0.0, np.float32)
    got, _ = _run(B, Win, W, V, 0 if Win == 1 else 3, x, s)
    for b in range(B):
        assert list(got[b]["token"]) == list(range(W)) and list(got[b]["parent"]) == [0] * W
        assert len(set(got[b]["score"].tolist())) == 1
        assert abs(float(got[b]["score"][0]) - (float(s[0]) - np.log(V))) <= BR.EPS_S
    # with EOS = token 1: flat index 1 enters the pool (rank 1 < W), the live beams are 0, 2, 3, ...
    got, _ = _run(B, Win, W, V, 0 if Win == 1 else 3, x, s, eos=1)
    for b in range(B):
        assert list(got[b]["token"]) == [0] + list(range(2, W + 1)) and int(got[b]["pool"][3]) == 1
        assert (int(got[b]["pool"][1][0]), int(got[b]["pool"][2][0])) == (0 if Win == 1 else 3, 0)


def _ranking(x, s, W, V):
    """Flat candidates of one batch row, best first (reference order)."""
    c = np.stack([s[j] + BR.log_softmax_row(x[j]) for j in range(x.shape[0])]).ravel()
    return [divmod(int(i), V) for i in np.argsort(-c, kind="stable")[: 2 * W]]


def test_eos_inside_and_outside_the_first_w():
    B, Win, W, V, g = 2, 4, 4, 502, 4
    x, s = _gauss(B, Win, V, seed=2)
    rank = _ranking(x[:Win], s[:Win], W, V)
    inside = rank[1][1]
    _, ref, _ = _check(B, Win, W, V, g, x, s, eos=inside, alpha=1.3)
    assert [p["end"] for p in ref[0]["pool"]][:1] == [g] and ref[0]["pool"][0]["parent"] == rank[1][0]
    outside = None
    for j, v in rank[W:]:                                                   # a token whose only top-2W appearance is at rank >= W
        if all(v != v2 for _, v2 in rank[:W]) and sum(v == v2 for _, v2 in rank) == 1:
            outside = v
            break
    assert outside is not None
    got, ref, _ = _check(B, Win, W, V, g, x, s, eos=outside, alpha=1.3)
    assert ref[0]["pool"] == [] and int(got[0]["pool"][3]) == 0            # skipped: the pool is unchanged
    assert outside not in ref[0]["token"]


@pytest.mark.parametrize("early", [False, True])
def test_full_pool_replacement_done_and_frozen_rows(early):
    B, Win, W, V, g = 3, 4, 4, 502, 6
    x, s = _gauss(B, Win, V, seed=3)
    eos = _ranking(x[:Win], s[:Win], W, V)[0][1]                            # row 0's best candidate is an EOS
    x[Win:2 * Win] = x[:Win]                                                # rows 0 and 1 rank the same candidates
    s[Win:2 * Win] = s[:Win]
    low = [dict(score=-50.0 - k, end=1, parent=k) for k in range(W)]        # any newcomer is better
    high = [dict(score=-0.001 * (k + 1), end=1, parent=k) for k in range(W)]   # no newcomer is
    three = high[:W - 1]
    got, ref, _ = _check(B, Win, W, V, g, x, s, eos=eos, early=early, pools=[low, high, three], alpha=1.0)
    assert [p["end"] for p in ref[0]["pool"]].count(g) >= 1 and ref[0]["pool"][W - 1]["end"] == g      # the worst (last) was replaced
    assert ref[1]["pool"] == high                                           # a worse newcomer changes nothing
    assert ref[0]["done"] == early                                          # low pool: a live beam can still beat it
    assert ref[1]["done"] is True                                           # high pool: nothing live can
    assert [bool(r["done"]) for r in got] == [r["done"] for r in ref]
    # the next step: the done rows are frozen — pool, scores kept; pad; identity
    dones = [r["done"] for r in ref]
    pools = [r["pool"] for r in ref]
    s2 = np.concatenate([np.asarray(r["score"], np.float32) for r in ref])
    got2, ref2, _ = _check(B, Win, W, V, g + 1, x, s2, eos=eos, early=early, pools=pools, dones=dones, alpha=1.0)
    b = 1
    assert list(got2[b]["token"]) == [PAD] * W and list(got2[b]["parent"]) == list(range(W))
    assert got2[b]["score"].tobytes() == s2[b * W:(b + 1) * W].tobytes() and bool(got2[b]["done"])
    BR.check_pool(got2[b]["pool"], pools[b])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("t", [0, 1, 7, 10])
def test_kv_cache_gather(dtype, t):
    L, Bs, Bd, nh, Tmax = 2, 2, 6, 3, 10
    g = torch.Generator().manual_seed(t)
    sk, sv = (torch.randn((L, Bs, nh, Tmax, 64), generator=g).to(dtype).cuda() for _ in range(2))
    dk, dv = (torch.full((L, Bd, nh, Tmax, 64), -3.0, dtype=dtype, device="cuda") for _ in range(2))
    idx = torch.tensor([1, 0, 0, 1, 1, 0], dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.kv_cache_gather(sk, sv, dk, dv, t, idx, err)
    for src, dst in ((sk, dk), (sv, dv)):
        assert torch.equal(dst[:, :, :, :t], src.index_select(1, idx.long())[:, :, :, :t])
        assert bool((dst[:, :, :, t:] == -3.0).all())                       # rows at and after t are not written
    assert int(err.item()) == 0
    # an out-of-range source row copies nothing for that row and raises the sticky bit
    dk.fill_(-3.0), dv.fill_(-3.0)
    bad = torch.tensor([1, 2, 0, -1, 1, 0], dtype=torch.int32, device="cuda")
    ops.kv_cache_gather(sk, sv, dk, dv, t, bad, err)
    ok = [0, 2, 4, 5]
    for src, dst in ((sk, dk), (sv, dv)):
        assert torch.equal(dst[:, ok, :, :t], src.index_select(1, bad[ok].long())[:, :, :, :t])
        assert bool((dst[:, [1, 3]] == -3.0).all()) and bool((dst[:, :, :, t:] == -3.0).all())
    assert int(err.item()) == (H.KX_RAGGED_ERR_GATHER if t > 0 else 0)
    # overlapping buffers: an error code, nothing launched
    whole = torch.full((2, L, Bd, nh, Tmax, 64), -3.0, dtype=dtype, device="cuda")
    with pytest.raises(RuntimeError, match="overlap"):
        ops.kv_cache_gather(whole[0], whole[1], whole[0], whole[1], t, idx, err)           # in place
    with pytest.raises(RuntimeError, match="overlap"):
        ops.kv_cache_gather(sk, sv, whole[0], whole[0], t, idx, err)                       # dst_k is dst_v
    assert bool((whole == -3.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("t", [0, 1, 7, 10])
def test_kv_cache_gather_row_major_layout(dtype, t):
    """Tuning key 9 = 1: the caches are [L, B, Tmax, heads, 64] and dst[l, r, :t] = src[l, src_row[r], :t] — the first t rows of
    heads * 64 elements per (layer, sequence).  (Copying rows 0:t of [L, B, heads, Tmax, 64] there moves the wrong memory.)
    Distinct values everywhere in src, so a row taken from another head, position or sequence shows."""
    L, Bs, Bd, nh, Tmax = 2, 2, 6, 3, 10
    g = torch.Generator().manual_seed(t)
    sk, sv = (torch.randn((L, Bs, Tmax, nh, 64), generator=g).to(dtype).cuda() for _ in range(2))
    dk, dv = (torch.full((L, Bd, Tmax, nh, 64), -3.0, dtype=dtype, device="cuda") for _ in range(2))
    idx = torch.tensor([1, 0, 0, 1, 1, 0], dtype=torch.int32, device="cuda")
    bad = torch.tensor([1, 2, 0, -1, 1, 0], dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = H.load()
    lib.kx_set_tuning(9, 1)
    try:
        ops.kv_cache_gather(sk, sv, dk, dv, t, idx, err, layout="row_major")
        for src, dst in ((sk, dk), (sv, dv)):
            assert torch.equal(dst[:, :, :t], src.index_select(1, idx.long())[:, :, :t])
            assert bool((dst[:, :, t:] == -3.0).all())                      # rows at and after t are not written
        assert int(err.item()) == 0
        # an out-of-range source row copies nothing for that row and raises the sticky bit
        dk.fill_(-3.0), dv.fill_(-3.0)
        ops.kv_cache_gather(sk, sv, dk, dv, t, bad, err, layout="row_major")
        ok = [0, 2, 4, 5]
        for src, dst in ((sk, dk), (sv, dv)):
            assert torch.equal(dst[:, ok, :t], src.index_select(1, bad[ok].long())[:, :, :t])
            assert bool((dst[:, [1, 3]] == -3.0).all()) and bool((dst[:, :, t:] == -3.0).all())
        assert int(err.item()) == (H.KX_RAGGED_ERR_GATHER if t > 0 else 0)
        # overlapping buffers: an error code, nothing launched
        whole = torch.full((2, L, Bd, Tmax, nh, 64), -3.0, dtype=dtype, device="cuda")
        with pytest.raises(RuntimeError, match="overlap"):
            ops.kv_cache_gather(whole[0], whole[1], whole[0], whole[1], t, idx, err, layout="row_major")
        assert bool((whole == -3.0).all())
    finally:
        lib.kx_set_tuning(9, 0)
