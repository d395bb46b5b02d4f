"""attention_bwd_ref (the float64 reference of the attention backward and the checks built on it) validated without a GPU.

1. The reference is the definition: autograd through softmax(S) o M in float64.
2. A right kernel passes: `tiled_backward`, a restatement of the two-pass scheme the kernels follow, stays at or under HALF of
   every bound on every configuration, shape and input family tests/test_attention_backward_gpu.py launches — in float64 (what is
   left is the rounding of P and dS to bf16) and with float32 products and sums (that run fixes attention_bwd_ref.GAMMA).
3. Wrong kernels fail: each of MUTANTS, applied to the restatement, exceeds a bound on at least one of those inputs.
4. The pair probes see every pair and every mask bit: leaving one kept pair out of a sum, or flipping one keep bit, moves an
   element by more than two bounds."""
import functools

import numpy as np
import pytest
import torch

import attention_bwd_ref as BR
import train_ref as TR

NAMES = ["fp32", "bf16p/bf16", "valu-drop", "bf16-drop/bf16"]      # fp32-valu and the .../f32 twins share inputs and bounds with these
LOG2E = 1.4426950408889634
MUTANTS = ["dkv_drop_tile_last_query", "dq_drop_tile_last_key", "causal_strict", "clamp_dup", "dkv_causal_start_late",
           "dq_causal_end_early", "last_wave_block_skipped", "heads_swapped", "batch_swapped", "lse_without_log2e",
           "mask_transposed", "mask_aligned_only", "mask_missing_in_dP", "no_inv_keep", "buffer_parity"]
MASK_MUTANTS = ["mask_transposed", "mask_aligned_only", "mask_missing_in_dP", "no_inv_keep"]


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """The restatement is thousands of small matrix products: a thread pool only gets in their way."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ---- the two-pass scheme, restated ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _keep4(n_blocks, p, seed, site):
    """int64 [n_blocks]: bit r of entry b = the keep bit of element 4 b + r (one Philox block each)."""
    return (TR.keep_mask(4 * n_blocks, p, seed, site).reshape(n_blocks, 4).astype(np.int64) * np.array([1, 2, 4, 8])).sum(1)


def _tile_keep(Bc, Hc, T, rows, cols, mask, aligned_only):
    """bool [B, H, 64, 64]: the keep bits of mask rows `rows` x columns `cols` (64 positions each, the columns in sixteen groups of
    four that start at a multiple of four), drawn as the kernels draw them: ONE Philox block per row and group when T % 4 == 0,
    else the splice of the two blocks the group straddles.  `aligned_only` forgets the second block."""
    p, seed, site = mask
    k4 = _keep4((Bc * Hc * T * T) // 4 + 64, p, seed, site)
    bh = (np.arange(Bc)[:, None] * Hc + np.arange(Hc)[None, :])[:, :, None, None]
    idx = (bh * T + np.minimum(rows, T - 1)[None, None, :, None]) * T + cols[::4][None, None, None, :]        # [B, H, 64, 16]
    lo = k4[idx >> 2]
    four = lo if (T % 4 == 0 or aligned_only) else ((lo | (k4[(idx >> 2) + 1] << 4)) >> (idx & 3)) & 15
    return torch.from_numpy(((four[..., None] >> np.arange(4)) & 1).reshape(Bc, Hc, 64, 64).astype(bool))


def tiled_backward(q, k, v, dO, out, lse, causal, fmt, mask=None, mutant=None, arith=torch.float64):
    """-> (dq, dk, dv) [B, T, H, 64] float64 by the scheme of the kernels: delta = rowsum(dO o out) first; a dK/dV pass in which the
    owner of 64 keys (rows past T loaded from key T - 1, never written) walks the 64-query tiles (rows past T loaded as zeros and
    masked), from tile key0 / 64 when causal; a dQ pass in which the owner of 64 queries walks the key tiles, up to tile q0 / 64
    when causal; P = exp(S - lse) (with `fmt`: exp2(S log2e - lse log2e)), P o M and dS rounded to `fmt` (None / torch.bfloat16)
    before the second products; mask = (p, seed, site): keep bits drawn per block of four keys (_tile_keep).  `arith` is the
    dtype of every product and sum.  `mutant` makes it wrong in ONE way:
      dkv_drop_tile_last_query  the last query of every 64-query tile is masked in the dK/dV pass
      dq_drop_tile_last_key     the last key of every 64-key tile is masked in the dQ pass
      causal_strict             key < query instead of <=
      clamp_dup                 the streamed rows past T are loaded from row T - 1 and left unmasked: row T - 1 counts again
      dkv_causal_start_late     the causal dK/dV pass starts one tile late
      dq_causal_end_early       the causal dQ pass ends one tile early
      last_wave_block_skipped   the rows of the last 16-row block are never written (they stay NaN)
      heads_swapped, batch_swapped   heads / batch rows 0 and 1 of the three gradients change places
      lse_without_log2e         exp2(S log2e - lse): the statistic is not scaled
      mask_transposed           the dK/dV pass takes keep(key, query)
      mask_aligned_only         the block index ignores T % 4
      mask_missing_in_dP        dS = P (dPd - delta): the mask and its scale are not applied to dPd
      no_inv_keep               kept probabilities are not scaled by 1 / (1 - p)
      buffer_parity             the dK/dV pass reads, at every odd step, the tile data of the step before"""
    assert mutant is None or mutant in MUTANTS
    Bc, T, Hc, _ = q.shape
    hm = lambda x: x.to(arith).permute(0, 2, 1, 3)                                   # noqa: E731
    qh, kh, vh, gh = hm(q), hm(k), hm(v), hm(dO)
    delta = (gh * hm(out.reshape(Bc, T, Hc, 64))).sum(-1)                            # [B, H, T]
    lse = lse.to(arith)
    exp2 = fmt is not None or mutant == "lse_without_log2e"
    L = lse if not exp2 or mutant == "lse_without_log2e" else lse * LOG2E
    inv = 1.0
    if mask is not None and mutant != "no_inv_keep":
        inv = float(np.float32(1.0) / (np.float32(1.0) - np.float32(mask[0])))
    nt = (T + 63) // 64
    last = 16 * ((T - 1) // 16) if mutant == "last_wave_block_skipped" else T
    dup = mutant == "clamp_dup"
    rnd = (lambda x: x) if fmt is None else (lambda x: x.to(fmt).to(arith))
    zero = torch.zeros((), dtype=arith)

    def fixed(x, pos):                                     # the owner's rows: clamped to T - 1
        return x[:, :, pos.clamp(max=T - 1)]

    def streamed(x, pos):                                  # a streamed tile: zeros past T
        y = fixed(x, pos)
        if not dup:
            y = y * (pos < T).to(arith).reshape([1, 1, 64] + [1] * (y.dim() - 3))
        return y

    def probs(S, Lq):                                      # S [B, H, 64 q, 64 k], Lq [B, H, 64 q]
        return torch.exp2(S * LOG2E - Lq[..., None]) if exp2 else torch.exp(S - Lq[..., None])

    def valid(qpos, kpos, streamed_is_q):
        qv, kv = qpos < T, kpos < T
        if dup:
            qv, kv = (torch.ones_like(qv), kv) if streamed_is_q else (qv, torch.ones_like(kv))
        ok = qv[:, None] & kv[None, :]
        if causal:
            qc, kc = (qpos.clamp(max=T - 1), kpos.clamp(max=T - 1)) if dup else (qpos, kpos)
            ok = ok & ((kc[None, :] < qc[:, None]) if mutant == "causal_strict" else (kc[None, :] <= qc[:, None]))
        return ok

    def keep_scale(qpos, kpos, transposed=False):
        if mask is None:
            return None
        if transposed:
            bits = _tile_keep(Bc, Hc, T, kpos.numpy(), qpos.numpy(), mask, mutant == "mask_aligned_only").transpose(-1, -2)
        else:
            bits = _tile_keep(Bc, Hc, T, qpos.numpy(), kpos.numpy(), mask, mutant == "mask_aligned_only")
        return bits.to(arith) * inv

    def p_and_ds(S, dP, Lq, Dq, ok, km):
        pv = torch.where(ok, probs(S, Lq), zero)
        if km is None:
            return rnd(pv), rnd(pv * (dP - Dq[..., None]))
        return rnd(pv * km), rnd(pv * ((dP if mutant == "mask_missing_in_dP" else dP * km) - Dq[..., None]))

    grads = [torch.full((Bc, Hc, T, 64), float("nan"), dtype=torch.float64) for _ in range(3)]
    dq, dk, dv = grads
    for kt in range(nt):                                                             # ---- dK / dV: the owner of keys
        kpos = torch.arange(64 * kt, 64 * kt + 64)
        Kf, Vf = fixed(kh, kpos), fixed(vh, kpos)
        t0 = (kt + (1 if mutant == "dkv_causal_start_late" else 0)) if causal else 0
        aK, aV = torch.zeros(Bc, Hc, 64, 64, dtype=arith), torch.zeros(Bc, Hc, 64, 64, dtype=arith)
        for t in range(t0, nt):
            qpos = torch.arange(64 * t, 64 * t + 64)
            src = qpos - 64 if (mutant == "buffer_parity" and (t - t0) % 2 == 1) else qpos
            Qt, Gt, Lt, Dt = streamed(qh, src), streamed(gh, src), streamed(L, src), streamed(delta, src)
            ok = valid(qpos, kpos, True)
            if mutant == "dkv_drop_tile_last_query":
                ok = ok & (qpos % 64 != 63)[:, None]
            km = keep_scale(qpos, kpos, transposed=mutant == "mask_transposed")
            pb, sb = p_and_ds(Qt @ Kf.transpose(-1, -2), Gt @ Vf.transpose(-1, -2), Lt, Dt, ok, km)
            aV += pb.transpose(-1, -2) @ Gt
            aK += sb.transpose(-1, -2) @ Qt
        rows = kpos[kpos < last]
        dk[:, :, rows], dv[:, :, rows] = aK[:, :, : len(rows)].double(), aV[:, :, : len(rows)].double()
    for qt in range(nt):                                                             # ---- dQ: the owner of queries
        qpos = torch.arange(64 * qt, 64 * qt + 64)
        Qf, Gf, Lf, Df = fixed(qh, qpos), fixed(gh, qpos), fixed(L, qpos), fixed(delta, qpos)
        t_end = min(nt, qt + (0 if mutant == "dq_causal_end_early" else 1)) if causal else nt
        aQ = torch.zeros(Bc, Hc, 64, 64, dtype=arith)
        for t in range(t_end):
            kpos = torch.arange(64 * t, 64 * t + 64)
            Kt, Vt = streamed(kh, kpos), streamed(vh, kpos)
            ok = valid(qpos, kpos, False)
            if mutant == "dq_drop_tile_last_key":
                ok = ok & (kpos % 64 != 63)[None, :]
            _, sb = p_and_ds(Qf @ Kt.transpose(-1, -2), Gf @ Vt.transpose(-1, -2), Lf, Df, ok, keep_scale(qpos, kpos))
            aQ += sb @ Kt
        rows = qpos[qpos < last]
        dq[:, :, rows] = aQ[:, :, : len(rows)].double()
    if mutant == "heads_swapped" and Hc > 1:
        grads = [x[:, [1, 0] + list(range(2, Hc))] for x in grads]
    if mutant == "batch_swapped" and Bc > 1:
        grads = [x[[1, 0] + list(range(2, Bc))] for x in grads]
    return tuple(x.permute(0, 2, 1, 3).contiguous() for x in grads)


def _run(name, inputs, causal, p=0.0, mutant=None, arith=torch.float64):
    """The restatement on one case, handed the reference's fp32 out and lse as the kernels are."""
    q, k, v, dO, R = inputs[:5]
    mask = (p, BR.SEED, BR.SITE) if p else None
    return tiled_backward(q, k, v, dO, R.out.float(), R.lse.float(), causal, BR.CONFIGS[name].fmt, mask, mutant, arith)


def _inputs(name, family, causal):
    """[(what, case tuple, p)] of one family of a configuration: every shape, the (1, 9, 257) case and the spikes for random."""
    cfg = BR.CONFIGS[name]
    got = []
    for Bc, Hc, T, p in BR.shapes(name) + ([BR.wide_shape(name)] if family == "random" else []):
        got.append(((family, Bc, Hc, T, p), BR.case(family, Bc, Hc, T, cfg.values, causal, p), p))
    if family == "random" and cfg.entry == "plain":
        for i, spike in enumerate(BR.SPIKES):
            if spike[1] == causal:
                got.append((("spike",) + spike, BR.spike_case(cfg.values, i), 0.0))
    return got


# ---- 1. the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_the_reference_is_autograd_through_the_definition(p, causal):
    Bc, Hc, T = 2, 3, 37
    q, k, v, dO = BR.random_inputs(Bc, Hc, T, torch.float32, seed=5)
    M = BR.keep_scale(Bc, Hc, T, p)
    R = BR.Reference(q, k, v, dO, causal, M)
    leaves = [x.double().permute(0, 2, 1, 3).clone().requires_grad_() for x in (q, k, v)]
    s = leaves[0] @ leaves[1].transpose(-1, -2)
    if causal:
        s = s + torch.triu(torch.full((T, T), float("-inf"), dtype=torch.float64), 1)
    o = (torch.softmax(s, -1) * M) @ leaves[2]
    (o * dO.double().permute(0, 2, 1, 3)).sum().backward()
    assert float((R.out - o.detach().permute(0, 2, 1, 3).reshape(Bc, T, Hc * 64)).abs().max()) < 1e-13
    assert float((R.lse - torch.logsumexp(s.detach(), -1)).abs().max()) < 1e-13
    for x, leaf in zip((R.dq, R.dk, R.dv), leaves):
        assert float((x - leaf.grad.permute(0, 2, 1, 3)).abs().max()) < 1e-12
    if p:                                                                            # the mask is train_ref's, element by element
        keep = TR.keep_mask(Bc * Hc * T * T, p, BR.SEED, BR.SITE).reshape(Bc, Hc, T, T)
        assert 0.7 < keep.mean() < 0.8 and torch.equal(M > 0, torch.from_numpy(keep.astype(bool)))
        assert float(M.max()) == 1.0 / (1.0 - 0.25)
    # the bound of one element of dV, spelled out
    b, h, j, d = 1, 2, 4, 9
    r = sum(float(R.Pd[b, h, i, j]) * abs(float(dO[b, i, h, d])) for i in range(T))
    c = sum(float(R.Pd[b, h, i, j]) * (1 + float(q[b, i, h].double().abs() @ k[b, j, h].double().abs()) + abs(float(R.lse[b, h, i])))
            * abs(float(dO[b, i, h, d])) for i in range(T))
    want = (2 * 2.0 ** -9 * r) + (2 * 2.0 ** -9 * r) + BR.GAMMA * 2.0 ** -24 * c + 3e-5 * R.rms["dv"]
    assert abs(float(R.bound("bf16p/bf16", "dv")[b, j, h, d]) - want) < 1e-12 * want
    assert torch.equal(R.bound("fp32", "dv"), BR.GAMMA * 2.0 ** -24 * R.C["dv"] + 3e-5 * R.rms["dv"])    # u_p = 0: no rounding term


def test_the_probes_are_what_they_claim():
    """Every score 0, P = 1 / n_i, dK (A) and dQ (B) exactly zero with a bound of exactly zero, every value exact in bf16."""
    for causal in (True, False):
        for kind in ("A", "B"):
            q, k, v, dO, R = BR.case(kind, 2, 3, 131, torch.float32, causal, 0.25)
            for x in (q, k, v, dO):
                assert torch.equal(x.to(torch.bfloat16).float(), x)
            n = BR.visible(131, causal).sum(-1).double()
            assert float((R.P.sum(-1) - 1).abs().max()) < 1e-14
            assert float((R.P[0, 0] * n[:, None])[BR.visible(131, causal)].sub(1).abs().max()) < 1e-14
            z = "dk" if kind == "A" else "dq"
            assert float(getattr(R, z).abs().max()) == 0.0 and float(R.bound("bf16-drop/bf16", z).max()) == 0.0
            assert BR._grad_ratio("bf16-drop/bf16", z, torch.zeros(2, 131, 3, 64), R) == 0.0
            wrong = torch.zeros(2, 131, 3, 64)
            wrong[1, 130, 2, 63] = 1e-30
            assert BR._grad_ratio("bf16-drop/bf16", z, wrong, R) > 1e100


# ---- 2. a right kernel passes, with half of every bound to spare -----------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "unmasked"])
@pytest.mark.parametrize("family", ["random", "A", "B"])
@pytest.mark.parametrize("arith", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_stays_under_half_of_every_bound(name, arith, family, causal):
    """Condition: error / bound <= 0.5 for the unmutated restatement on every shape, the (1, 9, 257) case and the spikes.
    Worst ratios, float64 arithmetic: fp32 0.052 (random, unmasked T = 257, dV: out and lse are handed over in fp32), probes 0.027;
    valu-drop 0.062 (T = 1: 1 / (1 - p) in fp32); bf16p 0.486 (the spike (192, 191), dV), random 0.47 (causal T = 63, dK), probes 0.497
    (A, unmasked T = 128, dQ); bf16-drop random 0.465 (unmasked T = 63, dQ), probes 0.495 (A, causal T = 131, dQ).
    float32 arithmetic (what fixes GAMMA = 4; it needs 2.97): fp32 0.398 (random, unmasked T = 130, dK), spikes 0.344, probes 0.046;
    valu-drop 0.363 (random, causal T = 257, dV); the bf16 configurations as in float64 (the bf16 rounding is all there is).
    Against the bound without attention_bwd_ref's few-terms term the bf16 configurations sat at 0.88 .. 0.99: one rounding of one
    term reaches 2 u_p R exactly."""
    got = []
    for what, inputs, p in _inputs(name, family, causal):
        dq, dk, dv = _run(name, inputs, causal, p, arith=arith)
        got += BR.grad_ratios(name, dq, dk, dv, inputs[4], what)
    BR.verdict(got, f"restatement, {name} {family} {'causal' if causal else 'unmasked'} {arith}", limit=0.5)


# ---- 3. wrong kernels fail ------------------------------------------------------------------------------------------------
MUTANT_T = [130, 65, 5, 193, 64, 17, 257]            # tried in this order: the first shape at which a mutant shows ends its test


def _mutant_cases():
    for m in MUTANTS:
        for name in (NAMES[2:] if m in MASK_MUTANTS else NAMES):
            yield m, name


def _first_input_over(mutant, name, families):
    """The first of the listed inputs (shapes of MUTANT_T, in that order) on which the mutant exceeds a bound: (ratio, what), or None."""
    for family in families:
        for causal in (True, False):
            cases = [c for c in _inputs(name, family, causal) if c[0][0] != "spike" and c[0][3] in MUTANT_T]
            for what, inputs, p in sorted(cases, key=lambda c: MUTANT_T.index(c[0][3])):
                dq, dk, dv = _run(name, inputs, causal, p, mutant=mutant)
                worst = max(BR.grad_ratios(name, dq, dk, dv, inputs[4], what + (causal,)))
                if worst[0] > 1.0:
                    return worst
    return None


@pytest.mark.parametrize("families", [("random",), ("A", "B")], ids=["random", "probes"])
@pytest.mark.parametrize("mutant,name", list(_mutant_cases()))
def test_every_mutant_exceeds_a_bound(mutant, name, families):
    """... on the random inputs, and on the pair probes alone."""
    worst = _first_input_over(mutant, name, families)
    assert worst is not None, f"{mutant} passes every {name} check on {families}"
    print(f"{mutant}, {name}: error / bound {worst[0]:.3g} at {worst[1]}")
    with pytest.raises(AssertionError):                                              # ... and verdict turns that into a failure
        BR.verdict([worst], f"{mutant}, {name}")


# ---- 4. the probes see every pair and every bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "unmasked"])
@pytest.mark.parametrize("name", NAMES)
def test_the_probes_see_every_pair_and_every_mask_bit(name, causal):
    """EVERY (b, h, query, key) of every shape (not a sample): with one kept pair left out of a sum, or one keep bit flipped, the
    element the pair lands in is off by more than 2 bounds.  Allowed to stay invisible: no pair in dV; in dQ (probe A) and dK
    (probe B) without dropout at most 0.5 % of the pairs of rows that see two keys or more (a row of one key has dS = 0 by
    definition, and a pair whose dPd equals its row's mean has dS_ij = 0: nothing to see); no bit flip in dV, dQ or dK.
    Invisible pairs: causal 0.015 % (0.024 % with dropout), unmasked 0.001 %."""
    drop = BR.CONFIGS[name].entry != "plain"
    pairs = hidden = 0
    for Bc, Hc, T, p in BR.shapes(name):
        for kind in ("A", "B"):
            R = BR.case(kind, Bc, Hc, T, torch.float32, causal, p)[4]
            vis, kept, moves = BR.pair_visibility(name, kind, R, causal)
            assert bool((moves["dv"][kept] > 2).all()), (T, kind, "dv", float(moves["dv"][kept].min()))
            rows2 = kept & (vis.sum(-1) >= 2)[:, None]
            pairs += int(rows2.sum())
            hidden += int((moves["ds"][rows2] <= 2).sum())
            if drop:
                seen = vis.expand_as(kept)
                for x in ("dv_flip", "ds_flip"):
                    assert bool((moves[x][seen] > 2).all()), (T, kind, x, float(moves[x][seen].min()))
    print(f"pairs, {name} {'causal' if causal else 'unmasked'}: {hidden} of {pairs} invisible in dQ (A) / dK (B): {hidden / pairs:.3%}")
    assert hidden <= 0.005 * pairs, (hidden, pairs)               # (with dropout as well)
