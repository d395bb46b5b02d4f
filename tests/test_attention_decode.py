"""decode_ref (the float64 reference of the decode-step attention) validated without a GPU.

1. The reference at position t equals row t of a causal full attention over the same t + 1 tokens — the lines of torchscale's
   MultiheadAttention.forward restated in tests/test_xpos_kat_gpu.py (_torchscale_attention): fp32 bmm, nan_to_num, mask,
   softmax, bmm — including one overflowing score and one NaN score.
2. The inputs the GPU tests use (tests/test_attention_decode_gpu.py) tell a right kernel from a wrong one: torch stand-ins that
   are wrong in one way each — key t read from the (poisoned) cache row, one slot's state dropped from the merge, the reload of a
   later round skipped — miss the bounds those tests assert."""
import pytest
import torch

import decode_ref as DR

BOUND = 2e-5                                                             # the GPU tests' parity bound


def _torchscale_attention(q, k, v):
    """bmm, nan_to_num, + mask, softmax, bmm in fp32 (q, k, v [B, T, H, 64]) -> [B, T, H*64]."""
    B, T, Hh, _ = q.shape
    a = torch.einsum("bihd,bmhd->bhim", q, k)
    a = torch.nan_to_num(a) + torch.triu(torch.full((T, T), float("-inf")), 1)
    return torch.einsum("bhim,bmhd->bihd", torch.softmax(a, -1), v).reshape(B, T, Hh * 64)


def _as_step(q, k, v, Tmax):
    """The last token of [B, T, H, 64] sequences as a decode step at t = T - 1: qkv row and caches (rows >= t poisoned)."""
    B, T, Hh, _ = q.shape
    t = T - 1
    qkv = torch.cat([x[:, t].reshape(B, Hh * 64) for x in (q, k, v)], 1)
    kc, vc = (torch.full((B, Hh, Tmax, 64), float("nan")) for _ in range(2))
    kc[:, :, :t], vc[:, :, :t] = k[:, :t].transpose(1, 2), v[:, :t].transpose(1, 2)
    return qkv, kc, vc, t


@pytest.mark.parametrize("t", [0, 1, 16, 69])
def test_reference_is_the_last_row_of_a_causal_full_attention(t):
    B, Hh, T = 2, 3, t + 1
    g = torch.Generator().manual_seed(100 + t)
    q, k, v = (torch.randn(B, T, Hh, 64, generator=g) for _ in range(3))
    q *= 0.35
    qkv, kc, vc, _ = _as_step(q, k, v, Tmax=t + 3)
    out, k2, v2 = DR.decode_attention_ref(qkv, kc, vc, t, nan_to_num=True)
    # float64 statement of the same lines: nothing but rounding of the last place between the two
    a = torch.einsum("bhd,bmhd->bhm", q[:, t].double(), k.double())
    full = torch.einsum("bhm,bmhd->bhd", torch.softmax(a, -1), v.double()).reshape(B, Hh * 64)
    assert DR.rel_err64(out, full) < 1e-13
    # the fp32 statement: fp32 rounding of at most 70 keys (plain fp32 torch sits at 2.3e-6 from float64 at 2048 keys)
    assert DR.rel_err64(_torchscale_attention(q, k, v)[:, t], out) < 5e-6
    # the append: row t holds the new k | v, the poison after it is still there, nothing before it moved
    D = Hh * 64
    assert torch.equal(k2[:, :, t].reshape(B, D), qkv[:, D:2 * D]) and torch.equal(v2[:, :, t].reshape(B, D), qkv[:, 2 * D:])
    keep = [j for j in range(t + 3) if j != t]
    assert torch.equal(DR.bits(k2[:, :, keep]), DR.bits(kc[:, :, keep])) and torch.equal(DR.bits(v2[:, :, keep]), DR.bits(vc[:, :, keep]))
    assert bool(torch.isnan(kc[:, :, t]).all())                          # the inputs were not touched


def test_reference_nan_to_num_on_an_overflowing_and_a_nan_score():
    T = 70
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(2, T, 1, 64, generator=g) for _ in range(3))
    q[0, T - 1, 0, 0] = 1e20
    k[0, 3, 0, 0] = 1e20                                                 # +inf in fp32 -> FLT_MAX: one-hot on key 3
    k[0, 9, 0, 0] = -1e20                                                # -inf -> -FLT_MAX: probability 0
    q[1], k[1] = q[1] * 0.05, k[1] * 0.05
    k[1, 30, 0, 7] = float("nan")                                        # a NaN score at small magnitude: counted as 0
    full = _torchscale_attention(q, k, v)[:, T - 1]
    assert bool(torch.isfinite(full).all())
    qkv, kc, vc, t = _as_step(q, k, v, Tmax=T)
    out, _, _ = DR.decode_attention_ref(qkv, kc, vc, t, nan_to_num=True)
    assert float((out[0] - v[0, 3, 0].double()).abs().max()) < 1e-12
    assert float((out - full.double()).abs().max()) < 2e-6
    p = DR.decode_weights(qkv, kc, t, nan_to_num=True)
    assert float(p[0, 0, 3]) == 1.0 and float(p[0, 0, 9]) == 0.0 and 0.9 / T < float(p[1, 0, 30]) < 1.1 / T
    # without nan_to_num the same inputs are not finite: the flag is what makes them so
    bad, _, _ = DR.decode_attention_ref(qkv, kc, vc, t, nan_to_num=False)
    assert not bool(torch.isfinite(bad[1]).all())


# ---- wrong stand-ins ---------------------------------------------------------------------------------------------------------
def _standin(qkv, kc, vc, t, fault, round_keys):
    """float64 softmax(K q) V over the keys a kernel with 16 interleaved slots (slot = j % 16) and rounds of `round_keys` keys
    would read, wrong in ONE way: 'cache_row_t' = key t from the cache row instead of the qkv row; 'drop_slot' = slot 7 left
    out of the merge; 'skip_reload' = later rounds compute on the first round's registers (key j -> key j % round_keys)."""
    B, Hh, _, _ = kc.shape
    q, kn, vn = (x.double() for x in DR.new_token(qkv, Hh))
    K = torch.cat([kc[:, :, :t].double(), kn[:, :, None]], 2)
    V = torch.cat([vc[:, :, :t].double(), vn[:, :, None]], 2)
    idx = torch.arange(t + 1)
    if fault == "cache_row_t":
        K[:, :, t], V[:, :, t] = kc[:, :, t].double(), vc[:, :, t].double()
    elif fault == "drop_slot":
        idx = idx[idx % 16 != 7]
    elif fault == "skip_reload":
        idx = idx % round_keys
    else:
        assert fault is None
    K, V = K[:, :, idx], V[:, :, idx]
    s = (K * q[:, :, None]).sum(-1)
    return (torch.softmax(s, -1)[..., None] * V).sum(2).reshape(B, Hh * 64)


@pytest.mark.parametrize("dtype,round_keys", [(torch.float32, 128), (torch.bfloat16, 256)], ids=["fp32", "bf16"])
def test_the_parity_inputs_tell_wrong_kernels_apart(dtype, round_keys):
    B, Hh, Tmax = 2, 3, 640
    for t in (0, 7, 17, 129, 257, 513):
        qkv, kc, vc = DR.random_step(B, Hh, Tmax, t, dtype, seed=t)
        ref, _, _ = DR.decode_attention_ref(qkv, kc, vc, t, nan_to_num=dtype == torch.float32)
        assert DR.rel_err64(_standin(qkv, kc, vc, t, None, round_keys), ref) < 1e-13
        # key t from the poisoned cache row: not finite (unpoisoned it would be the previous occupant: any value)
        assert not bool(torch.isfinite(_standin(qkv, kc, vc, t, "cache_row_t", round_keys)).any())
        if t >= 7:
            assert DR.rel_err64(_standin(qkv, kc, vc, t, "drop_slot", round_keys), ref) > 100 * BOUND, t
        if t >= round_keys:
            assert DR.rel_err64(_standin(qkv, kc, vc, t, "skip_reload", round_keys), ref) > 100 * BOUND, t


def test_a_spike_of_half_the_weight_tells_a_missed_rescale_from_a_right_one():
    """The GPU test's spike k_j = c q carries a softmax weight in [0.3, 0.7]: dropping the spike's slot, or the rest of the row,
    both move the output far beyond the bound.  With c = 40 (weight 1.0) a kernel that loses everything BUT the spike passes."""
    B, Hh, Tmax, t = 2, 3, 640, 600
    qkv, kc, vc = DR.random_step(B, Hh, Tmax, t, torch.float32, seed=3)
    q, _, _ = DR.new_token(qkv, Hh)
    for c in (None, 40.0):
        k2 = kc.clone()
        cc = DR.spike_scale(qkv, kc, t, 599) if c is None else torch.full((B, Hh), c, dtype=torch.float64)
        k2[:, :, 599] = (q.double() * cc[..., None]).float()
        w = DR.decode_weights(qkv, k2, t, True)[:, :, 599]
        ref, _, _ = DR.decode_attention_ref(qkv, k2, vc, t, True)
        only_spike = vc[:, :, 599].double().reshape(B, Hh * 64)          # every other key lost
        if c is None:
            assert bool(((w > 0.3) & (w < 0.7)).all())
            assert DR.rel_err64(only_spike, ref) > 100 * BOUND
            assert DR.rel_err64(_standin(qkv, k2, vc, t, "drop_slot", 128), ref) > 100 * BOUND       # 599 % 16 == 7
        else:
            assert float(w.min()) == 1.0 and DR.rel_err64(only_spike, ref) < 1e-12                 # a one-hot row sees nothing


@pytest.mark.parametrize("t", [1, 7])
def test_the_row_major_gather_case_tells_the_head_major_copy_apart(t):
    """tests/test_beam_step_gpu.py::test_kv_cache_gather_row_major_layout: a gather that copies rows 0:t of [L, B, heads, Tmax, 64]
    from memory that is laid out [L, B, Tmax, heads, 64] (what a gather that does not read tuning key 9 does) fails both of its
    assertions — wrong values in rows < t and writes at rows >= t — for every 0 < t < Tmax."""
    L, Bs, Bd, nh, Tmax = 2, 2, 6, 3, 10
    src = torch.randn((L, Bs, Tmax, nh, 64), generator=torch.Generator().manual_seed(t))
    dst = torch.full((L, Bd, Tmax, nh, 64), -3.0)
    idx = torch.tensor([1, 0, 0, 1, 1, 0])
    dst.view(L, Bd, nh, Tmax, 64)[:, :, :, :t] = src.view(L, Bs, nh, Tmax, 64).index_select(1, idx)[:, :, :, :t]
    assert not torch.equal(dst[:, :, :t], src.index_select(1, idx)[:, :, :t])
    assert not bool((dst[:, :, t:] == -3.0).all())
