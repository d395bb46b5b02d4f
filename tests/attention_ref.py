"""CPU reference of the forward attention (kx_attention in include/kosmosx_hip.h), torch / float64, and the checks the CPU and GPU
tests of it share (tests/test_attention_ref.py, tests/test_attention_forward_gpu.py).

Test infrastructure, written from the kx_attn_args contract, not from the kernels.  Per (batch row, head):
  q [B, Tq, H, 64] arrives pre-scaled, k / v [B, Tk, H, 64]; score = <q_i, k_j>; KX_ATTN_CAUSAL (Tq == Tk) keeps key <= query;
  softmax over the kept keys; out [B, Tq, H*64] = P V; lse [B, H, Tq] = the log-sum-exp of the kept scores.
The reference knows nothing of tiles, blocks or the order of the sums.  `tiled_attention` below is the opposite: a float64
restatement of the flash scheme the kernels follow, there to show that the bounds accept a right kernel and that each of the
listed mistakes (MUTANTS) misses them.

Bounds (none is fitted to what a kernel returns):
  probe   |out - ref| <= 2^-21 |ref| + 1e-30 per element: 8 fp32 ulps for the one division (or reciprocal and multiply) that is
          left when every P is exactly 1 and every sum an integer below 2^24.
  parity  |out - ref| <= 2 u_p (P |V|) + 2 u_p (P |V|) + floor per element.  u_p belongs to the format P is rounded to before P V
          (bf16: 2^-9, fp16: 2^-12, the fp32 kernels: 0); the factor 2 of the first term covers the normaliser, summed from the
          rounded P or from the exact one.  The second term is the binade term: u_p is half a spacing of the values in [1/2, 1),
          so a rounded p in [2^-e-1, 2^-e) is off by up to u_p 2^-e, which is u_p p only at the top of the binade and 2 u_p p at
          its bottom (bf16 keeps 8 significant bits: relative error up to 2^-8 = 2 u_p; fp16 11: 2^-11).  The online softmax
          scales every p by factors that are no powers of two, so where in its binade a p was rounded is not known from the
          contract: with p~_j = p_j (1 + d_j), |d_j| <= 2 u_p, and out = sum p~ v / sum p~, the error is sum_j P_j d_j (v_j - out)
          to first order, at most 2 u_p (P |V| + |out|) <= 4 u_p (P |V|).  Without the term a right kernel sits at 0.75 (bf16) and
          0.63 (fp16) of the bound (test_attention_ref.py: the float64 restatement; the kernels measure the same on an MI355X),
          over the half that a right kernel must stay under; rows that lean on a few keys do not average one rounding down.
          floor = 2e-5 x the rms of the reference (the project's fp32-attention bound, test_ops_gpu.py::test_attention_f32), for
          fp16 plus Tk 2^-25 max|V|: a probability below 2^-14 is a subnormal fp16 number and is off by up to 2^-25 absolute,
          once per key.  f16c: floor = 3e-6 max(1, max|ref|), the bound of test_f16c_gpu.py::test_attention_f16c_split_products,
          held per element with u_p = 0 (P and V travel as two fp16 pieces there: 22 bits, fp32 class).
  lse     |lse - ref| <= 2 u_p + 1e-5 max(1, |ref|) (1e-5: the fp32 bound of test_grad_ops_gpu.py::test_attention_backward).
"""
from __future__ import annotations

import functools

import torch

from decode_ref import bits, rel_err64  # noqa: F401  (re-exported: the tests take them from here)

# name -> (dtype of q / k / v, format P is rounded to before P V, u_p of the parity bound)
CONFIGS = {
    "bf16": (torch.bfloat16, torch.bfloat16, 2.0 ** -9),
    "fp16": (torch.float16, torch.float16, 2.0 ** -12),
    "f16c": (torch.float32, None, 0.0),
    "fp32": (torch.float32, None, 0.0),
    "fp32-valu": (torch.float32, None, 0.0),
    "bf16-v1": (torch.bfloat16, torch.bfloat16, 2.0 ** -9),
}
CAUSAL_T = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 640, 1025]
FULL_TQ_TK = [(1, 1), (1, 321), (64, 321), (65, 64), (128, 63), (129, 257), (257, 257), (33, 1025), (385, 130)]


def shapes(causal):
    """(Tq, Tk) of every shape of a mask."""
    return [(t, t) for t in CAUSAL_T] if causal else list(FULL_TQ_TK)


def _heads_major(x):
    return x.double().permute(0, 2, 1, 3)


def attention_ref(q, k, v, causal):
    """-> (out [B, Tq, H*64], lse [B, H, Tq], P [B, H, Tq, Tk]), float64, on the VALUES of q, k, v (round them first)."""
    B, Tq, H, hd = q.shape
    Tk = k.shape[1]
    assert hd == 64 and tuple(k.shape) == (B, Tk, H, 64) and k.shape == v.shape and (not causal or Tq == Tk)
    qh, kh, vh = _heads_major(q), _heads_major(k), _heads_major(v)
    s = qh @ kh.transpose(-1, -2)
    if causal:
        keep = torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None]
        s = s.masked_fill(~keep, float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    out = (P @ vh).permute(0, 2, 1, 3).reshape(B, Tq, H * 64)
    return out, lse, P


def abs_pv(P, v):
    """P |V| in the layout of the output: [B, Tq, H*64]."""
    B, H, Tq, _ = P.shape
    return (P @ _heads_major(v).abs()).permute(0, 2, 1, 3).reshape(B, Tq, H * 64)


def elem_bound(P, v, u_p, floor):
    """The parity bound per output element: 2 u_p (P |V|) + floor."""
    return 2.0 * u_p * abs_pv(P, v) + floor


def binade_term(apv, u_p):
    """2 u_p (P |V|): a P rounded at the bottom of its binade is off by 2 u_p of itself (module docstring)."""
    return 2.0 * u_p * apv


class Reference:
    """What the checks need of one input: out, lse, P |V| (P itself is dropped: T^2 values), the floor terms."""

    def __init__(self, q, k, v, causal):
        self.out, self.lse, P = attention_ref(q, k, v, causal)
        self.apv = abs_pv(P, v)
        self.Tk = k.shape[1]
        self.vmax = float(v.double().abs().max())
        self.rms = float(self.out.pow(2).mean().sqrt())
        self.omax = float(self.out.abs().max())

    def parity_bound(self, name):
        _, _, u_p = CONFIGS[name]
        if name == "f16c":
            floor = 3e-6 * max(1.0, self.omax)
        else:
            floor = 2e-5 * self.rms
            if name == "fp16":
                floor += self.Tk * 2.0 ** -25 * self.vmax
        return 2.0 * u_p * self.apv + binade_term(self.apv, u_p) + floor

    def lse_bound(self, name):
        return 2.0 * CONFIGS[name][2] + 1e-5 * self.lse.abs().clamp(min=1.0)


# ---- the shared checks: every comparison of the CPU and the GPU file goes through these -------------------------------------
def _ratio(got, want, bound):
    got = got.detach().double().cpu()
    if got.shape != want.shape or not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - want).abs() / bound).max())


def probe_ratio(out, R):
    return _ratio(out, R.out, 2.0 ** -21 * R.out.abs() + 1e-30)


def parity_ratio(name, out, R):
    return _ratio(out, R.out, R.parity_bound(name))


def lse_ratio(name, lse, R):
    return _ratio(lse, R.lse, R.lse_bound(name))


def verdict(got, label, limit=1.0):
    """got = [(error / bound, what)] of one test: print the worst, then fail on any above `limit` (not finite = inf)."""
    worst = max(got, key=lambda x: x[0])
    print(f"{label}: worst error / bound {worst[0]:.3g} at {worst[1]} of {len(got)}")
    over = [(float(f"{r:.3g}"), w) for r, w in got if not r <= limit]
    assert not over, (label, over)
    return worst


# ---- inputs -------------------------------------------------------------------------------------------------------------
def random_qkv(B, H, Tq, Tk, dtype, seed, q_scale=0.35):
    """q = randn * q_scale [B, Tq, H, 64], k and v = randn [B, Tk, H, 64] in `dtype`, different for every (b, h)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Tq, H, 64, generator=g) * q_scale
    k, v = torch.randn(B, Tk, H, 64, generator=g), torch.randn(B, Tk, H, 64, generator=g)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def probe_qkv(B, H, Tq, Tk, dtype, seed):
    """q = 0, k random, v = random integers in [-4, 4] (exact in bf16, fp16, fp32 and in both fp16 pieces of the f16c split, also
    scaled by 2^8): every score is 0, every P exactly 1, and a row of the output is the mean of the value rows its query sees."""
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(B, Tq, H, 64)
    k = torch.randn(B, Tk, H, 64, generator=g)
    v = torch.randint(-4, 5, (B, Tk, H, 64), generator=g).float()
    return q.to(dtype), k.to(dtype), v.to(dtype)


def probe_means(v, Tq, causal):
    """The probe's reference rows [B, Tq, H*64]: integer sums of the value rows a query sees (exact in float64) over their count,
    one correctly rounded division per element."""
    B, Tk, H, _ = v.shape
    x = v.double().reshape(B, Tk, H * 64)
    if causal:
        return x.cumsum(1) / torch.arange(1, Tk + 1, dtype=torch.float64)[None, :, None]
    return (x.sum(1, keepdim=True) / Tk).expand(B, Tq, H * 64).clone()


def plant_spike(q, k, b, h, query, key, causal=True):
    """k[b, key, h] = c q[b, query, h] IN PLACE (after decode_ref.spike_scale: c |q|^2 = the log-sum-exp of the query's other
    scores, so the key holds about half of the softmax weight), rounded to k's dtype before anything is measured.  Returns the
    weight the rounded key holds: a one-hot row could not tell a missed rescale from a right one."""
    n = query + 1 if causal else k.shape[1]
    assert 0 <= key < n
    qq = q[b, query, h].double()
    s = k[b, :n, h].double() @ qq
    s[key] = float("-inf")
    c = torch.logsumexp(s, 0) / qq.pow(2).sum()
    k[b, key, h] = (c * qq).to(k.dtype)
    s[key] = k[b, key, h].double() @ qq
    return float(torch.softmax(s, 0)[key])


@functools.lru_cache(maxsize=None)
def case(kind, B, H, Tq, Tk, dtype, causal):
    """(q, k, v, Reference) of the probe / parity inputs of one shape, built once and shared: treat them as read-only."""
    build = {"probe": probe_qkv, "random": random_qkv}[kind]
    q, k, v = build(B, H, Tq, Tk, dtype, seed=(7 if kind == "probe" else 11) * 100003 + Tq * 2053 + Tk + 5 * H)
    R = Reference(q, k, v, causal)
    if kind == "probe":                             # the exact rows (the float64 softmax leaves 1e-16 where the mean is 0)
        exact = probe_means(v, Tq, causal)
        assert float((R.out - exact).abs().max()) < 1e-13
        R.out = exact
    return q, k, v, R


# (Tq, Tk, causal, query, key).  Causal T = 640 is nx = 5: pairs (0, 4) and (1, 3), block 2 alone — a key of the second pass's first
# tile, of its diagonal tile, of the middle block, and a first-pass key at a tile start; unmasked: the last key of a ragged last tile
# for the one query of the last block.
SPIKES = [(640, 640, True, 600, 5), (640, 640, True, 600, 590), (640, 640, True, 300, 130), (640, 640, True, 70, 64),
          (129, 321, False, 128, 320)]


@functools.lru_cache(maxsize=None)
def spike_case(dtype, i, B=2, H=3):
    """(q, k, v, Reference, weights) of SPIKES[i]: random inputs with the spike planted in every (b, h); read-only."""
    Tq, Tk, causal, query, key = SPIKES[i]
    q, k, v = random_qkv(B, H, Tq, Tk, dtype, seed=900 + i)
    w = [plant_spike(q, k, b, h, query, key, causal) for b in range(B) for h in range(H)]
    return q, k, v, Reference(q, k, v, causal), w


# ---- the flash scheme, restated in float64 -------------------------------------------------------------------------------
MUTANTS = ["drop_tile_last_key", "causal_strict", "clamp_dup", "second_pass_same_block", "skip_middle", "no_rescale",
           "heads_swapped", "batch_swapped", "max_reset"]


def tiled_attention(q, k, v, causal, p_fmt, mutant=None):
    """-> (out [B, Tq, H*64], lse [B, H, Tq]) float64 by the scheme of the matrix-core kernels: 128-query blocks, 64-key tiles
    whose rows past Tk are loaded from key Tk - 1 and masked, online softmax (running maximum m, P = exp(s - m) rounded to `p_fmt`
    (torch.bfloat16 / torch.float16 / None), l summed from the rounded P, O and l rescaled when m moves), causal launches
    walking the block pairs (x, nx-1-x) with the tiles above a block's diagonal never visited.  `mutant` makes it wrong in ONE way:
      drop_tile_last_key      the last key of every 64-key tile is masked
      causal_strict           key < query instead of <=
      clamp_dup               the row after the last key (loaded from key Tk - 1) is left unmasked: key Tk - 1 counts twice
      second_pass_same_block  the second pass of a pair runs block x again: block nx-1-x is never written
      skip_middle             the unpaired middle block of an odd nx >= 3 is skipped
      no_rescale              O and l are not rescaled when the maximum moves
      heads_swapped           heads 0 and 1 of the output change places
      batch_swapped           batch rows 0 and 1 of the output change places
      max_reset               the running maximum starts from -inf in every tile"""
    assert mutant is None or mutant in MUTANTS
    B, Tq, H, _ = q.shape
    Tk = k.shape[1]
    qh, kh, vh = _heads_major(q), _heads_major(k), _heads_major(v)
    out = torch.full((B, H, Tq, 64), float("nan"), dtype=torch.float64)
    lse = torch.full((B, H, Tq), float("nan"), dtype=torch.float64)
    nx, ntk = (Tq + 127) // 128, (Tk + 63) // 64
    if causal:
        schedule = [[y] + ([nx - 1 - y] if nx - 1 - y > y else []) for y in range((nx + 1) // 2)]
    else:
        schedule = [[x] for x in range(nx)]
    for blocks in schedule:
        for npass, blk in enumerate(blocks):
            if mutant == "second_pass_same_block" and npass == 1:
                blk = blocks[0]
            if mutant == "skip_middle" and causal and nx >= 3 and len(blocks) == 1:
                continue
            q0, q1 = blk * 128, min(blk * 128 + 128, Tq)
            qi = torch.arange(q0, q1)
            nt = min(ntk, ((q1 - 1) >> 6) + 1) if causal else ntk
            m = torch.full((B, H, q1 - q0), float("-inf"), dtype=torch.float64)
            l = torch.zeros_like(m)
            o = torch.zeros((B, H, q1 - q0, 64), dtype=torch.float64)
            for t in range(nt):
                pos = torch.arange(t * 64, t * 64 + 64)
                src = pos.clamp(max=Tk - 1)
                ok = (pos <= Tk if mutant == "clamp_dup" else pos < Tk)[None, :].expand(q1 - q0, 64)
                if causal:
                    ok = ok & ((pos[None, :] < qi[:, None]) if mutant == "causal_strict" else (pos[None, :] <= qi[:, None]))
                if mutant == "drop_tile_last_key":
                    ok = ok & (pos % 64 != 63)[None, :]
                s = (qh[:, :, q0:q1] @ kh[:, :, src].transpose(-1, -2)).masked_fill(~ok, float("-inf"))
                m_old = torch.full_like(m, float("-inf")) if mutant == "max_reset" else m
                m_new = torch.maximum(m_old, s.max(-1).values)
                m_safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
                alpha = torch.ones_like(m) if mutant == "no_rescale" else torch.exp(m_old - m_safe)
                p = torch.exp(s - m_safe[..., None])
                if p_fmt is not None:
                    p = p.to(p_fmt).double()
                l = l * alpha + p.sum(-1)
                o = o * alpha[..., None] + p @ vh[:, :, src]
                m = m_new
            out[:, :, q0:q1] = o / l[..., None]
            lse[:, :, q0:q1] = m + torch.log(l)
    if mutant == "heads_swapped":
        idx = [1, 0] + list(range(2, H))
        out, lse = out[:, idx], lse[:, idx]
    if mutant == "batch_swapped":
        idx = [1, 0] + list(range(2, B))
        out, lse = out[idx], lse[idx]
    return out.permute(0, 2, 1, 3).reshape(B, Tq, H * 64), lse
