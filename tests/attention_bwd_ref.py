"""CPU reference of the attention backward (kx_attention_backward, kx_attention_backward_dropout and
kx_attention_backward_dropout_bf16 in include/kosmosx_hip.h), torch / float64, the inputs and the checks the CPU and the GPU
tests of it share (tests/test_attention_bwd_ref.py, tests/test_attention_backward_gpu.py).

Test infrastructure, written from the header contract, not from the kernels.  Per (batch row, head), with q pre-scaled, the keep
mask M (all ones, or keep / (1 - p) of the Philox mask at element ((b H + h) T + q) T + k, drawn on the CPU by train_ref.keep_mask):
  S = Q K^T (KX_ATTN_CAUSAL keeps key <= query), lse = logsumexp(S), P = exp(S - lse), Pd = P o M, O = Pd V,
  delta = rowsum(dO o O), dPd = dO V^T, dS = P o (dPd o M - delta), dV = Pd^T dO, dK = dS^T Q, dQ = dS K.
The reference works on the VALUES of q, k, v and dO as rounded to what the kernel multiplies (round them first); the tests hand the
kernels out = fp32(O) and lse = fp32(lse) OF THE REFERENCE, so the backward is tested alone.  It knows nothing of tiles, waves or
the order of the sums; test_attention_bwd_ref.tiled_backward is the opposite, a restatement of the two-pass scheme of the kernels.

Bound, per element of X in (dV, dK, dQ); none of it is fitted to what a kernel returns:
  |X - ref| <= 2 u_p R_X + 2 u_p R_X + GAMMA 2^-24 C_X + floor_X
  u_p     2^-9 for the configurations with bf16 products: P (dropped and scaled) is rounded to bf16 before dV, dS before dK and dQ;
          a round-to-nearest bf16 (8 significant bits) is off by half a spacing, which is 2 u_p of the value at the bottom of its
          binade.  0 for the fp32 configurations.  The first term is that rounding; the second is the same term once more, the
          few-terms term: 2 u_p R_X is not an estimate but the EXACT worst case of one rounding, and a sum of one term reaches it —
          which is what the pair probes are built from (an element of dV there is c_i P_ij of ONE pair when T <= 64, of at most
          nine pairs at T = 513) and what a row that leans on one key is.  Against 2 u_p R_X alone the float64 restatement of
          tests/test_attention_bwd_ref.py, whose only error IS that rounding, reaches 0.99 of the bound on the probes, 0.96
          at a spike and 0.88 .. 0.93 on the random inputs, over the half that a right kernel must stay under (the forward's bound
          met the same and carries its binade term for it, attention_ref.py); with the term: 0.497, 0.49 and 0.44 .. 0.47.  One pair more or
          less, or one flipped keep bit, still moves an element of a probe by more than two of these bounds
          (test_the_probes_see_every_pair_and_every_mask_bit).
  R_X     what those rounded factors are multiplied into: R_dV = Pd^T |dO|, R_dK = |dS|^T |Q|, R_dQ = |dS| |K|.
  C_X     the fp32 condition of X: the same formula with every factor replaced by its absolute value and P and dS by their fp32
          uncertainty in units of 2^-24.  P = exp(S - lse): relative, 1 + sum_d |q_id k_jd| + |lse_i| (the products of the score, the
          statistic as stored in fp32, the exponential).  dS = P (dPd M - delta): P's relative uncertainty times |dPd M - delta|, plus
          P times the absolute uncertainty of the difference, sum_d |dO_id v_jd| M + sum_d |dO_id O_id| (the two sums it is the
          difference of; delta is summed from the fp32 O the kernel is handed).
          C_dV = (Pd o condP)^T |dO|, C_dK = E^T |Q|, C_dQ = E |K| with E = P o (condP o |dPd M - delta| + that absolute term).
  floor_X 3e-5 x the rms of the reference's X block (3e-5 is the project's bound of test_grad_ops_gpu.py::test_attention_backward
          on max |d| / rms, so this is no looser).  A block that is exactly zero (dK of probe A, dQ of probe B) has R = C = floor
          = 0: the check is then equality with zero.
  GAMMA   = 4: the smallest power of two at which the float32-arithmetic restatement of tests/test_attention_bwd_ref.py (fp32
          products and sums, no bf16 rounding) stays at or under 0.5 of the bound on every shape and input below: it needs 2.97
          (fp32, random, unmasked T = 130, dK; the dropout configuration 2.35 at causal T = 257, dV; the probes and the configurations
          with bf16 products less than 1) and sits at 0.40 with 4 — measured against that restatement, never against a kernel.
"""
from __future__ import annotations

import collections
import functools

import numpy as np
import torch

import attention_ref as AR
import train_ref as TR
from attention_ref import bits, verdict, random_qkv, plant_spike  # noqa: F401  (re-exported: the tests take them from here)

GAMMA = 4.0
FLOOR = 3e-5

Config = collections.namedtuple("Config", "entry values store fmt u_p key2")
# name -> entry point ("plain" = kx_attention_backward, "valu-drop" = kx_attention_backward_dropout, "bf16-drop" = ..._dropout_bf16),
# dtype the VALUES of q / k / v / dO are exact in, dtype q / k / v are stored in, format P and dS are rounded to, u_p, tuning key 2
CONFIGS = {
    "fp32": Config("plain", torch.float32, torch.float32, None, 0.0, 0),
    "fp32-valu": Config("plain", torch.float32, torch.float32, None, 0.0, 1),
    "bf16p/f32": Config("plain", torch.bfloat16, torch.float32, torch.bfloat16, 2.0 ** -9, 0),
    "bf16p/bf16": Config("plain", torch.bfloat16, torch.bfloat16, torch.bfloat16, 2.0 ** -9, 0),
    "valu-drop": Config("valu-drop", torch.float32, torch.float32, None, 0.0, 0),
    "bf16-drop/f32": Config("bf16-drop", torch.bfloat16, torch.float32, torch.bfloat16, 2.0 ** -9, 0),
    "bf16-drop/bf16": Config("bf16-drop", torch.bfloat16, torch.bfloat16, torch.bfloat16, 2.0 ** -9, 0),
}
PLAIN = [n for n, c in CONFIGS.items() if c.entry == "plain"]
DROP = [n for n, c in CONFIGS.items() if c.entry != "plain"]
B, H = 2, 3
PLAIN_T = [1, 2, 15, 16, 17, 63, 64, 65, 79, 80, 81, 127, 128, 129, 130, 131, 191, 192, 193, 257, 321, 513]
DROP_T = [1, 3, 4, 5, 63, 64, 65, 70, 114, 130, 131, 257]       # every residue of T mod 4
P_DROP = 0.25
SEED, SITE = 0x5DEECE66D1234, 5                                  # a seed with bits above 2^32


def shapes(name):
    """(B, H, T, p) of every shape of a configuration (both masks run all of them)."""
    if CONFIGS[name].entry == "plain":
        return [(B, H, t, 0.0) for t in PLAIN_T]
    return [(B, H, t, P_DROP) for t in DROP_T] + [(B, H, 114, 0.1)]


def wide_shape(name):
    """The one (B, H) = (1, 9) case: the bf16 grids are head-fastest and tuned for H % 8 == 0."""
    return (1, 9, 257, 0.0 if CONFIGS[name].entry == "plain" else P_DROP)


def _hm(x):
    """[B, T, H, 64] -> heads-major float64 [B, H, T, 64]."""
    return x.double().permute(0, 2, 1, 3)


def _tm(x):
    """... and back: [B, H, T, 64] -> [B, T, H, 64]."""
    return x.permute(0, 2, 1, 3).contiguous()


def f32(x: float) -> float:
    return float(np.float32(x))


def keep_scale(Bc, Hc, T, p, seed=SEED, site=SITE):
    """M [B, H, T, T] float64: keep / (1 - p) of the CPU Philox mask (train_ref.keep_mask) at ((b H + h) T + q) T + k; ones at p = 0."""
    if p == 0:
        return torch.ones(Bc, Hc, T, T, dtype=torch.float64)
    keep = TR.keep_mask(Bc * Hc * T * T, p, seed, site).reshape(Bc, Hc, T, T)
    return torch.from_numpy(keep.astype(np.float64)) / (1.0 - f32(p))


def visible(T, causal):
    """bool [T, T]: query i (rows) sees key j (columns)."""
    if not causal:
        return torch.ones(T, T, dtype=torch.bool)
    return torch.arange(T)[None, :] <= torch.arange(T)[:, None]


class Reference:
    """The float64 gradients of one input, what the kernels are handed (out, lse) and the parts of the bounds; [B, T, H, 64]."""

    def __init__(self, q, k, v, dO, causal, M=None):
        Bc, T, Hc, hd = q.shape
        assert hd == 64 and k.shape == q.shape and v.shape == q.shape and dO.shape == q.shape
        qh, kh, vh, gh = _hm(q), _hm(k), _hm(v), _hm(dO)
        M = torch.ones(Bc, Hc, T, T, dtype=torch.float64) if M is None else M
        S = (qh @ kh.transpose(-1, -2)).masked_fill(~visible(T, causal), float("-inf"))
        lse = torch.logsumexp(S, -1)
        P = torch.exp(S - lse[..., None])
        Pd = P * M
        O = Pd @ vh
        delta = (gh * O).sum(-1)
        dPd = gh @ vh.transpose(-1, -2)
        X = dPd * M - delta[..., None]
        dS = P * X
        self.dv, self.dk, self.dq = _tm(Pd.transpose(-1, -2) @ gh), _tm(dS.transpose(-1, -2) @ qh), _tm(dS @ kh)
        self.out, self.lse = _tm(O).reshape(Bc, T, Hc * 64), lse
        self.P, self.M, self.Pd, self.dPd, self.dS = P, M, Pd, dPd, dS        # (T^2 values each: the largest shape holds 1.6 M)
        condP = 1.0 + qh.abs() @ kh.abs().transpose(-1, -2) + lse.abs()[..., None]
        absdiff = (gh.abs() @ vh.abs().transpose(-1, -2)) * M + (gh * O).abs().sum(-1)[..., None]
        E = P * (condP * X.abs() + absdiff)
        self.R = {"dv": _tm(Pd.transpose(-1, -2) @ gh.abs()), "dk": _tm(dS.abs().transpose(-1, -2) @ qh.abs()),
                  "dq": _tm(dS.abs() @ kh.abs())}
        self.C = {"dv": _tm((Pd * condP).transpose(-1, -2) @ gh.abs()), "dk": _tm(E.transpose(-1, -2) @ qh.abs()),
                  "dq": _tm(E @ kh.abs())}
        self.rms = {x: float(getattr(self, x).pow(2).mean().sqrt()) for x in ("dv", "dk", "dq")}

    def rounding_term(self, name, x):
        return 2.0 * CONFIGS[name].u_p * self.R[x]

    def few_terms_term(self, name, x):
        """2 u_p R_X once more: the rounding term is reached by a sum of ONE term (module docstring)."""
        return 2.0 * CONFIGS[name].u_p * self.R[x]

    def bound(self, name, x):
        return self.rounding_term(name, x) + self.few_terms_term(name, x) + GAMMA * 2.0 ** -24 * self.C[x] + FLOOR * self.rms[x]


# ---- the shared checks: every comparison of the CPU and the GPU file goes through these -------------------------------------
def _grad_ratio(name, x, got, R):
    """max error / bound of one gradient ([B, T, H, 64]); a bound of exactly 0 admits exactly 0 (1e-300 turns 0 / 0 into 0)."""
    want = getattr(R, x)
    if tuple(got.shape) != tuple(want.shape):
        return float("inf")
    return AR._ratio(got, want, R.bound(name, x).clamp(min=1e-300))


def dq_ratio(name, dq, R):
    return _grad_ratio(name, "dq", dq, R)


def dk_ratio(name, dk, R):
    return _grad_ratio(name, "dk", dk, R)


def dv_ratio(name, dv, R):
    return _grad_ratio(name, "dv", dv, R)


def grad_ratios(name, dq, dk, dv, R, what):
    """[(error / bound, (what, gradient))] of the three gradients of one launch, for verdict."""
    return [(dq_ratio(name, dq, R), (what, "dq")), (dk_ratio(name, dk, R), (what, "dk")), (dv_ratio(name, dv, R), (what, "dv"))]


# ---- inputs -------------------------------------------------------------------------------------------------------------
def random_inputs(Bc, Hc, T, values, seed):
    """random_qkv's q = randn * 0.35, k, v = randn, and dO = randn, all rounded to `values` (for the configurations with bf16
    products the kernel's own rounding of Q, K, V and dO is then a no-op, and the reference needs no term for it)."""
    q, k, v = random_qkv(Bc, Hc, T, T, values, seed)
    dO = torch.randn(Bc, T, Hc, 64, generator=torch.Generator().manual_seed(seed + 1)).to(values)
    return q, k, v, dO


def probe_inputs(Bc, Hc, T, causal, which, seed):
    """The pair probes (float32; every value is exact in bf16).  With n_i the number of keys query i sees and c_i = 2^ceil(log2 n_i):
    dO[i] = c_i e_(i mod 64), v = random integers of +-{1, 2, 3}; probe "A": q = 0, K[j] = e_(j mod 64); probe "B": k = 0,
    Q[i] = e_(i mod 64).  Every score is 0 and P_ij = 1 / n_i, so that c_i P_ij lies in [1, 2): an element of dV is a sum of at most
    ceil(T / 64) such terms, one per query i = d (mod 64) — every pair shows in it on its own; an element of dQ (A) or dK (B)
    is a sum of at most ceil(T / 64) terms dS_ij; dK (A) and dQ (B) are exactly 0."""
    assert which in ("A", "B")
    g = torch.Generator().manual_seed(seed)
    n = torch.arange(1, T + 1) if causal else torch.full((T,), T)
    c = 2.0 ** torch.ceil(torch.log2(n.double()))
    unit = torch.eye(64)[torch.arange(T) % 64]                                      # [T, 64]: row i = e_(i mod 64)
    dO = (c[:, None] * unit.double()).float()[None, :, None, :].expand(Bc, T, Hc, 64).contiguous()
    v = (torch.randint(1, 4, (Bc, T, Hc, 64), generator=g) * (2 * torch.randint(0, 2, (Bc, T, Hc, 64), generator=g) - 1)).float()
    rows = unit[None, :, None, :].expand(Bc, T, Hc, 64).contiguous()
    zero = torch.zeros(Bc, T, Hc, 64)
    return (zero, rows, v, dO) if which == "A" else (rows, zero, v, dO)


@functools.lru_cache(maxsize=None)
def _case(kind, Bc, Hc, T, values, causal, p):
    seed = {"random": 11, "A": 7, "B": 13}[kind] * 100003 + T * 2053 + 5 * Hc + (1 if causal else 0)
    if kind == "random":
        q, k, v, dO = random_inputs(Bc, Hc, T, values, seed)
    else:
        q, k, v, dO = probe_inputs(Bc, Hc, T, causal, kind, seed)
    return q, k, v, dO, Reference(q, k, v, dO, causal, keep_scale(Bc, Hc, T, p))


def case(kind, Bc, Hc, T, values, causal, p=0.0):
    """(q, k, v, dO [B, T, H, 64], Reference) of the "random" / "A" / "B" inputs of one shape, built once and shared: read-only.
    The probes are the same float32 tensors for every configuration (their values are exact in bf16)."""
    return _case(kind, Bc, Hc, T, values if kind == "random" else torch.float32, causal, float(p))


# (T, causal, query, key): causal T = 193 (four tiles, a last tile of one row) — a key of the first tile and one next to the
# diagonal for the only query of the last tile, a key at a tile start for a query two tiles on and for one of its own tile;
# unmasked T = 129: the diagonal pair of the ragged last tile.
SPIKES = [(193, True, 192, 0), (193, True, 192, 191), (193, True, 130, 64), (193, True, 70, 64), (129, False, 128, 128)]


@functools.lru_cache(maxsize=None)
def spike_case(values, i):
    """(q, k, v, dO, Reference, weights) of SPIKES[i]: random inputs with attention_ref.plant_spike's key in every (b, h) — the key
    holds about half of its row, so P is neither flat nor one-hot and |lse| is a few units; read-only."""
    T, causal, query, key = SPIKES[i]
    q, k, v, dO = random_inputs(B, H, T, values, seed=900 + i)
    w = [plant_spike(q, k, b, h, query, key, causal) for b in range(B) for h in range(H)]
    return q, k, v, dO, Reference(q, k, v, dO, causal), w


# ---- what one pair or one mask bit is worth (the coverage of the probes) --------------------------------------------------
def pair_visibility(name, kind, R, causal):
    """For every (b, h, query i, key j) of a probe: by how many bounds the ONE element a pair lands in moves when that pair is
    left out of a sum, and when its mask bit is flipped.  A pair lands in dV[j, i mod 64] with Pd_ij c_i and, with dS_ij, in
    dQ[i, j mod 64] (probe A: K[j] = e_(j mod 64)) or in dK[j, i mod 64] (probe B: Q[i] = e_(i mod 64)).  A flipped bit (delta as
    handed in) moves Pd_ij by P_ij / (1 - p) and dS_ij by P_ij dPd_ij / (1 - p).
    -> (vis [T, T] bool, kept [B, H, T, T] bool, {"dv", "ds", "dv_flip", "ds_flip": [B, H, T, T] float64 moves / bound})."""
    T = R.P.shape[-1]
    vis = visible(T, causal)
    ii, jj = torch.arange(T)[:, None].expand(T, T), torch.arange(T)[None, :].expand(T, T)
    hm = {x: R.bound(name, x).permute(0, 2, 1, 3) for x in ("dv", "dk", "dq")}           # [B, H, T, 64]
    bdv = hm["dv"][:, :, jj, ii % 64]
    bds = hm["dq"][:, :, ii, jj % 64] if kind == "A" else hm["dk"][:, :, jj, ii % 64]
    c = (2.0 ** torch.ceil(torch.log2(vis.sum(-1).double())))[:, None]
    inv = float(R.M.max())                                       # 1 / (1 - p), or 1
    return vis, (R.M > 0) & vis, {"dv": (R.Pd * c).abs() / bdv, "ds": R.dS.abs() / bds,
                                  "dv_flip": R.P * inv * c / bdv, "ds_flip": (R.P * R.dPd * inv).abs() / bds}
