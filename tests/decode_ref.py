"""CPU restatement of the decode step's single-query attention (kx_attention_decode in include/kosmosx_hip.h), torch / float64.

Test infrastructure, written from the contract, not from the kernel.  Per (sequence, head):
  keys / values = cache rows 0 .. t-1 followed by the new token's k | v of the qkv row (cache row t is never read),
  score_j = <k_j, q> (q arrives pre-scaled), nan_to_num on the scores of the fp32 cache (NaN -> 0, beyond +-FLT_MAX ->
  +-FLT_MAX: torchscale's `attn_weights = torch.nan_to_num(attn_weights)` at one query), softmax, P V;
  the new k | v are appended to row t of the caches.
Default cache layout only: [B, H, Tmax, 64].  Nothing here knows of slots, rounds or the order of the sums.
"""
from __future__ import annotations

import torch

FLT_MAX = 3.4028234663852886e38


def new_token(qkv: torch.Tensor, H: int):
    """q, k, v of the new token, each [B, H, 64] in the dtype of the row."""
    B = qkv.shape[0]
    x = qkv.reshape(B, 3, H, 64)
    return x[:, 0], x[:, 1], x[:, 2]


def decode_scores(qkv, kcache, t, nan_to_num):
    """[B, H, t + 1] float64: the scores of keys 0 .. t (key t = the new token's)."""
    B, H, Tmax, hd = kcache.shape
    assert hd == 64 and 0 <= t < Tmax and tuple(qkv.shape) == (B, 3 * H * 64)
    q, kn, _ = new_token(qkv, H)
    K = torch.cat([kcache[:, :, :t].double(), kn.double()[:, :, None]], 2)
    s = (K * q.double()[:, :, None]).sum(-1)
    if nan_to_num:
        s = torch.where(torch.isnan(s), torch.zeros_like(s), s).clamp(-FLT_MAX, FLT_MAX)
    return s


def decode_weights(qkv, kcache, t, nan_to_num):
    """[B, H, t + 1] float64 softmax weights."""
    s = decode_scores(qkv, kcache, t, nan_to_num)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def decode_attention_ref(qkv, kcache, vcache, t, nan_to_num):
    """qkv [B, 3*H*64], kcache / vcache [B, H, Tmax, 64] (fp32 or bf16 VALUES; the arithmetic is float64), t = the number of
    cached tokens.  Returns (out [B, H*64] float64, kcache and vcache as they must be after the append: new tensors)."""
    B, H, Tmax, _ = kcache.shape
    _, kn, vn = new_token(qkv, H)
    p = decode_weights(qkv, kcache, t, nan_to_num)
    V = torch.cat([vcache[:, :, :t].double(), vn.double()[:, :, None]], 2)
    out = (p[..., None] * V).sum(2).reshape(B, H * 64)
    k2, v2 = kcache.clone(), vcache.clone()
    k2[:, :, t] = kn
    v2[:, :, t] = vn
    return out, k2, v2


def spike_scale(qkv, kcache, t, j):
    """c [B, H] float64 such that the key c * q in place of key j (j <= t) holds half of the softmax weight: c |q|^2 = the
    log-sum-exp of the other scores."""
    B, Hh = kcache.shape[:2]
    q, _, _ = new_token(qkv, Hh)
    s = decode_scores(qkv, kcache, t, False)
    s[:, :, j] = float("-inf")
    return torch.logsumexp(s, -1) / q.double().pow(2).sum(-1)


def rel_err64(a, b):
    """helpers.rel_err (max |a - b| over the rms of the reference b) without the detour through fp32."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.pow(2).mean().sqrt() + 1e-300))


def bits(x: torch.Tensor) -> torch.Tensor:
    """Integer view of the bits (NaN != NaN, and a poisoned cache is full of them)."""
    return x.contiguous().view(torch.int32 if x.element_size() == 4 else torch.int16)


def random_step(B, H, Tmax, t, dtype, seed, q_scale=0.35, poison=True):
    """qkv, kcache, vcache on the CPU in `dtype`: q = randn * q_scale, k and v = randn, different for every (b, h).  poison: cache
    rows >= t of both caches are NaN — row t too: key t comes from the qkv row, and the append must overwrite the poison."""
    g = torch.Generator().manual_seed(seed)
    D = H * 64
    qkv = torch.randn(B, 3 * D, generator=g)
    qkv[:, :D] *= q_scale
    kc, vc = torch.randn(B, H, Tmax, 64, generator=g), torch.randn(B, H, Tmax, 64, generator=g)
    if poison:
        kc[:, :, t:], vc[:, :, t:] = float("nan"), float("nan")
    return qkv.to(dtype), kc.to(dtype), vc.to(dtype)
