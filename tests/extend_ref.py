"""CPU restatement of the attention of Tn new rows over a filled KV cache (kx_attention_extend in include/kosmosx_hip.h),
torch / float64.

Test infrastructure, written from the contract, not from the kernels.  Per (sequence, head):
  keys / values = cache rows 0 .. P-1 followed by the k | v of the Tn qkv rows (cache rows >= P are never read),
  score_ij = <k_j, q_i> (q arrives pre-scaled) for j <= P + i, -inf above that shifted diagonal, nan_to_num on the scores of
  the fp32 values (NaN -> 0, beyond +-FLT_MAX -> +-FLT_MAX, as decode_ref), softmax, P V;
  the new k | v are appended to rows P .. P + Tn - 1 of the caches.
Default cache layout only: [B, H, Tmax, 64].  Nothing here knows of tiles, query blocks or the order of the sums.
"""
from __future__ import annotations

import torch

FLT_MAX = 3.4028234663852886e38


def new_rows(qkv: torch.Tensor, B: int, H: int):
    """q, k, v of the new rows, each [B, H, Tn, 64] in the dtype of the rows (row b * Tn + i = sequence b's i-th)."""
    Tn = qkv.shape[0] // B
    x = qkv.reshape(B, Tn, 3, H, 64).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def extend_attention_ref(qkv, kcache, vcache, P, nan_to_num):
    """qkv [B*Tn, 3*H*64], kcache / vcache [B, H, Tmax, 64] (fp32 or bf16 VALUES; the arithmetic is float64), P = the rows every
    sequence has cached.  Returns (out [B*Tn, H*64] float64, kcache and vcache as they must be after the append: new tensors)."""
    B, H, Tmax, hd = kcache.shape
    Tn = qkv.shape[0] // B
    assert hd == 64 and tuple(qkv.shape) == (B * Tn, 3 * H * 64) and Tn >= 1 and 0 <= P and P + Tn <= Tmax
    q, kn, vn = new_rows(qkv, B, H)
    K = torch.cat([kcache[:, :, :P].double(), kn.double()], 2)                # [B, H, P + Tn, 64]
    V = torch.cat([vcache[:, :, :P].double(), vn.double()], 2)
    s = q.double() @ K.transpose(-1, -2)                                      # [B, H, Tn, P + Tn]
    if nan_to_num:
        s = torch.where(torch.isnan(s), torch.zeros_like(s), s).clamp(-FLT_MAX, FLT_MAX)
    i = torch.arange(Tn)[:, None]
    j = torch.arange(P + Tn)[None, :]
    s = torch.where(j <= P + i, s, torch.full((), float("-inf"), dtype=torch.float64))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    out = (p @ V).permute(0, 2, 1, 3).reshape(B * Tn, H * 64)
    k2, v2 = kcache.clone(), vcache.clone()
    k2[:, :, P:P + Tn] = kn
    v2[:, :, P:P + Tn] = vn
    return out, k2, v2


def random_extend(B, H, Tmax, P, Tn, dtype, seed, q_scale=0.35, k_scale=1.0, poison=True):
    """qkv, kcache, vcache on the CPU in `dtype`: q = randn * q_scale, k = randn * k_scale, v = randn, different for every (b, h).
    poison: cache rows >= P of both caches are NaN — the append must overwrite rows P .. P + Tn - 1, and nothing may read the rest."""
    g = torch.Generator().manual_seed(seed)
    D = H * 64
    qkv = torch.randn(B * Tn, 3 * D, generator=g)
    qkv[:, :D] *= q_scale
    qkv[:, D:2 * D] *= k_scale
    kc = torch.randn(B, H, Tmax, 64, generator=g) * k_scale
    vc = torch.randn(B, H, Tmax, 64, generator=g)
    if poison:
        kc[:, :, P:], vc[:, :, P:] = float("nan"), float("nan")
    return qkv.to(dtype), kc.to(dtype), vc.to(dtype)
