"""CPU restatement of the ragged extend attention (kx_attention_extend_ragged in include/kosmosx_hip.h), torch / float64: the
attention of tests/extend_ref.py applied to every sequence on its own, with the sequence's own P.

Test infrastructure, written from the contract: sequence b's caches hold positions[b] rows, its Tn rows are appended at
positions[b] .. positions[b] + Tn - 1 and query i attends that sequence's cache rows 0 .. positions[b] + i.  A sequence whose rows
leave [0, Tmax) is guarded: no output row, no cache row.  Default cache layout only.
"""
from __future__ import annotations

import torch

import extend_ref as ER


def guarded(P: int, Tn: int, Tmax: int) -> bool:
    return P < 0 or P + Tn > Tmax


def random_extend_ragged(H, Tmax, positions, Tn, dtype, seed, q_scale=0.35, k_scale=1.0):
    """qkv [B*Tn, 3*H*64], kcache, vcache [B, H, Tmax, 64] on the CPU in `dtype`; sequence b's cache rows at and after
    positions[b] are NaN (a guarded sequence: from row 0 for a negative position, nothing for one past the end)."""
    B = len(positions)
    qkv, kc, vc = ER.random_extend(B, H, Tmax, 0, Tn, dtype, seed, q_scale, k_scale, poison=False)
    for b, P in enumerate(positions):
        kc[b, :, max(P, 0):], vc[b, :, max(P, 0):] = float("nan"), float("nan")
    return qkv, kc, vc


def sequence(qkv, kc, vc, b, Tn):
    """Sequence b alone: its qkv rows and its caches as a batch of one."""
    return qkv[b * Tn:(b + 1) * Tn].contiguous(), kc[b:b + 1].contiguous(), vc[b:b + 1].contiguous()


def extend_ragged_attention_ref(qkv, kcache, vcache, positions, nan_to_num):
    """Returns (out [B*Tn, H*64] float64 — NaN rows for a guarded sequence, which has no output —, kcache and vcache as they must
    be after the launch: new tensors, a guarded sequence's unchanged)."""
    B, H, Tmax, _ = kcache.shape
    Tn = qkv.shape[0] // B
    out = torch.full((B * Tn, H * 64), float("nan"), dtype=torch.float64)
    k2, v2 = kcache.clone(), vcache.clone()
    for b, P in enumerate(positions):
        if guarded(P, Tn, Tmax):
            continue
        o, kb, vb = ER.extend_attention_ref(*sequence(qkv, kcache, vcache, b, Tn), P, nan_to_num)
        out[b * Tn:(b + 1) * Tn], k2[b], v2[b] = o, kb[0], vb[0]
    return out, k2, v2
