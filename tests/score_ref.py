"""CPU restatements for score() (include/kosmosx_hip.h, "Scoring candidates over a shared prompt cache"), torch / float64.

Test infrastructure, written from the contract, not from the kernels.
  shared_attention_ref: C candidates of K rows over Bc cache sequences; row (c, j) attends over cache[seq[c], :t0] and over the
    candidate's own rows 0..j, whose keys and values come from the qkv rows; the caches are returned as they were given.  Built
    from tests/decode_ref.py: a candidate is a block of K single-query steps on a private copy of its sequence.
  token_logprob_ref: x[target] - logsumexp(x) per output row, 0.0 for a target or a row index out of range.
The ``wrong`` argument of shared_attention_ref builds the stand-ins a broken kernel would compute; tests/test_score.py checks that
the GPU tests' inputs tell each of them from the reference.
"""
from __future__ import annotations

import torch

import decode_ref as DR

HH, TMAX, BC = 2, 320, 2
CACHE_SEQ = [1, 0, 1]
BASES = [0, 1, 5, 127, 128, 255, 256, 300]                 # both sides of the 128-key (fp32) and 256-key (bf16) first rounds
ROWS = [1, 2, 5, 16]


def shared_inputs(t0, K, dtype, seed, Tmax=TMAX, Hh=HH, Bc=BC, cache_seq=CACHE_SEQ):
    """qkv [C * K, 3D], caches [Bc, H, Tmax, 64] with rows >= t0 NaN, positions [C * K] int32, cache_seq [C] int32 — on the CPU."""
    C, D = len(cache_seq), Hh * 64
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(C * K, 3 * D, generator=g)
    qkv[:, :D] *= 0.35
    kc, vc = torch.randn(Bc, Hh, Tmax, 64, generator=g), torch.randn(Bc, Hh, Tmax, 64, generator=g)
    kc[:, :, t0:], vc[:, :, t0:] = float("nan"), float("nan")
    pos = torch.tensor([t0 + j for _ in range(C) for j in range(K)], dtype=torch.int32)
    return qkv.to(dtype), kc.to(dtype), vc.to(dtype), pos, torch.tensor(cache_seq, dtype=torch.int32)


def shared_attention_ref(qkv, kcache, vcache, t0, cache_seq, K, nan_to_num, wrong=None):
    """-> (out [C * K, H * 64] float64, kcache, vcache — the tensors given, untouched).
    ``wrong``: None, or the stand-in to compute instead — "cache_keys" (keys t0 + i, i < j, read from the cache rows, where nothing
    was appended), "candidate0" (every candidate's earlier rows taken from candidate 0), "identity_seq" (candidate c reads cache
    sequence c mod Bc, not cache_seq[c])."""
    C, Bc = len(cache_seq), kcache.shape[0]
    k0, v0 = kcache.clone(), vcache.clone()
    out = []
    for c in range(C):
        s = int(cache_seq[c]) if wrong != "identity_seq" else c % Bc
        kb, vb = kcache[s:s + 1].clone(), vcache[s:s + 1].clone()
        for j in range(K):
            r = c * K + j
            o, k2, v2 = DR.decode_attention_ref(qkv[r:r + 1], kb, vb, t0 + j, nan_to_num)
            out.append(o)
            if wrong == "cache_keys":
                continue                                    # the next row finds the poison at rows t0 .. t0 + j
            if wrong == "candidate0":                       # ... or candidate 0's k | v
                _, k2, v2 = DR.decode_attention_ref(qkv[j:j + 1], kb, vb, t0 + j, nan_to_num)
            kb, vb = k2, v2
    assert torch.equal(DR.bits(kcache), DR.bits(k0)) and torch.equal(DR.bits(vcache), DR.bits(v0))
    return torch.cat(out, 0), kcache, vcache


def causal_full_attention(qkv, kcache, vcache, t0, seq, c, K):
    """Candidate c as a causal attention over [prefix ‖ candidate]: the last K query rows of a (t0 + K)-token sequence.  float64,
    [K, H * 64].  (No nan_to_num: the rows it reads are finite.)"""
    Hh = kcache.shape[1]
    x = qkv[c * K:(c + 1) * K].double().reshape(K, 3, Hh, 64)
    q = x[:, 0].transpose(0, 1)                                                       # [H, K, 64]
    k = torch.cat([kcache[seq, :, :t0].double(), x[:, 1].transpose(0, 1)], 1)         # [H, t0 + K, 64]
    v = torch.cat([vcache[seq, :, :t0].double(), x[:, 2].transpose(0, 1)], 1)
    s = q @ k.transpose(1, 2)                                                         # [H, K, t0 + K]
    keep = torch.arange(t0 + K)[None, :] <= (t0 + torch.arange(K))[:, None]
    s = s.masked_fill(~keep[None], float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(K, Hh * 64)


def token_logprob_ref(logits, target, row_index=None, vocab=None):
    """float64 [R]: logits [rows, ld] (any float dtype), target [R] ints, row_index [R] ints or None (row r)."""
    rows, ld = logits.shape
    V = ld if vocab is None else vocab
    out = torch.zeros(len(target), dtype=torch.float64)
    for r in range(len(target)):
        row = r if row_index is None else int(row_index[r])
        tg = int(target[r])
        if not (0 <= tg < V and 0 <= row < rows):
            continue
        x = logits[row, :V].double()
        out[r] = x[tg] - torch.logsumexp(x, 0)
    return out
