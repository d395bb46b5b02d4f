"""CPU restatements for the prefix form of the decode attention (include/kosmosx_hip.h, "Decoding rows over a shared, read-only
prefix cache plus a private tail cache"), torch / float64.

Test infrastructure, written from the contract, not from the kernel.
  prefix_inputs: qkv [M, 3D], prefix caches [Bp, H, Tmax, 64], tail caches [M, H, Ttail, 64] and the rows' three words.  The caches
    are poisoned so that a wrong read shows: prefix rows >= P and tail rows >= t - P are NaN (tail row t - P too: key t comes from the
    qkv row, and the append must overwrite the poison), the tail rows are drawn independently of the prefix rows at the same index,
    and the last prefix key of a sequence carries real softmax weight for the rows that read it.
  assemble: the private cache [M, H, Tmax, 64] a ragged launch would hold — rows 0 .. P - 1 the prefix rows of prefix_seq[r], rows
    P .. t - 1 the tail rows 0 .. t - P - 1 of sequence r, NaN from row t on.
  prefix_attention_ref: row r is tests/decode_ref.py's single-query step at t on its assembled sequence; returns the outputs and the
    tail caches as they must be after the append.
The ``wrong`` argument of prefix_attention_ref builds the stand-ins a broken kernel would compute; tests/test_prefix_ref.py checks that
the GPU tests' inputs tell each of them from the reference.
"""
from __future__ import annotations

import torch

import decode_ref as DR
from score_ref import HH, TMAX

BP, TTAIL = 2, 48
PREFIX_SEQ = [1, 0, 1, 1, 0]
M = len(PREFIX_SEQ)
PREFIXES = [0, 1, 127, 128, 129, 255, 256, 257]            # both sides of the 128-key (fp32) and 256-key (bf16) first rounds
FILLS = [0, 1, 15, 16, 17, 40]                              # tail keys t - P; 0: the first step, no tail key
CASES = [(P, f) for P in PREFIXES for f in FILLS]
assert all(P + f < TMAX and f < TTAIL for P, f in CASES)
WRONG = ("tail_at_j", "identity_seq", "key_t_from_tail", "prefix_short")


def _per_row(v, rows):
    return [int(v)] * rows if isinstance(v, int) else [int(x) for x in v]


def prefix_inputs(P, fill, dtype, seed, Tmax=TMAX, Hh=HH, Bp=BP, Ttail=TTAIL, prefix_seq=PREFIX_SEQ):
    """``P`` / ``fill``: an int for every row, or one per row.  -> qkv, kprefix, vprefix, ktail, vtail (in ``dtype``), positions,
    prefix_seq, prefix_len (int32 [M]) — on the CPU.  Prefix sequence c is NaN from the largest P of the rows that name it."""
    rows, D = len(prefix_seq), Hh * 64
    Ps, fills = _per_row(P, rows), _per_row(fill, rows)
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(rows, 3 * D, generator=g)
    qkv[:, :D] *= 0.35
    kp, vp = torch.randn(Bp, Hh, Tmax, 64, generator=g), torch.randn(Bp, Hh, Tmax, 64, generator=g)
    kt, vt = torch.randn(rows, Hh, Ttail, 64, generator=g), torch.randn(rows, Hh, Ttail, 64, generator=g)
    for c in range(Bp):
        top = max([Ps[r] for r in range(rows) if prefix_seq[r] == c], default=0)
        kp[c, :, top:], vp[c, :, top:] = float("nan"), float("nan")
        if top >= 1:
            # The last prefix key is the sum of its rows' queries: its score is about |q|^2 = 64 * 0.35^2 = 7.8 for each of them, the
            # height of the largest of a few hundred random scores (std 2.8), so it holds a few per cent of the softmax weight at
            # least and a kernel that drops it (or takes it from the other sequence) is off by far more than any rounding.
            kp[c, :, top - 1] = sum(qkv[r, :D].reshape(Hh, 64) for r in range(rows) if prefix_seq[r] == c and Ps[r] == top)
    for r in range(rows):
        kt[r, :, fills[r]:], vt[r, :, fills[r]:] = float("nan"), float("nan")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    return (qkv.to(dtype), kp.to(dtype), vp.to(dtype), kt.to(dtype), vt.to(dtype), i32([p + f for p, f in zip(Ps, fills)]),
            i32(list(prefix_seq)), i32(Ps))


def assemble(prefix, tail, positions, prefix_seq, prefix_len, Tmax=None):
    """[M, H, Tmax, 64] in the caches' dtype: sequence r = prefix rows 0 .. P - 1 of prefix_seq[r], then tail rows 0 .. t - P - 1 of
    sequence r, NaN from row t on."""
    rows, Hh = tail.shape[:2]
    Tmax = prefix.shape[2] if Tmax is None else Tmax
    out = torch.full((rows, Hh, Tmax, 64), float("nan"), dtype=prefix.dtype)
    for r in range(rows):
        t, c, P = int(positions[r]), int(prefix_seq[r]), int(prefix_len[r])
        out[r, :, :P] = prefix[c, :, :P]
        out[r, :, P:t] = tail[r, :, :t - P]
    return out


def _wrong_sequence(wrong, r, kp, vp, kt, vt, t, c, P):
    """The private (k, v) sequence [1, H, Tmax, 64] of row r as the stand-in ``wrong`` would read it, and the position it attends at."""
    Tmax, Ttail, Bp = kp.shape[2], kt.shape[2], kp.shape[0]
    if wrong == "identity_seq":                              # prefix sequence r, not prefix_seq[r]
        c = r % Bp
    seq = []
    for pre, tail in ((kp, kt), (vp, vt)):
        x = torch.full((1, pre.shape[1], Tmax + 1, 64), float("nan"), dtype=pre.dtype)
        x[0, :, :P] = pre[c, :, :P]
        if wrong == "tail_at_j":                             # tail key j read from tail row j, not j - P
            for j in range(P, t):
                if j < Ttail:
                    x[0, :, j] = tail[r, :, j]
        else:
            x[0, :, P:t] = tail[r, :, :t - P]
        if wrong == "prefix_short" and P >= 1:               # the prefix stops one key early: key P - 1 is never attended
            x = torch.cat([x[:, :, :P - 1], x[:, :, P:]], 2)
        seq.append(x)
    return seq[0], seq[1], (t - 1 if wrong == "prefix_short" and P >= 1 else t)


def prefix_attention_ref(qkv, kprefix, vprefix, ktail, vtail, positions, prefix_seq, prefix_len, nan_to_num, wrong=None):
    """-> (out [M, H * 64] float64, ktail, vtail as they must be after the append: new tensors; kprefix / vprefix are only read).
    ``wrong``: None, or the stand-in to compute instead (the outputs alone are meant) — "tail_at_j" (tail key j read from tail row j
    instead of j - P), "identity_seq" (row r reads prefix sequence r mod Bp, not prefix_seq[r]), "key_t_from_tail" (key t read from
    tail row t - P, where nothing was appended yet, instead of the qkv row), "prefix_short" (the prefix stops one key early)."""
    rows, Hh = ktail.shape[:2]
    k0, v0 = kprefix.clone(), vprefix.clone()
    out, kt2, vt2 = [], ktail.clone(), vtail.clone()
    for r in range(rows):
        t, c, P = int(positions[r]), int(prefix_seq[r]), int(prefix_len[r])
        assert 0 <= c < kprefix.shape[0] and 0 <= P <= t and t - P < ktail.shape[2]
        row = qkv[r:r + 1]
        if wrong is None:
            kb = assemble(kprefix, ktail[r:r + 1], [t], [c], [P])
            vb = assemble(vprefix, vtail[r:r + 1], [t], [c], [P])
            tt = t
        else:
            kb, vb, tt = _wrong_sequence(wrong, r, kprefix, vprefix, ktail, vtail, t, c, P)
            if wrong == "key_t_from_tail":                   # the new token's k | v replaced by what tail row t - P holds
                row = qkv[r:r + 1].clone().reshape(1, 3, Hh, 64)
                row[0, 1], row[0, 2] = ktail[r, :, t - P], vtail[r, :, t - P]
                row = row.reshape(1, 3 * Hh * 64)
        o, k2, v2 = DR.decode_attention_ref(row, kb, vb, tt, nan_to_num)
        out.append(o)
        if wrong is None:
            kt2[r, :, t - P], vt2[r, :, t - P] = k2[0, :, t], v2[0, :, t]
    assert torch.equal(DR.bits(kprefix), DR.bits(k0)) and torch.equal(DR.bits(vprefix), DR.bits(v0))
    return torch.cat(out, 0), kt2, vt2


def direct_attention(qkv, kprefix, vprefix, ktail, vtail, t, c, P, r):
    """Row r as a softmax over [prefix rows ‖ tail rows ‖ new key], written out once more without decode_ref: float64 [H * 64].
    (No nan_to_num: the rows it reads are finite.)"""
    Hh = ktail.shape[1]
    x = qkv[r].double().reshape(3, Hh, 64)
    k = torch.cat([kprefix[c, :, :P].double(), ktail[r, :, :t - P].double(), x[1][:, None]], 1)      # [H, t + 1, 64]
    v = torch.cat([vprefix[c, :, :P].double(), vtail[r, :, :t - P].double(), x[2][:, None]], 1)
    s = (k * x[0][:, None]).sum(-1)
    return (torch.softmax(s, -1)[..., None] * v).sum(1).reshape(Hh * 64)
