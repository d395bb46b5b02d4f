"""Float64 references of the small kernels the training step is built from (kx_backward.hip / kx_rowops.hip: dropout masks,
cross-entropy, embedding backward, AdamW, Lion, QuickGELU, add_rowvec, patchify, vit_assemble), restated from the C header's
definitions in numpy / torch on the CPU, and the inputs the CPU test (test_train_ref.py) and the GPU test
(test_train_kernels_gpu.py) share.  Nothing here imports the product."""
from __future__ import annotations

import math

import numpy as np
import torch

# ---------------------------------------------------------------------------------------------------------------------
# Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in integer arithmetic
# ---------------------------------------------------------------------------------------------------------------------
_M0, _M1 = 0xD2511F53, 0xCD9E8D57            # round multipliers
_W0, _W1 = 0x9E3779B9, 0xBB67AE85            # Weyl key increments
_MASK = 0xFFFFFFFF


def philox4x32_10(ctr4, key2, rounds: int = 10) -> np.ndarray:
    """ctr4: four 32-bit counter words (ints or equal-shaped integer arrays), key2: two 32-bit key words (ints)
    -> uint64 array [..., 4] holding the four 32-bit output words.  Products of two 32-bit words fit 64 bits exactly."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & np.uint64(_MASK) for c in np.broadcast_arrays(*ctr4))
    k0, k1 = int(key2[0]) & _MASK, int(key2[1]) & _MASK
    sh, mask = np.uint64(32), np.uint64(_MASK)
    for _ in range(rounds):
        p0, p1 = c0 * np.uint64(_M0), c2 * np.uint64(_M1)
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack([c0, c1, c2, c3], -1)


def dropout_thresh(p: float) -> int:
    """Keep iff word >= thresh: 0 for p = 0, else floor(fp32(p) * 2^32) (exact in fp32: a power-of-two scaling)."""
    return 0 if p == 0 else int(float(np.float32(p)) * 2 ** 32)


def keep_mask(n: int, p: float, seed: int, site: int, rounds: int = 10) -> np.ndarray:
    """uint8 [n]: element i keeps iff word (i & 3) of Philox(ctr = (lo32(i>>2), hi32(i>>2), site, 0),
    key = (lo32(seed), hi32(seed))) >= thresh."""
    blk = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((blk & np.uint64(_MASK), blk >> np.uint64(32), np.uint64(site), np.uint64(0)),
                      (seed & _MASK, (seed >> 32) & _MASK), rounds)
    return (w.reshape(-1)[:n] >= np.uint64(dropout_thresh(p))).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# cross-entropy rows
# ---------------------------------------------------------------------------------------------------------------------
def cross_entropy(logits: torch.Tensor, target: torch.Tensor, scale: float):
    """-> (loss_rows [M], dlogits [M,V]) in float64: loss = logsumexp(row) - row[target], dlogits = (softmax - onehot) *
    scale; a target outside [0, V) gives zero loss and a zero gradient row."""
    x = logits.double()
    M, V = x.shape
    mx = x.max(1, keepdim=True).values
    e = torch.exp(x - mx)
    s = e.sum(1, keepdim=True)
    lse = (mx + torch.log(s))[:, 0]
    valid = (target >= 0) & (target < V)
    tg = target.clamp(0, V - 1)
    loss = torch.where(valid, lse - x.gather(1, tg[:, None])[:, 0], torch.zeros_like(lse))
    g = e / s
    g[torch.arange(M), tg] -= 1.0
    g = g * float(scale)
    g[~valid] = 0.0
    return loss, g


# ---------------------------------------------------------------------------------------------------------------------
# embedding backward
# ---------------------------------------------------------------------------------------------------------------------
def embed_backward(tokens: torch.Tensor, dx: torch.Tensor, vocab: int, max_pos: int, pos_offset: int = 0):
    """-> (dembed [vocab,d], dpos [max_pos,d]) in float64: dembed[v] = sum of the dx rows whose token is v,
    dpos[2 + pos_offset + t] = sum_b dx[b, t], every other row zero."""
    B, T, d = dx.shape
    x = dx.double()
    de = torch.zeros(vocab, d, dtype=torch.float64).index_add_(0, tokens.reshape(-1), x.reshape(B * T, d))
    dp = torch.zeros(max_pos, d, dtype=torch.float64)
    dp[2 + pos_offset:2 + pos_offset + T] = x.sum(0)
    return de, dp


def embed_backward_inorder_f32(tokens: torch.Tensor, dx: torch.Tensor, vocab: int, max_pos: int, pos_offset: int = 0):
    """The same sums taken in fp32, each from 0 in increasing (b, t) order: pure adds, so a kernel that keeps the order
    gives these bits."""
    B, T, d = dx.shape
    x = dx.float().reshape(B * T, d)
    de = torch.zeros(vocab, d, dtype=torch.float32)
    for r, v in enumerate(tokens.reshape(-1).tolist()):
        de[v] += x[r]
    dp = torch.zeros(max_pos, d, dtype=torch.float32)
    for b in range(B):
        dp[2 + pos_offset:2 + pos_offset + T] += dx[b].float()
    return de, dp


# ---------------------------------------------------------------------------------------------------------------------
# optimizers (one flat tensor, float64)
# ---------------------------------------------------------------------------------------------------------------------
def clip_factor(grad_norm_sq, max_norm: float) -> float:
    """clip_grad_norm_'s factor as the header states it: min(1, max_norm / (sqrt(gsq) + 1e-6)); 1 without a norm."""
    return 1.0 if grad_norm_sq is None else min(1.0, max_norm / (math.sqrt(float(grad_norm_sq)) + 1e-6))


def adamw_step(p, g, m, v, step: int, lr: float, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 0.0,
               grad_norm_sq=None, max_norm: float = 1.0):
    """torch.optim.AdamW's step -> (p, m, v), float64, inputs untouched."""
    b1, b2 = betas
    g = g.double() * clip_factor(grad_norm_sq, max_norm)
    p = p.double() * (1.0 - lr * weight_decay)
    m = b1 * m.double() + (1.0 - b1) * g
    v = b2 * v.double() + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps))
    return p, m, v


def lion_step(p, g, m, lr: float, betas=(0.9, 0.99), weight_decay: float = 0.0, grad_norm_sq=None, max_norm: float = 1.0):
    """lion_pytorch.Lion's step -> (p, m, ambiguous), float64.  ambiguous marks the entries whose update
    u = b1*m + (1-b1)*g is a cancellation to within 1e-5 of its larger term: fp32 arithmetic may give u the other sign there
    (a step of 2*lr the other way), so a comparison at fp32 precision has to leave them out."""
    b1, b2 = betas
    g = g.double() * clip_factor(grad_norm_sq, max_norm)
    m = m.double()
    a, b = b1 * m, (1.0 - b1) * g
    u = a + b
    ambiguous = u.abs() <= 1e-5 * torch.maximum(a.abs(), b.abs())
    p = p.double() * (1.0 - lr * weight_decay) - lr * torch.sign(u)
    return p, b2 * m + (1.0 - b2) * g, ambiguous


# ---------------------------------------------------------------------------------------------------------------------
# element-wise and layout kernels
# ---------------------------------------------------------------------------------------------------------------------
def quick_gelu(x: torch.Tensor) -> torch.Tensor:
    """HF QuickGELUActivation: x * sigmoid(1.702 x), float64."""
    x = x.double()
    return x * torch.sigmoid(1.702 * x)


def quick_gelu_grad(x: torch.Tensor) -> torch.Tensor:
    """d/dx of quick_gelu: s + 1.702 x s (1 - s), s = sigmoid(1.702 x), float64."""
    x = x.double()
    s = torch.sigmoid(1.702 * x)
    return s + 1.702 * x * s * (1.0 - s)


def patchify(pixels: torch.Tensor, patch: int, kpad: int) -> torch.Tensor:
    """pixels [B,3,S,S] -> [B*(S/patch)^2, kpad] in the dtype of pixels: row b*G*G + py*G + px, columns (channel, dy, dx) as
    Conv2d.weight.flatten(1), zero padded to kpad.  A pure copy."""
    B = pixels.shape[0]
    k = 3 * patch * patch
    cols = torch.nn.functional.unfold(pixels, patch, stride=patch)           # [B, 3*patch^2, G*G]
    out = torch.zeros(B * cols.shape[2], kpad, dtype=pixels.dtype)
    out[:, :k] = cols.transpose(1, 2).reshape(-1, k)
    return out


def vit_assemble(patch_out: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, B: int) -> torch.Tensor:
    """cat(class_embedding, patch_out[b]) + position_embedding -> [B, tokens, dim], in the dtype of the inputs (one add
    per element: the fp32 result is the correctly rounded one)."""
    tokens, dim = pos.shape
    return torch.cat([cls.reshape(1, 1, dim).expand(B, 1, dim), patch_out.reshape(B, tokens - 1, dim)], 1) + pos


def add_rowvec(x: torch.Tensor, vec: torch.Tensor) -> torch.Tensor:
    return x + vec


# ---------------------------------------------------------------------------------------------------------------------
# inputs the CPU and the GPU test share (the CPU test checks the conditions the GPU assertions rest on)
# ---------------------------------------------------------------------------------------------------------------------
def _g(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# name -> (B, T, d, vocab).  256 = the number of token positions embed_bwd_kernel scans per chunk.
EMBED_CASES = {
    "three_chunks_heavy_duplicates": (3, 200, 64, 7),
    "full_chunk_one_id": (1, 512, 320, 5),                  # positions 0..255 all id 2; id 3 first at 256; id 4 absent
    "chunk_edge_255_256": (1, 512, 320, 5),                 # positions 0..254 id 2; id 3 at 255 and 256; id 4 absent
    "d_2048": (2, 130, 2048, 1002),
    "d_not_multiple_of_256": (1, 257, 1000, 3),
}


def embed_inputs(name: str):
    """-> (tokens [B,T] int64, dx [B,T,d] fp32, vocab)."""
    B, T, d, vocab = EMBED_CASES[name]
    g = _g(100 + sum(map(ord, name)))
    tok = torch.randint(0, vocab, (B, T), generator=g)
    if name in ("full_chunk_one_id", "chunk_edge_255_256"):
        tok = torch.randint(0, 4, (B, T), generator=g)                       # id 4 never appears
        n2 = 256 if name == "full_chunk_one_id" else 255
        tok[0, :n2] = 2
        tok[0, n2:257] = 3
        tok[0, 257:300] = torch.randint(0, 2, (43,), generator=g)            # a stretch without ids 2 and 3
    return tok, torch.randn(B, T, d, generator=g), vocab


OPT_SIZES = (1, 255, 256, 257, 100003)        # one lane, one short of / exactly / one past a 256-thread block, many blocks
LION_STEPS = 5
LION_HYPER = dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.1, max_norm=1.0)
LION_AMBIGUOUS_CAP = 1e-4                     # at most 0.01 % of the entries may be left out


def f32(x: float) -> float:
    """The value a float argument has once it crossed the C ABI as `float`."""
    return float(np.float32(x))


def lion_inputs(n: int):
    """-> (p0 [n], [g_1 .. g_LION_STEPS]) fp32.  p0 is uniform in (-0.9, 0.9), so that rel_err(p) < 1e-6 is a bound correct
    fp32 arithmetic cannot miss: |p| stays below 0.905 < 1 over five steps of 1e-3, where a rounding of p is at most half an
    ulp = 3e-8; the kernel rounds p at most twice a step (3e-7 over 5 steps at the very worst), its fp32 decay factor
    1 - lr*wd is within 3e-8 of the exact one (1.4e-7 over 5 steps), and p's RMS is 0.52: 8.5e-7.  (Among 1e5 normal values
    some exceed 4 RMS, where half an ulp is 2.4e-7 and five roundings alone may pass 1e-6.)"""
    g = _g(700 + n)
    return torch.rand(n, generator=g) * 1.8 - 0.9, [torch.randn(n, generator=g) * 3 for _ in range(LION_STEPS)]


def norm_sq_f32(g: torch.Tensor) -> torch.Tensor:
    """The squared gradient norm as the float64 sum rounded to fp32 ([1] fp32: what the kernels read from the device)."""
    return (g.double() ** 2).sum().float().reshape(1)


def lion_reference(n: int, clipped: bool = True):
    """The float64 trajectory over lion_inputs(n) -> list of (p, m, ambiguous) per step."""
    h = LION_HYPER
    p, grads = lion_inputs(n)
    p, m = p.double(), torch.zeros(n, dtype=torch.float64)
    out = []
    for gr in grads:
        p, m, amb = lion_step(p, gr, m, f32(h["lr"]), tuple(map(f32, h["betas"])), f32(h["weight_decay"]),
                              float(norm_sq_f32(gr)) if clipped else None, h["max_norm"])
        out.append((p, m, amb))
    return out
