"""train_ref.py checked on the CPU: Philox4x32-10 against its published known answers, the float64 references against
torch's own operators, and the conditions the assertions of test_train_kernels_gpu.py rest on, on that test's inputs."""
import numpy as np
import pytest
import torch

import train_ref as R
from helpers import rel_err


def _g(seed):
    return torch.Generator().manual_seed(seed)


# Random123's kat_vectors for philox4x32 with 10 rounds (counter, key -> output); the third is the "pi" vector
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,out", PHILOX_KAT)
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(w) for w in R.philox4x32_10(ctr, key)[0]) == out
    assert tuple(int(w) for w in R.philox4x32_10(ctr, key, rounds=9)[0]) != out


def test_philox_is_elementwise_over_counter_arrays():
    ctrs = np.array([k[0] for k in PHILOX_KAT], dtype=np.uint64)
    key = PHILOX_KAT[2][1]
    got = R.philox4x32_10(tuple(ctrs[:, j] for j in range(4)), key)
    assert got.shape == (3, 4)
    for i in range(3):
        assert np.array_equal(got[i], R.philox4x32_10(tuple(int(c) for c in ctrs[i]), key)[0])


def test_keep_mask_follows_the_header_definition():
    seed, site = 0x299F31D0A4093822, 0x13198A2E
    # element 4*blk + j of (seed, site) is word j of the block with counter (lo32(blk), hi32(blk), site, 0): with blk = 0x243F6A88
    # that would need 2^31 elements, so the definition is checked on block 1 against a direct call instead
    w = R.philox4x32_10((1, 0, site, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]
    for p in (0.1, 0.5, 0.999):
        t = int(float(np.float32(p)) * 2 ** 32)
        assert R.dropout_thresh(p) == t
        assert np.array_equal(R.keep_mask(7, p, seed, site)[4:7], (w[:3] >= t).astype(np.uint8))
    assert R.dropout_thresh(0.0) == 0 and R.keep_mask(4099, 0.0, 5, 1).all()
    for p in (0.1, 0.25, 0.5):                                                 # keeps 1 - p of the elements (4 sigma)
        kept = R.keep_mask(40000, p, 1234, 7).mean()
        assert abs(kept - (1 - p)) < 4 * np.sqrt(p * (1 - p) / 40000)
    assert not np.array_equal(R.keep_mask(64, 0.5, 1234, 0), R.keep_mask(64, 0.5, 1234 + (1 << 32), 0))    # k1 takes part
    assert not np.array_equal(R.keep_mask(64, 0.5, 1234, 0), R.keep_mask(64, 0.5, 1234, 1))


def test_cross_entropy_matches_torch_float64():
    g = _g(1)
    M, V = 9, 301
    logits = (torch.randn(M, V, generator=g) * 5 + 20).double().requires_grad_()
    tgt = torch.randint(0, V, (M,), generator=g)
    tgt[0], tgt[1], tgt[4] = 0, V - 1, -100
    rows = torch.nn.functional.cross_entropy(logits, tgt, ignore_index=-100, reduction="none")
    (rows.sum() / 36).backward()
    loss, grad = R.cross_entropy(logits.detach().float(), tgt, 1.0 / 36)
    torch.testing.assert_close(loss, rows.detach(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(grad, logits.grad, rtol=1e-13, atol=1e-16)
    assert float(loss[4]) == 0.0 and not grad[4].any()
    tgt[7] = V                                                                 # an id past the vocabulary: ignored too
    loss2, grad2 = R.cross_entropy(logits.detach().float(), tgt, 1.0 / 36)
    assert float(loss2[7]) == 0.0 and not grad2[7].any()
    keep = torch.arange(M) != 7
    assert torch.equal(loss2[keep], loss[keep]) and torch.equal(grad2[keep], grad[keep])


def test_adamw_step_matches_torch_float64():
    g = _g(2)
    n, lr, betas, eps, wd = 1000, 1e-2, (0.9, 0.999), 1e-8, 0.1
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        gr = torch.randn(n, generator=g, dtype=torch.float64) * (3 if step != 3 else 1e-3)     # step 3: below max_norm
        ref.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_([ref], 1.0)
        opt.step()
        p, m, v = R.adamw_step(p, gr, m, v, step, lr, betas, eps, wd, grad_norm_sq=float((gr ** 2).sum()), max_norm=1.0)
        torch.testing.assert_close(p, ref.detach(), rtol=1e-12, atol=1e-14)
    assert R.clip_factor(None, 1.0) == 1.0 and R.clip_factor(1e-6, 1.0) == 1.0


@pytest.mark.parametrize("off", [0, 5])
def test_embed_backward_matches_autograd(off):
    g = _g(3)
    B, T, d, V = 3, 11, 6, 9
    P = T + 9
    tok = torch.randint(0, V, (B, T), generator=g)
    emb = torch.randn(V, d, generator=g, dtype=torch.float64).requires_grad_()
    pos = torch.randn(P, d, generator=g, dtype=torch.float64).requires_grad_()
    dx = torch.randn(B, T, d, generator=g)
    ((emb[tok] + pos[2 + off:2 + off + T][None]) * dx.double()).sum().backward()
    de, dp = R.embed_backward(tok, dx, V, P, off)
    torch.testing.assert_close(de, emb.grad, rtol=1e-14, atol=1e-14)
    torch.testing.assert_close(dp, pos.grad, rtol=1e-14, atol=1e-14)
    de32, dp32 = R.embed_backward_inorder_f32(tok, dx, V, P, off)
    assert de32.dtype == torch.float32 and rel_err(de32, de) < 1e-6 and rel_err(dp32, dp) < 1e-6


def test_patchify_matches_conv2d():
    g = _g(4)
    B, S, ps, kpad, dim = 2, 28, 14, 640, 5
    pixels = torch.randn(B, 3, S, S, generator=g, dtype=torch.float64)
    W = torch.randn(dim, 3, ps, ps, generator=g, dtype=torch.float64)
    rows = R.patchify(pixels, ps, kpad)
    assert rows.shape == (B * 4, kpad) and not rows[:, 3 * ps * ps:].any()
    conv = torch.nn.functional.conv2d(pixels, W, stride=ps)                    # [B, dim, G, G]
    torch.testing.assert_close(rows[:, :3 * ps * ps] @ W.flatten(1).t(), conv.flatten(2).transpose(1, 2).reshape(B * 4, dim),
                               rtol=1e-12, atol=1e-12)


def test_quick_gelu_grad_matches_autograd_and_vit_assemble_matches_its_definition():
    x = (torch.randn(500, generator=_g(5)) * 4).double().requires_grad_()
    (x * torch.sigmoid(1.702 * x)).sum().backward()
    torch.testing.assert_close(R.quick_gelu_grad(x.detach()), x.grad, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(R.quick_gelu(x.detach()), (x * torch.sigmoid(1.702 * x)).detach(), rtol=0, atol=0)
    g = _g(6)
    B, tokens, dim = 2, 5, 8
    po, cls, pos = torch.randn(B * 4, dim, generator=g), torch.randn(dim, generator=g), torch.randn(tokens, dim, generator=g)
    x = R.vit_assemble(po, cls, pos, B)
    for b in range(B):
        assert torch.equal(x[b, 0], cls + pos[0])
        for s in range(1, tokens):
            assert torch.equal(x[b, s], po[b * 4 + s - 1] + pos[s])
    assert torch.equal(R.add_rowvec(po, cls), po + cls[None])


# ---- conditions of the GPU assertions, on the GPU test's own inputs ----
@pytest.mark.parametrize("name", list(R.EMBED_CASES))
def test_embed_inputs_reach_their_paths_and_the_inorder_fp32_sum_meets_the_gpu_bound(name):
    tok, dx, vocab = R.embed_inputs(name)
    B, T, d = dx.shape
    flat = tok.reshape(-1)
    assert B * T > 256 and int(flat.max()) < vocab
    if name == "full_chunk_one_id":
        assert (flat[:256] == 2).all() and int(flat[256]) == 3 and not (flat[:256] == 3).any()
    if name == "chunk_edge_255_256":
        assert (flat[:255] == 2).all() and int(flat[255]) == 3 and int(flat[256]) == 3
    if name in ("full_chunk_one_id", "chunk_edge_255_256"):
        assert not (flat == 4).any()                                           # an absent id: every chunk skipped
        assert not ((flat[257:300] == 2) | (flat[257:300] == 3)).any()
    for off in (0, 5):
        de, dp = R.embed_backward(tok, dx, vocab, T + 9, off)
        de32, dp32 = R.embed_backward_inorder_f32(tok, dx, vocab, T + 9, off)
        assert rel_err(de32, de) < 1e-5 and rel_err(dp32, dp) < 1e-5


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("n", R.OPT_SIZES)
def test_lion_exclusion_rule_stays_under_its_cap(n, clipped):
    left_out = torch.zeros(n, dtype=torch.bool)
    for _, _, amb in R.lion_reference(n, clipped):
        left_out |= amb
    assert int(left_out.sum()) <= R.LION_AMBIGUOUS_CAP * n
