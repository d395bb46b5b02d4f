"""Thin torch-tensor wrappers over the primitive C-ABI ops of libkosmosx_hip.so.

PyTorch is plumbing here (device memory + the current HIP stream); the arithmetic runs in the
hand-written gfx950 kernels.  Every wrapper requires CUDA tensors and raises otherwise.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _hip as H


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("kosmosx ops run on the MI355X HIP path only: tensor is not on a CUDA/HIP device")


def _cdt(dtype) -> int:
    if dtype == torch.float32:
        return H.KX_F32
    if dtype == torch.bfloat16:
        return H.KX_BF16
    if dtype == torch.float16:
        return H.KX_F16
    raise TypeError(f"unsupported dtype {dtype}")


def pack_f16c_rows(x: torch.Tensor) -> torch.Tensor:
    """[rows, K] fp32 -> KX_F16C activation rows [rows, 4K] uint8: [fp16(x) | fp8(x) | fp8((x - fp16(x)) * 2^11)]
    (torch conversions; the device producers write the same bytes — kx_precision in include/kosmosx_hip.h)."""
    x = x.float()
    h = x.clamp(-65504.0, 65504.0).to(torch.float16)     # the fp16 piece saturates (csrc/kx_common.h: clamp_f16)
    e = x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    r = ((x - h.float()) * 2048.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return torch.cat([h.view(torch.uint8).reshape(x.shape[0], -1), e.view(torch.uint8), r.view(torch.uint8)], dim=1).contiguous()


def unpack_f16c_rows(rows: torch.Tensor, K: int):
    """KX_F16C activation rows [rows, 4K] uint8 -> (h, e, r) as fp32 tensors [rows, K] (r still carries its 2^11)."""
    h = rows[:, : 2 * K].contiguous().view(torch.float16).float()
    e = rows[:, 2 * K: 3 * K].contiguous().view(torch.float8_e4m3fn).float()
    r = rows[:, 3 * K: 4 * K].contiguous().view(torch.float8_e4m3fn).float()
    return h, e, r


def layernorm(x, gamma, beta, eps=1e-5, out_dtype=torch.float32, pre_add=None, out=None,
              rows_per_group=None, out_group_stride=0, out_row_offset=0, x3=False, f16c=False):
    """x [rows, cols] fp32 -> LN(x (+pre_add)) * gamma + beta.  x3: KX_BF16X3 rows [hi | hi | lo] ([rows, 3*cols] bf16);
    f16c: KX_F16C rows ([rows, 4*cols] uint8)."""
    _need_cuda(x, gamma, beta, pre_add, out)
    rows, cols = x.shape
    if out is None and f16c:
        out = torch.empty((rows, 4 * cols), dtype=torch.uint8, device=x.device)
    if out is None:
        out = torch.empty((rows, 3 * cols if x3 else cols), dtype=torch.bfloat16 if x3 else out_dtype, device=x.device)
    rc = H.load().kx_layernorm(H.ptr(x), H.ptr(pre_add), H.ptr(gamma), H.ptr(beta), H.ptr(out),
                               H.KX_F16C if f16c else H.KX_BF16X3 if x3 else _cdt(out.dtype),
                               rows, cols, float(eps), rows_per_group or rows, out_group_stride, out_row_offset,
                               _stream())
    H.check(rc, "kx_layernorm")
    return out


def gemm(a, w, bias=None, residual=None, act="none", out_dtype=torch.float32, qscale=1.0, qcols=0,
         xpos=None, xpos_dim=0, tile=0, out=None, row_stats=None, colsum=None, stats_out=None, splitk_ws=None,
         splitk=0, ln=None, stats_partials=None, stats_in_seg=64, stats_eps=1e-5, stats_out_seg=0, out_x3=False,
         ln_out=None, ln_operand=None, w_tiled_rows=0, ksplit=0, out2=None, residual2=None, a_add=None, out_pieces=False,
         a_pieces=False, pair_ws=None, splitk_flags=None):
    """epilogue(a [M,K] @ w[N,K]^T).  a/w both bf16 or both fp32.  xpos = (xq_cs, xq_ss, xk_cs, xk_ss) [T,32].
    tile=16 (weight streaming, bf16, M <= 16) extras: ln = (gamma, beta, eps) with `a` the raw fp32 rows;
    stats_partials [M,nseg,2] instead of row_stats; stats_out_seg=16.
    ln_out = (gamma, beta, eps, dtype) with split-K scratch on a skinny problem: also returns LayerNorm(out) (the
    row-owning reduce kernel); the call then returns (out, ln)."""
    _need_cuda(a, w, bias, residual, out)
    g, out, lnt, lop = _gemm_args(H.ptr, a, w, bias, residual, act, out_dtype, qscale, qcols, xpos, xpos_dim, tile, out, row_stats,
                                  colsum, stats_out, splitk_ws, splitk, ln, stats_partials, stats_in_seg, stats_eps, stats_out_seg,
                                  out_x3, ln_out, ln_operand, w_tiled_rows, ksplit, out2, residual2, a_add, out_pieces, a_pieces,
                                  pair_ws, splitk_flags)
    H.check(H.load().kx_gemm(C.byref(g), _stream()), "kx_gemm")
    if lop is not None:
        return (out,) + lop
    return out if lnt is None else (out, lnt)


def _gemm_args(ptr, a, w, bias, residual, act, out_dtype, qscale, qcols, xpos, xpos_dim, tile, out, row_stats, colsum, stats_out,
               splitk_ws, splitk, ln, stats_partials, stats_in_seg, stats_eps, stats_out_seg, out_x3, ln_out, ln_operand,
               w_tiled_rows, ksplit, out2, residual2, a_add, out_pieces, a_pieces, pair_ws, splitk_flags):
    """kx_gemm_args of a gemm() call and the outputs it allocates; `ptr` turns a tensor into an address (gemm_describe: a fake one)."""
    M, K = a.shape
    N = w_tiled_rows or w.shape[0]                 # w_tiled_rows = N: `w` is tile_weight_rows(W) (tile 16 only)
    prec = H.KX_PREC_BF16 if w.dtype == torch.bfloat16 else H.KX_PREC_F16 if w.dtype == torch.float16 else H.KX_PREC_F32
    if a.dtype != w.dtype and ln is None and w.dtype != torch.uint8:
        raise TypeError("gemm operands must share a dtype")
    if out is None:
        out = torch.empty((M, 3 * N if out_x3 else N), dtype=torch.bfloat16 if out_x3 else out_dtype, device=a.device)
    g = H.GemmArgs()
    g.A, g.lda, g.W, g.ldw = ptr(a), a.stride(0), ptr(w), (K if w_tiled_rows else w.stride(0))
    # uint8 tiles: 24-bit planes (tile_weight_rows_w24, 1536-byte blocks) or block-scaled 16-bit weights (_w16, 1088-byte blocks)
    g.w_tiled = ((3 if w.shape[-1] == 1088 else 2) if w.dtype == torch.uint8 else 1) if w_tiled_rows else 0
    g.C, g.ldc, g.cdt = ptr(out), out.stride(0), (H.KX_BF16X3 if out_x3 else H.KX_F16P if out_pieces else _cdt(out.dtype))
    if a_pieces:                                   # `a` holds KX_F16P rows (f16_pieces_rows, or a producer's out_pieces output)
        assert g.w_tiled == 3, "a_pieces rides on the block-scaled 16-bit planes"
        g.w_tiled = 4
    g.bias, g.residual, g.ldr = ptr(bias), ptr(residual), (residual.stride(0) if residual is not None else 0)
    g.M, g.N, g.K = M, N, K
    g.act, g.qscale, g.qcols = H.ACTS[act], float(qscale), qcols
    if xpos is not None:
        g.xq_cs, g.xq_ss, g.xk_cs, g.xk_ss = (ptr(t) for t in xpos)
        g.xpos_T, g.xpos_dim = xpos[0].shape[0], xpos_dim
    g.prec, g.tile = prec, tile
    g.row_stats, g.colsum, g.stats_out = ptr(row_stats), ptr(colsum), ptr(stats_out)
    if splitk_ws is not None:
        g.splitk_ws, g.splitk_ws_bytes, g.splitk = ptr(splitk_ws), splitk_ws.numel() * splitk_ws.element_size(), splitk
    if pair_ws is not None:         # scratch of the 256x256 kernel's pair split (first 4 KB zero: pair_scratch())
        g.pair_ws, g.pair_ws_bytes = ptr(pair_ws), pair_ws.numel() * pair_ws.element_size()
    if splitk_flags is not None:    # >= 2 x CUs int32 words (splitk_flags()): the split-K launch reduces its partials itself
        g.splitk_flags = ptr(splitk_flags)
    if ln is not None:
        g.ln_gamma, g.ln_beta, g.ln_eps = ptr(ln[0]), ptr(ln[1]), float(ln[2])
    if stats_partials is not None:
        g.stats_partials, g.stats_in_nseg = ptr(stats_partials), stats_partials.shape[1]
        g.stats_in_seg, g.stats_eps = stats_in_seg, float(stats_eps)
        if row_stats is not None and tile != 16:      # tile kernels: `row_stats` is the [M, 2] OUTPUT scratch of the finalize pass (ABI 7)
            g.row_stats, g.row_stats_scratch = None, ptr(row_stats)
    g.stats_out_seg = stats_out_seg
    # tile 16, the residual stream as a pair (kx_gemm_args.ksplit): out2 receives part 1's product
    g.ksplit, g.C2, g.residual2, g.a_add = ksplit, ptr(out2), ptr(residual2), ptr(a_add)
    lnt = None
    if ln_out is not None:
        lnt = torch.empty((M, N), dtype=ln_out[3], device=a.device)
        g.ln_out, g.ln_out_dt = ptr(lnt), _cdt(ln_out[3])
        g.ln_out_gamma, g.ln_out_beta, g.ln_out_eps = ptr(ln_out[0]), ptr(ln_out[1]), float(ln_out[2])
    lop = None
    if ln_operand is not None:      # dtype of the operand copy: torch.bfloat16 / torch.float16 / "f16c"
        lop = _ln_operand_buffers(g, ln_operand, M, N, a.device, ptr)
    return g, out, lnt, lop


def _ln_operand_buffers(g, dt, M, N, device, ptr=H.ptr):
    """Folded pre-LayerNorm producer outputs: (operand copy of the finished rows, partial statistics [M, N/64, 2])."""
    if dt == "f16c":
        cp, g.ln_operand_dt = torch.empty((M, 4 * N), dtype=torch.uint8, device=device), H.KX_F16C
    else:
        cp, g.ln_operand_dt = torch.empty((M, N), dtype=dt, device=device), _cdt(dt)
    st = torch.zeros((M, N // 64, 2), dtype=torch.float32, device=device)
    g.ln_operand_out, g.ln_operand_stats = ptr(cp), ptr(st)
    return cp, st


def tile_weight_rows(w: torch.Tensor) -> torch.Tensor:
    """[N, K] bf16 or fp32 (K % 32 == 0) -> the streaming layout of kx_gemm_args.w_tiled: [ceil(N/16), K/ks, 64, e] with
    e = 16 bytes of values (8 bf16 / 4 fp32) and ks = 4e the k-step; piece l of block (p, c) = row 16p + (l & 15), columns
    ks*c + e*(l >> 4) .. +e-1 — one contiguous 1 KB block per wave load; rows past N are zero.  A copy (torch data movement)."""
    N, K = w.shape
    assert K % 32 == 0 and w.dtype in (torch.bfloat16, torch.float32)
    e = 16 // w.element_size()
    ks = 4 * e
    Np = (N + 15) // 16 * 16
    if Np != N:
        w = torch.cat([w, torch.zeros((Np - N, K), dtype=w.dtype, device=w.device)], 0)
    # [p, i, c, g, e] -> [p, c, g, i, e]: piece index l = g * 16 + i
    return w.view(Np // 16, 16, K // ks, 4, e).permute(0, 2, 3, 1, 4).contiguous().view(Np // 16, K // ks, 64, e)


def round_to_24_bits(w: torch.Tensor) -> torch.Tensor:
    """fp32 -> the nearest (ties to even) fp32 value whose low mantissa byte is zero: 16 significant bits, what the 24-bit
    weight planes of kx_gemm_args.w_tiled = 2 can hold."""
    b = w.detach().float().contiguous().view(torch.int32)
    b = (b + 0x7F + ((b >> 8) & 1)) & ~0xFF
    return b.view(torch.float32)


def tile_weight_rows_w24(w: torch.Tensor) -> torch.Tensor:
    """[N, K] fp32 whose values fit 24 bits (round_to_24_bits), K % 32 == 0 -> kx_gemm_args.w_tiled = 2 planes, uint8
    [ceil(N/16), K/32, 1536]: per block of 16 rows x 32 columns, 64 pieces of 16 B (piece l = row 16p + (l & 15): the bf16
    halves of columns 32c + 4(l >> 4) .. +3, then 32c + 16 + 4(l >> 4) .. +3) followed by 64 pieces of 8 B (their third bytes)."""
    N, K = w.shape
    assert K % 32 == 0 and w.dtype == torch.float32
    bits = w.contiguous().view(torch.int32)
    assert int((bits & 0xFF).abs().max()) == 0, "values must be rounded to 24 bits first (round_to_24_bits)"
    Np = (N + 15) // 16 * 16
    if Np != N:
        bits = torch.cat([bits, torch.zeros((Np - N, K), dtype=torch.int32, device=w.device)], 0)
    # [p, i, c, half, g, j] -> [p, c, g, i, half, j]: piece l = g * 16 + i holds (half, j) = 8 values
    v = bits.view(Np // 16, 16, K // 32, 2, 4, 4).permute(0, 2, 4, 1, 3, 5).contiguous()
    hi = ((v >> 16) & 0xFFFF).to(torch.int16).view(Np // 16, K // 32, 64 * 8).view(torch.uint8)      # little-endian halves
    lo = ((v >> 8) & 0xFF).to(torch.uint8).view(Np // 16, K // 32, 64 * 8)
    return torch.cat([hi.view(Np // 16, K // 32, 1024), lo], dim=2).contiguous()


def quantize_block16(w: torch.Tensor):
    """fp32 [N, K] (K % 32 == 0) -> (q int16 [N, K], scale fp32 [N, K/32], wq fp32 [N, K]): per row and block of 32 columns
    scale = max|w| / 32767 (1 for an all-zero block), q = round(w / scale), wq = q * scale — the values the block-scaled 16-bit
    planes of kx_gemm_args.w_tiled = 3 hold, as the kernel rebuilds them ((float)q * scale, one fp32 rounding)."""
    N, K = w.shape
    assert K % 32 == 0
    wb = w.detach().float().reshape(N, K // 32, 32)
    amax = wb.abs().amax(-1)
    scale = torch.where(amax > 0, amax / 32767.0, torch.ones_like(amax))
    q = torch.round(wb / scale[..., None]).clamp(-32767, 32767).to(torch.int16)
    wq = (q.float() * scale[..., None]).reshape(N, K).contiguous()
    return q.reshape(N, K).contiguous(), scale.contiguous(), wq


def tile_weight_rows_w16(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """(q int16 [N, K], scale fp32 [N, K/32]) -> kx_gemm_args.w_tiled = 3 planes, uint8 [ceil(N/16), K/32, 1088]: per block
    64 pieces of 16 B (piece l = row 16p + (l & 15): columns 32c + 4(l >> 4) .. +3, then 32c + 16 + 4(l >> 4) .. +3) followed
    by the block's 16 row scales."""
    N, K = q.shape
    assert K % 32 == 0 and q.dtype == torch.int16 and scale.shape == (N, K // 32)
    Np = (N + 15) // 16 * 16
    if Np != N:
        q = torch.cat([q, torch.zeros((Np - N, K), dtype=q.dtype, device=q.device)], 0)
        scale = torch.cat([scale, torch.ones((Np - N, K // 32), dtype=scale.dtype, device=scale.device)], 0)
    v = q.view(Np // 16, 16, K // 32, 2, 4, 4).permute(0, 2, 4, 1, 3, 5).contiguous()          # [p, c, g, i, half, j]
    qb = v.view(Np // 16, K // 32, 64 * 8).view(torch.uint8).view(Np // 16, K // 32, 1024)
    sb = scale.float().view(Np // 16, 16, K // 32).permute(0, 2, 1).contiguous().view(torch.uint8).view(Np // 16, K // 32, 64)
    return torch.cat([qb, sb], dim=2).contiguous()


def f16_pieces_rows(x: torch.Tensor) -> torch.Tensor:
    """fp32 [M, K] (K % 32 == 0) -> KX_F16P rows as an fp32-typed [M, K] tensor: value = hi + lo, hi = fp16(x) toward zero
    (saturating at 65504), lo = fp16(x - hi); per 32 values [hi: 4 chunks of (4g..4g+3, 16+4g..16+4g+3) | lo: the same]."""
    M, K = x.shape
    assert K % 32 == 0 and x.dtype == torch.float32
    xc = x.clamp(-65504.0, 65504.0)
    h = xc.to(torch.float16)
    over = h.float().abs() > xc.abs()                                 # round-to-nearest went away from zero: one step back
    h = torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)
    lo = (x - h.float()).to(torch.float16)

    def order(t):                                                     # [M, K/32, half, g, j] -> [M, K/32, g, half, j]
        return t.reshape(M, K // 32, 2, 4, 4).permute(0, 1, 3, 2, 4).reshape(M, K // 32, 32)
    return torch.cat([order(h), order(lo)], dim=2).contiguous().view(torch.float32).reshape(M, K)


def f16_pieces_values(rows: torch.Tensor) -> torch.Tensor:
    """KX_F16P rows (fp32-typed [M, K]) -> the fp32 values hi + lo they stand for."""
    M, K = rows.shape
    p = rows.contiguous().view(torch.float16).reshape(M, K // 32, 2, 4, 2, 4).float()      # [M, blk, piece, g, half, j]
    v = p[:, :, 0] + p[:, :, 1]
    return v.permute(0, 1, 3, 2, 4).reshape(M, K)


def gemm_f16c(a_rows, w_packed, N, K, bias=None, residual=None, act="none", out_f16c=False, qscale=1.0, qcols=0,
              xpos=None, xpos_dim=0, tile=0, row_stats=None, colsum=None, stats_out=None, splitk_ws=None, splitk=0,
              ln_operand=None, pair_ws=None, out_hilo=False, stats_partials=None, stats_in_seg=64, stats_eps=1e-5, corr="both",
              splitk_flags=None):
    """KX_PREC_F16C GEMM: a_rows [M, 4K] uint8 (KX_F16C activation rows), w_packed = the flat packed weight matrix
    (N rows of 4K bytes + N scale bytes, model._operand_f16c).  Output fp32 [M, N] or KX_F16C rows [M, 4N] uint8.
    out_hilo (with xpos): the fp32-shaped output holds KX_F16HL head slots — [64 fp16 hi | 64 fp16 lo] of 2^8 x per 64 columns."""
    _need_cuda(a_rows, w_packed, bias, residual)
    g, out, lop = _gemm_f16c_args(H.ptr, a_rows, w_packed, N, K, bias, residual, act, out_f16c, qscale, qcols, xpos, xpos_dim, tile,
                                  row_stats, colsum, stats_out, splitk_ws, splitk, ln_operand, pair_ws, out_hilo, stats_partials,
                                  stats_in_seg, stats_eps, corr, splitk_flags)
    H.check(H.load().kx_gemm(C.byref(g), _stream()), "kx_gemm")
    return out if lop is None else (out,) + lop


def _gemm_f16c_args(ptr, a_rows, w_packed, N, K, bias, residual, act, out_f16c, qscale, qcols, xpos, xpos_dim, tile, row_stats,
                    colsum, stats_out, splitk_ws, splitk, ln_operand, pair_ws, out_hilo, stats_partials, stats_in_seg, stats_eps,
                    corr, splitk_flags):
    """kx_gemm_args of a gemm_f16c() call and the outputs it allocates (see _gemm_args)."""
    M = a_rows.shape[0]
    assert a_rows.dtype == torch.uint8 and a_rows.shape[1] == 4 * K and w_packed.numel() >= N * 4 * K + N
    out = (torch.empty((M, 4 * N), dtype=torch.uint8, device=a_rows.device) if out_f16c else
           torch.empty((M, N), dtype=torch.float32, device=a_rows.device))
    g = H.GemmArgs()
    g.A, g.lda, g.W, g.ldw = ptr(a_rows), a_rows.stride(0) // 2, ptr(w_packed), 2 * K
    g.C, g.ldc, g.cdt = ptr(out), (2 * N if out_f16c else out.stride(0)), (H.KX_F16C if out_f16c else H.KX_F16HL if out_hilo else H.KX_F32)
    g.w_scale = ptr(w_packed) + N * 4 * K
    g.bias, g.residual, g.ldr = ptr(bias), ptr(residual), (residual.stride(0) if residual is not None else 0)
    g.M, g.N, g.K = M, N, K
    g.act, g.qscale, g.qcols = H.ACTS[act], float(qscale), qcols
    if xpos is not None:
        g.xq_cs, g.xq_ss, g.xk_cs, g.xk_ss = (ptr(t) for t in xpos)
        g.xpos_T, g.xpos_dim = xpos[0].shape[0], xpos_dim
    g.prec, g.tile = H.KX_PREC_F16C, tile
    g.row_stats, g.colsum, g.stats_out = ptr(row_stats), ptr(colsum), ptr(stats_out)
    if stats_partials is not None:      # with row_stats (the OUTPUT scratch, kx_gemm_args.row_stats_scratch): finalised by kx_gemm's own pass
        g.stats_partials, g.stats_in_nseg = ptr(stats_partials), stats_partials.shape[1]
        g.stats_in_seg, g.stats_eps = stats_in_seg, float(stats_eps)
        if row_stats is not None:
            g.row_stats, g.row_stats_scratch = None, ptr(row_stats)
    g.f16c_corr = {"both": 0, "weight": 1, "act": 2, "none": 3}[corr]
    if splitk_ws is not None:
        g.splitk_ws, g.splitk_ws_bytes, g.splitk = ptr(splitk_ws), splitk_ws.numel() * splitk_ws.element_size(), splitk
    if pair_ws is not None:
        g.pair_ws, g.pair_ws_bytes = ptr(pair_ws), pair_ws.numel() * pair_ws.element_size()
    if splitk_flags is not None:
        g.splitk_flags = ptr(splitk_flags)
    lop = _ln_operand_buffers(g, ln_operand, M, N, a_rows.device, ptr) if ln_operand is not None else None
    return g, out, lop


def gemm_describe(*args, cu_count=0, **kw):
    """What kx_gemm would launch for a gemm(...) call — or, with (a_rows, w_packed, N, K, ...), a gemm_f16c(...) call — without
    launching anything: the same positional and keyword arguments, tensors on any device (`meta` tensors do; no operand is read).
    cu_count: the CU count to plan for (0 = the current device's, 256 without one).  Returns the parsed lines: a list of launches
    {"kernel", "args", "grid", "block"} (the finalize and weight-streaming launches carry their family name only) and the
    dict of the resolved tile and host flags.  A call kx_gemm would refuse raises with the same code and message."""
    def ptr(t):      # operands are never dereferenced: real addresses where there are any, else one fake 1 MB-aligned address
        return None if t is None else (t.data_ptr() if t.device.type != "meta" else 1 << 20)
    import inspect
    rows = args[0] if args else kw.get("a_rows")             # KX_F16C activation rows are uint8: gemm_f16c's form
    fn, build = (gemm_f16c, _gemm_f16c_args) if rows is not None and rows.dtype == torch.uint8 else (gemm, _gemm_args)
    b = inspect.signature(fn).bind(*args, **kw)
    b.apply_defaults()
    g = build(ptr, **b.arguments)[0]
    buf = C.create_string_buffer(4096)
    H.check(H.load().kx_gemm_describe(C.byref(g), int(cu_count), buf, len(buf)), "kx_gemm_describe")
    return parse_gemm_description(buf.value.decode())


def parse_gemm_description(text):
    """kx_gemm_describe's text -> (launches, plan)."""
    import re
    launches, plan = [], {}
    for line in text.strip().splitlines():
        if line.startswith("plan "):
            plan = {k: int(v) for k, v in (f.split("=") for f in line.split()[1:])}
            continue
        m = re.fullmatch(r"(\w+)<(.*)> grid=(\d+)x(\d+) block=(\d+)(?: lds=(\d+))?", line)
        if m is None:
            launches.append({"kernel": line})
        else:
            launches.append({"kernel": m.group(1), "args": [a.strip() for a in m.group(2).split(",")],
                             "grid": [int(m.group(3)), int(m.group(4))], "block": int(m.group(5))})
            if m.group(6) is not None:       # (a kernel trace's static + dynamic bytes: tests/golden/gemm_plan.json)
                launches[-1]["lds"] = int(m.group(6))
    return launches, plan


def pair_scratch(device="cuda", workgroups=256):
    """kx_gemm_args.pair_ws: 4 KB of hand-off words (zero now, zero again after every completed call) + one 128 KB slab per
    workgroup of the pair split."""
    return torch.zeros(4096 + workgroups * 131072, dtype=torch.uint8, device=device)


def set_objective(name: str) -> None:
    """Scheduling objective of the library's automatic kernel choice (kx_set_tuning key 18): "latency" (default; every launch
    chosen to finish soonest alone on the chip — one step at a time) or "throughput" (the caller keeps two or more steps in flight
    on separate streams: fewest CU-microseconds per launch).  Results are bit-identical either way."""
    v = {"latency": 0, "throughput": 1}[name]
    if H.load().kx_set_tuning(18, v) != 0:
        raise RuntimeError("kx_set_tuning(18) refused")


def splitk_flags(device="cuda"):
    """kx_gemm_args.splitk_flags: one word per workgroup of an in-launch split-K reduction (2 per CU), cleared once."""
    return torch.zeros(1024, dtype=torch.int32, device=device)


def pair_split_errors() -> int:
    """kx_pair_split_errors: 0 when every pair-split hand-off since the last call met its partner, else 1 + the index of the
    last workgroup whose bounded poll gave up (the word is cleared).  Synchronises the device: diagnostics only."""
    import ctypes
    w = ctypes.c_uint(0)
    H.check(H.load().kx_pair_split_errors(ctypes.byref(w)), "kx_pair_split_errors")
    return int(w.value)


def row_stats_finalize(partials, seg_size, eps=1e-5):
    """partials [rows, nseg, 2] (sum, M2 about the segment mean) -> [rows, 2] (mean, rstd)."""
    _need_cuda(partials)
    rows, nseg, _ = partials.shape
    out = torch.empty((rows, 2), dtype=torch.float32, device=partials.device)
    H.check(H.load().kx_row_stats_finalize(H.ptr(partials), rows, nseg, seg_size, float(eps), H.ptr(out), _stream()),
            "kx_row_stats_finalize")
    return out


def attention(q, k, v, causal=False, out_dtype=None, stats_out=None, out_x3=False, lse_out=None, f16c=False,
              out_f16c=False, dropout=None, hilo=False):
    """q [B,Tq,H,64], k/v [B,Tk,H,64] (any row/batch strides, last two dims contiguous) -> [B,Tq,H*64]
    (out_x3, fp32 inputs only: KX_BF16X3 rows [hi | hi | lo], [B,Tq,3*H*64] bf16).
    f16c (fp32 inputs): the KX_PREC_F16C kernel — split fp16 (hi, lo) products; out_f16c: KX_F16C rows [B,Tq,4*H*64] uint8."""
    _need_cuda(q, k, v)
    B, Tq, Hh, hd = q.shape
    Tk = k.shape[1]
    assert hd == 64 and q.stride(3) == 1 and q.stride(2) == 64 and k.stride(2) == 64 and v.stride(2) == 64
    assert k.stride(0) == v.stride(0) and k.stride(1) == v.stride(1)
    prec = (H.KX_PREC_BF16 if q.dtype == torch.bfloat16 else H.KX_PREC_F16 if q.dtype == torch.float16
            else (H.KX_PREC_F16CHL if hilo else H.KX_PREC_F16C if f16c or out_f16c else H.KX_PREC_F32))   # hilo: fp32-typed KX_F16HL rows
    out = (torch.empty((B, Tq, 4 * Hh * 64), dtype=torch.uint8, device=q.device) if out_f16c else
           torch.empty((B, Tq, 3 * Hh * 64), dtype=torch.bfloat16, device=q.device) if out_x3 else
           torch.empty((B, Tq, Hh * 64), dtype=out_dtype or q.dtype, device=q.device))
    a = H.AttnArgs()
    a.q, a.q_batch_stride, a.q_row_stride = H.ptr(q), q.stride(0), q.stride(1)
    a.k, a.v, a.kv_batch_stride, a.kv_row_stride = H.ptr(k), H.ptr(v), k.stride(0), k.stride(1)
    a.out, a.out_batch_stride, a.out_row_stride = H.ptr(out), out.stride(0), out.stride(1)
    if out_f16c:                                   # strides count 2-byte units
        a.out_batch_stride, a.out_row_stride = out.stride(0) // 2, out.stride(1) // 2
    a.odt = H.KX_F16C if out_f16c else H.KX_BF16X3 if out_x3 else _cdt(out.dtype)
    a.B, a.H, a.Tq, a.Tk = B, Hh, Tq, Tk
    a.mask, a.prec = (H.KX_ATTN_CAUSAL if causal else H.KX_ATTN_FULL), prec
    a.stats_out = H.ptr(stats_out)
    a.lse_out = H.ptr(lse_out)
    if dropout is not None:                        # (p, seed, site): attention dropout of the training step, fp32 only
        a.dropout_p, a.dropout_seed, a.dropout_site = float(dropout[0]), int(dropout[1]), int(dropout[2])
    H.check(H.load().kx_attention(C.byref(a), _stream()), "kx_attention")
    return out


def embed_splice(tokens, embed, pos, img=None, u1_alias=True, splice_at=2, pos_offset=0):
    """Decoder input assembly (see kx_embed_splice in include/kosmosx_hip.h)."""
    _need_cuda(tokens, embed, pos, img)
    if tokens is not None:
        B, Tt = tokens.shape
    else:
        B, Tt = img.shape[0], 0
    n_img = 0 if img is None else img.shape[1]
    d = embed.shape[1]
    out = torch.empty((B, Tt + n_img, d), dtype=torch.float32, device=embed.device)
    rc = H.load().kx_embed_splice(H.ptr(tokens), H.ptr(embed), H.ptr(pos), H.ptr(img), H.ptr(out), B, Tt, n_img, d,
                                  embed.shape[0], pos.shape[0], splice_at, int(u1_alias), pos_offset, _stream())
    H.check(rc, "kx_embed_splice")
    return out


def token_range(tokens, out=None):
    """Kernel-level wrapper (the model calls the library directly; this is what the kernel tests and tools drive).
    kx_token_range: (min, max) of the int64 ``tokens`` on the device -> int64 [2] (``out``: a buffer to reuse; the launcher
    initialises it)."""
    _need_cuda(tokens, out)
    if tokens.dtype != torch.int64 or not tokens.is_contiguous():
        raise TypeError("token_range: tokens must be a contiguous int64 tensor")
    if out is None:
        out = torch.empty(2, dtype=torch.int64, device=tokens.device)
    H.check(H.load().kx_token_range(tokens.data_ptr(), tokens.numel(), out.data_ptr(), _stream()), "kx_token_range")
    return out


class SampleRowTable:
    """Per-row sampling options in the form kx_sample_logits_rows reads, the counterpart of BiasTable: B kx_sample_row records in
    device memory (``table``, uint8 [B * 56]) and the launch summary ``flags`` kx_sample_rows_pack returned for them
    (H.SAMPLE_ROWS_PENALTY: some row has a repetition penalty; H.SAMPLE_ROWS_BUDGET: some row has a budget).
    ``rows``: B dicts naming any of do_sample, temperature, top_k, top_p, repetition_penalty, min_p, typical_p, epsilon_cutoff,
    eta_cutoff, seed and max_new_tokens (0 = no budget); what a dict leaves out is switched off (a row without ``do_sample`` is
    greedy).  ``V``: the vocabulary the table is for.  Packed on the host by the library (ValueError naming the row and the field for
    what it refuses), uploaded once; built once per generate() call and passed to every ops.sample_logits of the loop."""
    FIELDS = ("do_sample", "temperature", "top_k", "top_p", "repetition_penalty", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff",
              "seed", "max_new_tokens")

    def __init__(self, rows, V, device):
        rows = list(rows)
        if not rows:
            raise ValueError("SampleRowTable: rows must hold at least one record")
        rec = (H.SampleRow * len(rows))()
        for b, r in enumerate(rows):
            unknown = set(r) - set(self.FIELDS)
            if unknown:
                raise ValueError(f"SampleRowTable: rows[{b}] names {sorted(unknown)}, not among {self.FIELDS}")
            kw = {k: (float(v) if isinstance(getattr(rec[b], k), float) else int(v)) for k, v in r.items() if k not in ("seed", "max_new_tokens")}
            rec[b] = H.SampleRow(seed=int(r.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF, max_new=int(r.get("max_new_tokens", 0)), **kw)
        got = C.c_uint32(0)
        rc = H.load().kx_sample_rows_pack(rec, len(rows), int(V), rec, C.byref(got))
        if rc != 0:
            raise ValueError(f"SampleRowTable: {H.last_error()}")
        self.B, self.V, self.flags = len(rows), int(V), int(got.value)
        self.host = rec                                                   # the packed records (log_min_p filled in)
        self.table = torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8).to(device)


def sample_logits(logits, *, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, do_sample=True, seed=0,
                  position=0, sequence_ids=None, history=None, hist_len=0, finished=None, eos_token_id=None,
                  pad_token_id=1, return_debug=False, out=None, out_tokens=None, out_col=0, positions=None, advance=0, min_p=0.0,
                  typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, rows=None, kept_count=None):
    """Next token of every row of fp32 `logits` [B, V] (row stride >= V), drawn on the device by one launch
    (kx_sample_logits in include/kosmosx_hip.h: repetition penalty -> temperature -> top-k -> top-p -> Gumbel-max draw
    addressed by (seed, sequence id, position); greedy when ``do_sample`` is false or ``temperature`` is 0).

    history [B, >= hist_len + 1] int64: the ids the repetition penalty looks at; the new token is appended at column
    ``hist_len``.  finished [B] uint8 (in/out): finished rows emit ``pad_token_id``, a row that draws ``eos_token_id``
    becomes finished.  out [B] int64 / out_tokens [B, n] int64 with ``out_col``: caller-owned places for the result.
    positions [B] int32 (device, in/out): the ragged form (kx_sample_logits_ragged) — row b draws at Philox position
    ``positions[b] + advance`` and, when ``advance`` is not 0, leaves that value in ``positions[b]``; ``position`` is unused.
    min_p in [0, 1] (0 = off: the two entry points above are called as before): after top-p, keep only x_i >= x_max + log(min_p)
    (kx_sample_logits_min_p, either form); ignored under greedy.
    typical_p in (0, 1] (1 = off), epsilon_cutoff and eta_cutoff in [0, 1) (0 = off; with all three off the entry points above are
    called as before): the `transformers` truncation samplers, behind min-p in that order, each over what the one before it kept
    (kx_sample_logits_truncate, either form); ignored under greedy.
    rows (a SampleRowTable of B records, or None): row b is sampled under its own record — do_sample, temperature, top_k, top_p,
    repetition_penalty, min_p, the three cut-offs and the seed of this call are then ignored — and a row whose record has a budget
    max_new becomes finished by the launch with ``out_col`` + 1 >= max_new (kx_sample_logits_rows, either form; ``finished`` is then
    required).  Row b gets the bits of a one-row call with its record's values.
    kept_count [B] int32 (device, out): a caller-owned place for the size of the set every row drew from — ``return_debug``'s count
    without its mask; 0 for a row that entered the launch finished or had no candidate.
    Returns next_token [B] int64 (and kept_count [B] int32, keep_mask [B, V] uint8 with ``return_debug``)."""
    _need_cuda(logits, sequence_ids, history, finished, out, out_tokens, positions, kept_count)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise TypeError("sample_logits: logits must be fp32 [B, V] with unit column stride")
    for name, t, dt in (("sequence_ids", sequence_ids, torch.int64), ("history", history, torch.int64),
                        ("finished", finished, torch.uint8), ("out", out, torch.int64), ("out_tokens", out_tokens, torch.int64),
                        ("positions", positions, torch.int32), ("kept_count", kept_count, torch.int32)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise TypeError(f"sample_logits: {name} must be a contiguous {dt} tensor")
    B, V = logits.shape
    for name, t in (("sequence_ids", sequence_ids), ("finished", finished), ("out", out), ("positions", positions),
                    ("kept_count", kept_count)):
        if t is not None and tuple(t.shape) != (B,):
            raise ValueError(f"sample_logits: {name} must have shape [{B}]")
    for name, t in (("history", history), ("out_tokens", out_tokens)):
        if t is not None and (t.dim() != 2 or t.shape[0] != B):
            raise ValueError(f"sample_logits: {name} must be [{B}, n]")
    if out is None:
        out = torch.empty(B, dtype=torch.int64, device=logits.device)
    a = H.SampleArgs()
    a.do_sample = int(bool(do_sample))
    a.logits, a.ld, a.B, a.V = logits.data_ptr(), (logits.stride(0) if B > 1 else max(logits.stride(0), V)), B, V
    a.temperature, a.top_k, a.top_p, a.repetition_penalty = float(temperature), int(top_k), float(top_p), float(repetition_penalty)
    a.seed, a.position = int(seed) & 0xFFFFFFFFFFFFFFFF, int(position)
    a.sequence_ids = H.ptr(sequence_ids)
    a.history, a.hist_ld, a.hist_len = H.ptr(history), (0 if history is None else history.shape[1]), int(hist_len)
    a.finished = H.ptr(finished)
    a.eos_id, a.pad_id = (-1 if eos_token_id is None else int(eos_token_id)), int(pad_token_id)
    a.next_token = out.data_ptr()
    a.out_tokens, a.out_ld, a.out_col = H.ptr(out_tokens), (0 if out_tokens is None else out_tokens.shape[1]), int(out_col)
    kept = mask = None
    if kept_count is not None:
        a.kept_count = kept_count.data_ptr()
    if return_debug:
        kept = kept_count if kept_count is not None else torch.empty(B, dtype=torch.int32, device=logits.device)
        mask = torch.empty((B, V), dtype=torch.uint8, device=logits.device)
        a.kept_count, a.keep_mask = kept.data_ptr(), mask.data_ptr()
    if rows is not None:
        if not isinstance(rows, SampleRowTable):
            raise TypeError(f"sample_logits: rows must be an ops.SampleRowTable (or None), got {type(rows).__name__}")
        _need_cuda(rows.table)
        if rows.B != B or rows.V != V:
            raise ValueError(f"sample_logits: rows holds {rows.B} records for a vocabulary of {rows.V}, logits are [{B}, {V}]")
        if positions is not None:
            a.position = 0
        r = H.SampleRowsArgs(flags=rows.flags, table=rows.table.data_ptr())
        H.check(H.load().kx_sample_logits_rows(C.byref(a), H.ptr(positions), int(advance) if positions is not None else 0, C.byref(r),
                                               _stream()), "kx_sample_logits_rows")
        return (out, kept, mask) if return_debug else out
    min_p = float(min_p)
    if not 0.0 <= min_p <= 1.0:
        raise ValueError(f"sample_logits: min_p = {min_p} must be in [0, 1]")
    typical_p, epsilon_cutoff, eta_cutoff = float(typical_p), float(epsilon_cutoff), float(eta_cutoff)
    if not 0.0 < typical_p <= 1.0:
        raise ValueError(f"sample_logits: typical_p = {typical_p} must be in (0, 1]")
    for name, v in (("epsilon_cutoff", epsilon_cutoff), ("eta_cutoff", eta_cutoff)):
        if not 0.0 <= v < 1.0:
            raise ValueError(f"sample_logits: {name} = {v} must be in [0, 1)")
    if typical_p != 1.0 or epsilon_cutoff != 0.0 or eta_cutoff != 0.0:
        if positions is not None:
            a.position = 0
        t = H.TruncateArgs(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
        H.check(H.load().kx_sample_logits_truncate(C.byref(a), H.ptr(positions), int(advance) if positions is not None else 0,
                                                   C.byref(t), _stream()), "kx_sample_logits_truncate")
    elif min_p != 0.0:
        if positions is not None:
            a.position = 0
        H.check(H.load().kx_sample_logits_min_p(C.byref(a), H.ptr(positions), int(advance) if positions is not None else 0, min_p,
                                                _stream()), "kx_sample_logits_min_p")
    elif positions is not None:
        a.position = 0
        H.check(H.load().kx_sample_logits_ragged(C.byref(a), positions.data_ptr(), int(advance), _stream()), "kx_sample_logits_ragged")
    else:
        H.check(H.load().kx_sample_logits(C.byref(a), _stream()), "kx_sample_logits")
    return (out, kept, mask) if return_debug else out


class SequenceTable:
    """A list of token-id sequences (``bad_words_ids`` / ``stop_sequences``) in the CSR form kx_constrain_logits reads: ``ids``
    int64 and ``off`` int32 [n + 1] on the device, and the host copy of the offsets the library checks the limits on.  Built
    once per generate() call (the one upload), passed to every ops.constrain_logits of the loop."""

    def __init__(self, sequences, device):
        seqs = [[int(t) for t in s] for s in sequences]
        off = [0]
        for s in seqs:
            off.append(off[-1] + len(s))
        self.n = len(seqs)
        self.off_host = (C.c_int32 * len(off))(*off)
        self.ids = torch.tensor([t for s in seqs for t in s] or [0], dtype=torch.int64, device=device)
        self.off = torch.tensor(off, dtype=torch.int32, device=device)


def constrain_logits(logits, *, history=None, hist_len=0, prompt_width=0, prompt_lens=None, new_tokens=0, no_repeat_ngram_size=0,
                     bad_words=None, stop_sequences=None, min_new_tokens=0, eos_token_id=None, finished=None):
    """Ban ids in every row of fp32 `logits` [B, V] (row stride >= V) IN PLACE, by one launch, before ops.sample_logits or
    ops.beam_step reads them (kx_constrain_logits in include/kosmosx_hip.h): a banned id's logit becomes -inf, nothing else is
    written.  No-repeat n-gram of size ``no_repeat_ngram_size``, ``bad_words`` and the minimum length (``eos_token_id`` is banned
    while ``new_tokens`` < ``min_new_tokens``); a row whose sequence ends in one of ``stop_sequences`` after at least one new token
    becomes finished and gets no bans.

    history [B, > hist_len] int64: the buffer the sampler appends to, ``hist_len`` columns in use.  prompt_lens [B] int32 (device)
    with ``prompt_width``: the ragged form — row b's sequence is columns [0, prompt_lens[b]) then [prompt_width, hist_len).
    ``bad_words`` / ``stop_sequences``: SequenceTable.  finished [B] uint8 (in/out): finished rows are left untouched.  Returns None."""
    for name, t in (("bad_words", bad_words), ("stop_sequences", stop_sequences)):
        if t is not None and not isinstance(t, SequenceTable):
            raise TypeError(f"constrain_logits: {name} must be an ops.SequenceTable (or None), got {type(t).__name__}")
    bad_t = None if bad_words is None else (bad_words.ids, bad_words.off)
    stop_t = None if stop_sequences is None else (stop_sequences.ids, stop_sequences.off)
    _need_cuda(logits, history, prompt_lens, finished, *(bad_t or ()), *(stop_t or ()))
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise TypeError("constrain_logits: logits must be fp32 [B, V] with unit column stride")
    for name, t, dt in (("history", history, torch.int64), ("prompt_lens", prompt_lens, torch.int32), ("finished", finished, torch.uint8)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise TypeError(f"constrain_logits: {name} must be a contiguous {dt} tensor")
    B, V = logits.shape
    for name, t in (("prompt_lens", prompt_lens), ("finished", finished)):
        if t is not None and tuple(t.shape) != (B,):
            raise ValueError(f"constrain_logits: {name} must have shape [{B}]")
    if history is not None and (history.dim() != 2 or history.shape[0] != B):
        raise ValueError(f"constrain_logits: history must be [{B}, n]")
    if history is None and int(hist_len) != 0:
        raise ValueError(f"constrain_logits: hist_len = {hist_len} needs a history")
    if history is not None and not 0 <= int(hist_len) < history.shape[1]:
        raise ValueError(f"constrain_logits: hist_len = {hist_len} outside [0, {history.shape[1]}): history has {history.shape[1]} "
                         "columns and the sampler appends one after this launch")
    if prompt_lens is not None and not 0 <= int(prompt_width) <= int(hist_len):
        raise ValueError(f"constrain_logits: prompt_width = {prompt_width} outside [0, hist_len = {hist_len}]")
    a = H.ConstrainArgs()
    a.ngram = int(no_repeat_ngram_size)
    a.logits, a.ld, a.B, a.V = logits.data_ptr(), (logits.stride(0) if B > 1 else max(logits.stride(0), V)), B, V
    a.history, a.hist_ld, a.hist_len = H.ptr(history), (0 if history is None else history.shape[1]), int(hist_len)
    a.prompt_width, a.prompt_lens = int(prompt_width), H.ptr(prompt_lens)
    a.new_tokens, a.min_new = int(new_tokens), int(min_new_tokens)
    a.eos_id = -1 if eos_token_id is None else int(eos_token_id)
    if bad_words is not None and bad_words.n:
        a.bad_ids, a.bad_off, a.n_bad = bad_words.ids.data_ptr(), bad_words.off.data_ptr(), bad_words.n
        a.bad_off_host = C.cast(bad_words.off_host, C.c_void_p)
    if stop_sequences is not None and stop_sequences.n:
        a.stop_ids, a.stop_off, a.n_stop = stop_sequences.ids.data_ptr(), stop_sequences.off.data_ptr(), stop_sequences.n
        a.stop_off_host = C.cast(stop_sequences.off_host, C.c_void_p)
    a.finished = H.ptr(finished)
    H.check(H.load().kx_constrain_logits(C.byref(a), _stream()), "kx_constrain_logits")


class AutomatonTable:
    """A token automaton in the CSR form kx_automaton_step reads, the counterpart of SequenceTable: ``edge_off`` int32 [S + 1],
    ``edge_tok`` / ``edge_next`` int32 [E] and ``default_next`` int32 [S] on the device (TokenAutomaton.tables() makes them; raw
    arrays are taken as they are — the kernel range-checks what it reads).  Built once per generate() call (the one upload), passed
    to every ops.automaton_step of the loop."""

    def __init__(self, edge_off, edge_tok, edge_next, default_next, device):
        host = [torch.as_tensor(t, dtype=torch.int32).reshape(-1).cpu() for t in (edge_off, edge_tok, edge_next, default_next)]
        self.S, self.E = int(host[3].numel()), int(host[1].numel())
        if self.S < 1:
            raise ValueError("AutomatonTable: default_next is empty: an automaton has at least one state")
        if host[0].numel() != self.S + 1:
            raise ValueError(f"AutomatonTable: edge_off must have {self.S + 1} entries (states + 1), got {host[0].numel()}")
        if host[2].numel() != self.E:
            raise ValueError(f"AutomatonTable: edge_next must have {self.E} entries (one per edge_tok), got {host[2].numel()}")
        # (an empty tensor has no storage to point at: one unused word keeps the pointers valid; E stays 0)
        self.edge_off, self.edge_tok, self.edge_next, self.default_next = (
            (t if t.numel() else torch.zeros(1, dtype=torch.int32)).to(device).contiguous() for t in host)


def automaton_step(logits, table, state_in, state_out, *, src_row=None, last_token=None, finished=None):
    """Advance every row's automaton state and ban what the new state does not allow in fp32 `logits` [B, V] (row stride >= V) IN
    PLACE, by one launch, before ops.sample_logits or ops.beam_step reads them (kx_automaton_step in include/kosmosx_hip.h): a
    banned id's logit becomes -inf, nothing else is written.

    ``table``: AutomatonTable.  state_in int32 [B_in] / state_out int32 [B]: two buffers that do not overlap.  src_row int32 [B]:
    row b comes from state_in[src_row[b]] (beams); without it B_in == B.  last_token int64 [B]: the token the state advances on
    (None at step 0: mask only).  finished uint8 [B] (read only): finished rows carry their state over and keep their logits.
    Returns None."""
    if not isinstance(table, AutomatonTable):
        raise TypeError(f"automaton_step: table must be an ops.AutomatonTable, got {type(table).__name__}")
    _need_cuda(logits, state_in, state_out, src_row, last_token, finished, table.edge_off, table.edge_tok, table.edge_next,
               table.default_next)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise TypeError("automaton_step: logits must be fp32 [B, V] with unit column stride")
    for name, t, dt in (("state_in", state_in, torch.int32), ("state_out", state_out, torch.int32), ("src_row", src_row, torch.int32),
                        ("last_token", last_token, torch.int64), ("finished", finished, torch.uint8)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous()):
            raise TypeError(f"automaton_step: {name} must be a contiguous {dt} tensor")
    for name, t in (("state_in", state_in), ("state_out", state_out)):
        if t is None:
            raise TypeError(f"automaton_step: {name} must be a contiguous {torch.int32} tensor, got None")
    B, V = logits.shape
    for name, t in (("state_out", state_out), ("src_row", src_row), ("last_token", last_token), ("finished", finished)):
        if t is not None and tuple(t.shape) != (B,):
            raise ValueError(f"automaton_step: {name} must have shape [{B}]")
    if state_in.dim() != 1 or state_in.shape[0] < 1 or (src_row is None and state_in.shape[0] != B):
        raise ValueError(f"automaton_step: state_in must have shape [{B}]" + (" (any length >= 1 with a src_row)" if src_row is not None else "")
                         + f", got {tuple(state_in.shape)}")
    a = H.AutomatonArgs()
    a.logits, a.ld, a.B, a.V = logits.data_ptr(), (logits.stride(0) if B > 1 else max(logits.stride(0), V)), B, V
    a.edge_off, a.edge_tok, a.edge_next, a.default_next = (t.data_ptr() for t in (table.edge_off, table.edge_tok, table.edge_next,
                                                                                  table.default_next))
    a.S, a.E = table.S, table.E
    a.state_in, a.B_in, a.state_out = state_in.data_ptr(), state_in.shape[0], state_out.data_ptr()
    a.src_row, a.last_token, a.finished = H.ptr(src_row), H.ptr(last_token), H.ptr(finished)
    H.check(H.load().kx_automaton_step(C.byref(a), _stream()), "kx_automaton_step")


SHAPE_SLICE = 4096                      # ids per workgroup of kx_shape_logits (what its tests place their edges at)


class BiasTable:
    """Per-row logit biases in the CSR form kx_shape_logits reads, the counterpart of SequenceTable / AutomatonTable: ``off`` int32
    [B + 1], ``ids`` int32 ascending within a row and ``val`` fp32 on the device.  ``rows``: B sequences of (id, value) pairs (a
    dict's items() will do; they are sorted by id here).  Raw arrays are taken as they are with ``BiasTable.raw`` — the kernel
    range-checks what it reads.  Built once per generate() call (the one upload), passed to every ops.shape_logits of the loop."""

    def __init__(self, rows, device):
        rows = [sorted((int(i), float(v)) for i, v in (r.items() if hasattr(r, "items") else r)) for r in rows]
        off = [0]
        for r in rows:
            off.append(off[-1] + len(r))
        self._set(off, [i for r in rows for i, _ in r], [v for r in rows for _, v in r], device)

    def _set(self, off, ids, val, device):
        host = (torch.as_tensor(off, dtype=torch.int32).reshape(-1).cpu(), torch.as_tensor(ids, dtype=torch.int32).reshape(-1).cpu(),
                torch.as_tensor(val, dtype=torch.float32).reshape(-1).cpu())
        if host[0].numel() < 2:
            raise ValueError("BiasTable: off must have B + 1 >= 2 entries")
        if host[1].numel() != host[2].numel():
            raise ValueError(f"BiasTable: {host[1].numel()} ids but {host[2].numel()} values")
        self.B, self.n = int(host[0].numel()) - 1, int(host[1].numel())
        # (an empty tensor has no storage to point at: one unused word keeps the pointers valid; n stays 0)
        self.off, self.ids, self.val = ((t if t.numel() else torch.zeros(1, dtype=t.dtype)).to(device).contiguous() for t in host)

    @classmethod
    def raw(cls, off, ids, val, device):
        t = cls.__new__(cls)
        t._set(off, ids, val, device)
        return t


def shape_logits(logits, *, bias=None, counts=None, frequency_penalty=0.0, presence_penalty=0.0, last_token=None, finished=None,
                 frequency_rows=None, presence_rows=None):
    """Logit bias and presence / frequency penalties on every row of fp32 `logits` [B, V] (row stride >= V) IN PLACE, by one launch,
    after ops.constrain_logits / ops.automaton_step and before ops.sample_logits reads them (kx_shape_logits in
    include/kosmosx_hip.h): counts[b, last_token[b]] += 1, then l = l + bias for the listed ids, then where the count c is
    positive l = (l - frequency_penalty * c) - presence_penalty, each a single fp32 operation; -inf and NaN logits stay.

    ``bias``: BiasTable of B rows (or None).  counts int32 [B, V] (in/out; None when both penalties are 0): how often this call
    emitted each id, zeroed by the caller before the first step.  last_token int64 [B]: the sampler's token of the previous step
    (None at step 0).  finished uint8 [B] (read only): finished rows keep their logits and their counts.
    frequency_rows / presence_rows fp32 [B] (device; either may be None: the scalar for every row): row b's own penalties in the
    same three operations (kx_shape_logits_rows; ``counts`` is then required).  With both None the call is kx_shape_logits.
    Returns None."""
    if bias is not None and not isinstance(bias, BiasTable):
        raise TypeError(f"shape_logits: bias must be an ops.BiasTable (or None), got {type(bias).__name__}")
    _need_cuda(logits, counts, last_token, finished, *((bias.off, bias.ids, bias.val) if bias is not None else ()))
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise TypeError("shape_logits: logits must be fp32 [B, V] with unit column stride")
    _need_cuda(frequency_rows, presence_rows)
    for name, t, dt in (("counts", counts, torch.int32), ("last_token", last_token, torch.int64), ("finished", finished, torch.uint8),
                        ("frequency_rows", frequency_rows, torch.float32), ("presence_rows", presence_rows, torch.float32)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous()):
            raise TypeError(f"shape_logits: {name} must be a contiguous {dt} tensor")
    B, V = logits.shape
    for name, t in (("last_token", last_token), ("finished", finished), ("frequency_rows", frequency_rows), ("presence_rows", presence_rows)):
        if t is not None and tuple(t.shape) != (B,):
            raise ValueError(f"shape_logits: {name} must have shape [{B}]")
    if counts is not None and tuple(counts.shape) != (B, V):
        raise ValueError(f"shape_logits: counts must have shape [{B}, {V}], got {tuple(counts.shape)}")
    if bias is not None and bias.B != B:
        raise ValueError(f"shape_logits: bias has {bias.B} rows, logits {B}")
    a = H.ShapeArgs()
    a.logits, a.ld, a.B, a.V = logits.data_ptr(), (logits.stride(0) if B > 1 else max(logits.stride(0), V)), B, V
    if bias is not None:
        a.bias_off, a.bias_ids, a.bias_val, a.n_bias = bias.off.data_ptr(), bias.ids.data_ptr(), bias.val.data_ptr(), bias.n
    a.counts, a.frequency, a.presence = H.ptr(counts), float(frequency_penalty), float(presence_penalty)
    a.last_token, a.finished = H.ptr(last_token), H.ptr(finished)
    if frequency_rows is None and presence_rows is None:
        H.check(H.load().kx_shape_logits(C.byref(a), _stream()), "kx_shape_logits")
    else:
        H.check(H.load().kx_shape_logits_rows(C.byref(a), H.ptr(frequency_rows), H.ptr(presence_rows), _stream()), "kx_shape_logits_rows")


def guidance_logits(cond, uncond, *, scale, out=None, finished=None, positions=None, advance=0):
    """Classifier-free guidance on B pairs of raw fp32 rows `cond` / `uncond` [B, V] (unit column stride, any row stride >= V) by one
    launch, in front of ops.constrain_logits / ops.automaton_step / ops.shape_logits and ops.sample_logits (kx_guidance_logits in
    include/kosmosx_hip.h): out = lu + scale * (lc - lu) over the rows' log-softmaxes lc and lu — kx_token_logprob's arithmetic,
    then a subtract, a multiply and an add in fp32; a result that is not finite becomes -inf.

    ``out`` fp32 [B, V]: None or ``cond`` itself writes the guided rows over the conditional ones (in place); it never overlaps
    ``uncond``.  finished uint8 [B] (read only): finished pairs are neither read nor written.  positions int32 [B] (in/out) with
    ``advance`` 0 or 1: the unconditional rows' device positions, moved on by ``advance`` for every pair, finished ones included —
    what the ragged sampler launch does for the conditional rows.  Returns ``out``."""
    if out is None:
        out = cond
    _need_cuda(cond, uncond, out, finished, positions)
    for name, t in (("cond", cond), ("uncond", uncond), ("out", out)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1:
            raise TypeError(f"guidance_logits: {name} must be fp32 [B, V] with unit column stride")
    B, V = cond.shape
    for name, t in (("uncond", uncond), ("out", out)):
        if tuple(t.shape) != (B, V):
            raise ValueError(f"guidance_logits: {name} must have shape [{B}, {V}], got {tuple(t.shape)}")
    for name, t, dt in (("finished", finished, torch.uint8), ("positions", positions, torch.int32)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous()):
            raise TypeError(f"guidance_logits: {name} must be a contiguous {dt} tensor")
        if t is not None and tuple(t.shape) != (B,):
            raise ValueError(f"guidance_logits: {name} must have shape [{B}]")
    a = H.GuidanceArgs()
    ld = [t.stride(0) if B > 1 else max(t.stride(0), V) for t in (cond, uncond, out)]
    a.cond, a.ld_cond, a.uncond, a.ld_uncond, a.out, a.ld_out = cond.data_ptr(), ld[0], uncond.data_ptr(), ld[1], out.data_ptr(), ld[2]
    a.B, a.V, a.scale = B, V, float(scale)
    a.finished, a.positions, a.advance = H.ptr(finished), H.ptr(positions), int(advance)
    H.check(H.load().kx_guidance_logits(C.byref(a), _stream()), "kx_guidance_logits")
    return out


def embed_step(tokens, embed, pos, pos_a, pos_b=-1):
    """Kernel-level wrapper (the model calls the library directly; this is what the kernel tests and tools drive).
    kx_embed_step: [B, d] fp32 rows embed[tokens[b]] + pos[2 + pos_a] (+ pos[2 + pos_b]) for int64 ``tokens`` [B] on the device."""
    _need_cuda(tokens, embed, pos)
    B, d = tokens.shape[0], embed.shape[1]
    out = torch.empty((B, d), dtype=torch.float32, device=embed.device)
    H.check(H.load().kx_embed_step(tokens.data_ptr(), embed.data_ptr(), pos.data_ptr(), out.data_ptr(), B, d, embed.shape[0],
                                   pos.shape[0], int(pos_a), int(pos_b), _stream()), "kx_embed_step")
    return out


def step_prepare(tokens, embed, pos, positions, tables=None, pos_shift=0, error_word=None, out=None, xpos_rows=None):
    """kx_step_prepare, the start of a ragged decode step: per row b the embedding of ``tokens[b]`` (int64 [B]) at position
    ``positions[b]`` (int32 [B], device; with ``pos_shift`` the two rows positions[b] - pos_shift and positions[b]) and row
    positions[b] of each of the four XPos ``tables`` ([n, 32] fp32) gathered into [4, B, 32].  A position outside the tables
    sets KX_RAGGED_ERR_TABLE in ``error_word`` (int32 [1], sticky) and leaves that row untouched.
    Returns (x [B, d], xpos_rows [4, B, 32] or None, error_word)."""
    _need_cuda(tokens, embed, pos, positions, error_word, out, xpos_rows, *(tables or ()))
    if positions.dtype != torch.int32 or not positions.is_contiguous() or tokens.dtype != torch.int64:
        raise TypeError("step_prepare: tokens must be int64 and positions a contiguous int32 tensor")
    B, d = tokens.shape[0], embed.shape[1]
    if error_word is None:
        error_word = torch.zeros(1, dtype=torch.int32, device=embed.device)
    if out is None:                                    # (zeros: a rejected row is not written)
        out = torch.zeros((B, d), dtype=torch.float32, device=embed.device)
    tp, n = (0, 0, 0, 0), 0
    if tables is not None:
        n = tables[0].shape[0]
        if any(t.dtype != torch.float32 or tuple(t.shape) != (n, 32) or not t.is_contiguous() for t in tables):
            raise TypeError("step_prepare: tables are four contiguous fp32 [n, 32] tensors")
        tp = tuple(t.data_ptr() for t in tables)
        if xpos_rows is None:
            xpos_rows = torch.zeros((4, B, 32), dtype=torch.float32, device=embed.device)
    H.check(H.load().kx_step_prepare(tokens.data_ptr(), embed.data_ptr(), pos.data_ptr(), positions.data_ptr(), *tp,
                                     out.data_ptr(), H.ptr(xpos_rows if tables is not None else None), B, d, embed.shape[0],
                                     pos.shape[0], int(pos_shift), n, error_word.data_ptr(), _stream()), "kx_step_prepare")
    return out, (xpos_rows if tables is not None else None), error_word


def _decode_attention_args(fn, qkv, kcache, vcache, layout, out_dtype, positions, error_word, K=None, cache_seq=None):
    """What the three decode-attention wrappers share: the caches' layout, the shape / dtype checks (``fn`` names the wrapper in
    every message), the output rows and the kernel's precision.  K None: one row per cache sequence; else K rows per sequence, or
    per candidate of ``cache_seq``.  Returns (cache sequences, H, Tmax, rows, odt, out, prec)."""
    if layout not in ("head_major", "row_major"):
        raise ValueError(f"{fn}: layout is 'head_major' or 'row_major'")
    if layout == "row_major":
        B, Tmax, Hh, hd = kcache.shape
    else:
        B, Hh, Tmax, hd = kcache.shape
    if cache_seq is not None and (cache_seq.dtype != torch.int32 or cache_seq.dim() != 1 or not cache_seq.is_contiguous()):
        raise TypeError(f"{fn}: cache_seq must be a contiguous int32 [C] tensor")
    M = B if K is None else (B if cache_seq is None else cache_seq.shape[0]) * K
    rows, seqs = ("B" if K is None else "B*K", "B") if cache_seq is None else ("C*K", "Bc")
    if hd != 64 or vcache.shape != kcache.shape or tuple(qkv.shape) != (M, 3 * Hh * 64) or not (qkv.is_contiguous() and kcache.is_contiguous() and vcache.is_contiguous()):
        raise ValueError(f"{fn}: qkv [{rows}, 3*H*64], caches [{seqs}, H, Tmax, 64] ([{seqs}, Tmax, H, 64] row-major), contiguous")
    if qkv.dtype != kcache.dtype or kcache.dtype != vcache.dtype or qkv.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{fn}: qkv and the caches share one dtype, fp32 or bf16")
    if positions is not None:
        if positions.dtype != torch.int32 or tuple(positions.shape) != (M,) or not positions.is_contiguous():
            raise TypeError(f"{fn}: positions must be a contiguous int32 [{M}] tensor")
        if error_word is None or error_word.dtype != torch.int32 or error_word.numel() != 1:
            raise TypeError(f"{fn}: {'positions need error_word, an' if K is None else 'error_word is an'} int32 [1] tensor on the "
                            "device (the kernel's sticky word)")
    D = Hh * 64
    odt = {"f32": H.KX_F32, "bf16": H.KX_BF16, "f16c": H.KX_F16C, "f16p": H.KX_F16P}[out_dtype]
    if out_dtype == "f16c":
        out = torch.zeros((M, 4 * D), dtype=torch.uint8, device=qkv.device)
    else:
        out = torch.zeros((M, D), dtype=torch.bfloat16 if out_dtype == "bf16" else torch.float32, device=qkv.device)
    prec = H.KX_PREC_BF16 if qkv.dtype == torch.bfloat16 else (H.KX_PREC_F16C if out_dtype == "f16c" else H.KX_PREC_F32)
    return B, Hh, Tmax, M, odt, out, prec


def attention_decode(qkv, kcache, vcache, t=None, *, positions=None, error_word=None, out_dtype="f32", stats_out=None,
                     layout="head_major"):
    """Kernel-level wrapper (the model calls the library directly; this is what the kernel tests and tools drive).
    The decode step's single-query attention + cache append (kx_attention_decode / kx_attention_decode_ragged).
    qkv [B, 3 * H * 64] fp32 or bf16 rows of the new token; kcache / vcache [B, H, Tmax, 64] of the same dtype (updated in place).
    ``t``: every sequence at host position t; ``positions`` [B] int32 on the device: sequence b at positions[b], a position
    outside the cache sets KX_RAGGED_ERR_CACHE in ``error_word`` (int32 [1], sticky).  out_dtype "f32" | "bf16" | "f16c" | "f16p"
    (the KX_F16C / KX_F16P operand rows of the fp32 step).  Returns the attention output rows.
    ``layout`` "row_major": the caches are [B, Tmax, H, 64], the layout the library reads under tuning key 9 = 1.  The argument
    only names the shape that is checked; the caller sets the key (kx_set_tuning(9, 1)) around the call."""
    _need_cuda(qkv, kcache, vcache, positions, error_word, stats_out)
    B, Hh, Tmax, _, odt, out, prec = _decode_attention_args("attention_decode", qkv, kcache, vcache, layout, out_dtype, positions, error_word)
    lib = H.load()
    if positions is None:
        if t is None:
            raise TypeError("attention_decode: give the host position t or the device positions")
        H.check(lib.kx_attention_decode(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), odt,
                                        H.ptr(stats_out), B, Hh, int(t), Tmax, prec, _stream()), "kx_attention_decode")
        return out
    H.check(lib.kx_attention_decode_ragged(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), odt,
                                           H.ptr(stats_out), B, Hh, positions.data_ptr(), Tmax, prec, error_word.data_ptr(),
                                           _stream()), "kx_attention_decode_ragged")
    return out


def attention_decode_block(qkv, kcache, vcache, positions, error_word, *, rows_per_sequence, out_dtype="f32", stats_out=None,
                           layout="head_major"):
    """Kernel-level wrapper of kx_attention_decode_block (include/kosmosx_hip.h, "Speculative decoding by prompt lookup"): the
    decode attention over B * K rows of which K = ``rows_per_sequence`` consecutive ones belong to one cache sequence, at
    consecutive positions.  qkv [B * K, 3 * H * 64] fp32 or bf16; kcache / vcache [B, H, Tmax, 64] ([B, Tmax, H, 64] with
    ``layout`` "row_major", as ops.attention_decode) of the same dtype, updated in place; positions [B * K] int32 on the device;
    error_word int32 [1] (sticky: KX_RAGGED_ERR_CACHE for a row outside the cache or off its sequence's base + j).
    One launch = K successive ops.attention_decode(positions=...) launches, bit for bit.  Returns the output rows [B * K, ...]."""
    _need_cuda(qkv, kcache, vcache, positions, error_word, stats_out)
    K = int(rows_per_sequence)
    B, Hh, Tmax, _, odt, out, prec = _decode_attention_args("attention_decode_block", qkv, kcache, vcache, layout, out_dtype, positions,
                                                            error_word, K)
    H.check(H.load().kx_attention_decode_block(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), odt,
                                               H.ptr(stats_out), B, K, Hh, positions.data_ptr(), Tmax, prec, error_word.data_ptr(),
                                               _stream()), "kx_attention_decode_block")
    return out


def attention_decode_shared(qkv, kcache, vcache, positions, cache_seq, error_word, *, rows_per_candidate, out_dtype="f32",
                            stats_out=None, layout="head_major"):
    """Kernel-level wrapper of kx_attention_decode_shared (include/kosmosx_hip.h, "Scoring candidates over a shared prompt cache"):
    ops.attention_decode_block's rows with C candidates of K = ``rows_per_candidate`` rows, candidate c reading cache sequence
    cache_seq[c] and nobody appending.  qkv [C * K, 3 * H * 64] fp32 or bf16; kcache / vcache [Bc, H, Tmax, 64] ([Bc, Tmax, H, 64]
    with ``layout`` "row_major", as ops.attention_decode) of the same dtype, left untouched; positions [C * K] and cache_seq [C] int32
    on the device; error_word int32 [1] (sticky: KX_RAGGED_ERR_CACHE for a row outside the cache, off its candidate's base + j or
    with a cache sequence outside [0, Bc)).  The bits of the block launch on a cache replicated per candidate.  Returns the output
    rows [C * K, ...]."""
    _need_cuda(qkv, kcache, vcache, positions, cache_seq, error_word, stats_out)
    K = int(rows_per_candidate)
    Bc, Hh, Tmax, M, odt, out, prec = _decode_attention_args("attention_decode_shared", qkv, kcache, vcache, layout, out_dtype, positions,
                                                             error_word, K, cache_seq)
    H.check(H.load().kx_attention_decode_shared(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), odt,
                                                H.ptr(stats_out), M // K, K, Hh, positions.data_ptr(), cache_seq.data_ptr(), Bc, Tmax,
                                                prec, error_word.data_ptr(), _stream()), "kx_attention_decode_shared")
    return out


def attention_decode_prefix(qkv, kprefix, vprefix, ktail, vtail, positions, prefix_seq, prefix_len, error_word, *, out_dtype="f32",
                            stats_out=None, layout="head_major"):
    """Kernel-level wrapper of kx_attention_decode_prefix (include/kosmosx_hip.h, "Decoding rows over a shared, read-only prefix
    cache"): ops.attention_decode's ragged rows, row r reading keys 0 .. prefix_len[r] - 1 from sequence prefix_seq[r] of the prefix
    caches and the keys after them from sequence r of the tail caches, to which the new k / v are appended at row
    positions[r] - prefix_len[r].  qkv [M, 3 * H * 64] fp32 or bf16; kprefix / vprefix [Bp, H, Tmax, 64] (left untouched) and ktail /
    vtail [M, H, Ttail, 64] of the same dtype ([.., T, H, 64] with ``layout`` "row_major", as ops.attention_decode); positions,
    prefix_seq and prefix_len [M] int32 on the device; error_word int32 [1] (sticky: KX_RAGGED_ERR_CACHE for a row whose prefix
    sequence, prefix length or tail row is outside its cache — that row writes nothing).  The bits of the ragged launch on a private
    cache assembled from the prefix and tail rows.  Returns the output rows [M, ...]."""
    _need_cuda(qkv, kprefix, vprefix, ktail, vtail, positions, prefix_seq, prefix_len, error_word, stats_out)
    fn = "attention_decode_prefix"
    M, Hh, Ttail, _, odt, out, prec = _decode_attention_args(fn, qkv, ktail, vtail, layout, out_dtype, positions, error_word)
    Bp, a, b, hd = kprefix.shape
    Tmax, Hp = (a, b) if layout == "row_major" else (b, a)
    if hd != 64 or Hp != Hh or vprefix.shape != kprefix.shape or not (kprefix.is_contiguous() and vprefix.is_contiguous()):
        raise ValueError(f"{fn}: prefix caches [Bp, H, Tmax, 64] ([Bp, Tmax, H, 64] row-major) with the tails' H, contiguous")
    if kprefix.dtype != qkv.dtype or vprefix.dtype != qkv.dtype:
        raise TypeError(f"{fn}: qkv and the caches share one dtype, fp32 or bf16")
    for name, w in (("prefix_seq", prefix_seq), ("prefix_len", prefix_len)):
        if w.dtype != torch.int32 or tuple(w.shape) != (M,) or not w.is_contiguous():
            raise TypeError(f"{fn}: {name} must be a contiguous int32 [{M}] tensor")
    H.check(H.load().kx_attention_decode_prefix(qkv.data_ptr(), kprefix.data_ptr(), vprefix.data_ptr(), ktail.data_ptr(),
                                                vtail.data_ptr(), out.data_ptr(), odt, H.ptr(stats_out), M, Hh, positions.data_ptr(),
                                                prefix_seq.data_ptr(), prefix_len.data_ptr(), Bp, Tmax, Ttail, prec,
                                                error_word.data_ptr(), _stream()), "kx_attention_decode_prefix")
    return out


def attention_extend(qkv, kcache, vcache, P, *, out_dtype="f32", stats_out=None, layout="head_major", f16c=False):
    """Kernel-level wrapper of kx_attention_extend (include/kosmosx_hip.h, "Chunked prefill"): Tn new rows per sequence on top of
    caches that hold ``P`` rows (a host int, the same for every sequence).  qkv [B * Tn, 3 * H * 64] fp32 or bf16, row b * Tn + i the
    i-th new token of sequence b; kcache / vcache [B, H, Tmax, 64] ([B, Tmax, H, 64] with ``layout`` "row_major", as
    ops.attention_decode) of the same dtype: rows P .. P + Tn - 1 are appended, query i attends rows 0 .. P + i.  out_dtype "f32" |
    "bf16" | "f16c" (KX_F16C rows: the split-fp16 kernel; ``f16c`` asks for that kernel with an fp32 output); stats_out
    [B * Tn, H, 2] fp32 optional.  Returns the output rows [B * Tn, ...]."""
    _need_cuda(qkv, kcache, vcache, stats_out)
    B = kcache.shape[0]
    if B < 1 or qkv.dim() != 2 or qkv.shape[0] % B:
        raise ValueError("attention_extend: qkv [B*Tn, 3*H*64] holds the same number of new rows for each of the caches' B sequences")
    Tn = qkv.shape[0] // B
    B, Hh, Tmax, _, odt, out, prec = _decode_attention_args("attention_extend", qkv, kcache, vcache, layout, out_dtype, None, None, Tn)
    if f16c and prec == H.KX_PREC_F32:
        prec = H.KX_PREC_F16C
    H.check(H.load().kx_attention_extend(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), odt,
                                         H.ptr(stats_out), B, Hh, Tn, int(P), Tmax, prec, _stream()), "kx_attention_extend")
    return out


def attention_extend_ragged(qkv, kcache, vcache, positions, error_word, *, out_dtype="f32", stats_out=None, layout="head_major",
                            f16c=False, out=None):
    """Kernel-level wrapper of kx_attention_extend_ragged (include/kosmosx_hip.h, "Ragged extend"): ops.attention_extend with a
    per-sequence P on the device.  positions [B] int32: sequence b's caches hold positions[b] rows; its Tn rows are appended at
    positions[b] .. + Tn - 1.  error_word int32 [1] (sticky: KX_RAGGED_ERR_CACHE for a sequence whose rows leave the cache — that
    sequence writes nothing).  ``out``: the rows to write into instead of fresh zeros (a guarded sequence leaves its rows as they
    were).  Sequence b gives the bits of a B = 1 ops.attention_extend at P = positions[b].  Returns the output rows [B * Tn, ...]."""
    _need_cuda(qkv, kcache, vcache, positions, error_word, stats_out, out)
    B = kcache.shape[0]
    if B < 1 or qkv.dim() != 2 or qkv.shape[0] % B:
        raise ValueError("attention_extend_ragged: qkv [B*Tn, 3*H*64] holds the same number of new rows for each of the caches' B sequences")
    Tn = qkv.shape[0] // B
    if positions is None or positions.dtype != torch.int32 or tuple(positions.shape) != (B,) or not positions.is_contiguous():
        raise TypeError(f"attention_extend_ragged: positions must be a contiguous int32 [{B}] tensor")
    if error_word is None or error_word.dtype != torch.int32 or error_word.numel() != 1:
        raise TypeError("attention_extend_ragged: error_word is an int32 [1] tensor on the device (the kernel's sticky word)")
    B, Hh, Tmax, _, odt, fresh, prec = _decode_attention_args("attention_extend_ragged", qkv, kcache, vcache, layout, out_dtype, None, None, Tn)
    if out is None:
        out = fresh
    elif out.shape != fresh.shape or out.dtype != fresh.dtype or not out.is_contiguous():
        raise TypeError(f"attention_extend_ragged: out must be a contiguous {fresh.dtype} {tuple(fresh.shape)} tensor")
    if f16c and prec == H.KX_PREC_F32:
        prec = H.KX_PREC_F16C
    H.check(H.load().kx_attention_extend_ragged(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), odt,
                                                H.ptr(stats_out), B, Hh, Tn, positions.data_ptr(), Tmax, prec, error_word.data_ptr(),
                                                _stream()), "kx_attention_extend_ragged")
    return out


def token_logprob(logits, target, *, row_index=None, vocab=None, out=None):
    """Kernel-level wrapper of kx_token_logprob (include/kosmosx_hip.h, "Scoring candidates over a shared prompt cache"):
    out[r] = log softmax(logits[row_index[r], :V])[target[r]] in one launch, no softmax written.  logits fp32 [rows_available, ld]
    with unit column stride (a row pitch ld >= V; ``vocab`` = V, default the row's width); target int64 [R]; ``row_index`` int32 [R]
    or None (row r).  A target outside [0, V) or a row index outside the buffer gives exactly 0.0.  Returns fp32 [R]."""
    _need_cuda(logits, target, row_index, out)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise TypeError("token_logprob: logits is an fp32 [rows, ld] tensor with unit column stride")
    V = logits.shape[1] if vocab is None else int(vocab)
    if target.dtype != torch.int64 or target.dim() != 1 or not target.is_contiguous():
        raise TypeError("token_logprob: target is a contiguous int64 [R] tensor")
    R = target.shape[0]
    if row_index is None:
        if R != logits.shape[0]:
            raise ValueError(f"token_logprob: {R} targets for {logits.shape[0]} rows need a row_index")
    elif row_index.dtype != torch.int32 or tuple(row_index.shape) != (R,) or not row_index.is_contiguous():
        raise TypeError(f"token_logprob: row_index is a contiguous int32 [{R}] tensor")
    if out is None:
        out = torch.empty(R, dtype=torch.float32, device=logits.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (R,) or not out.is_contiguous():
        raise TypeError(f"token_logprob: out is a contiguous fp32 [{R}] tensor")
    H.check(H.load().kx_token_logprob(logits.data_ptr(), logits.shape[0], V, logits.stride(0), H.ptr(row_index), target.data_ptr(),
                                      out.data_ptr(), R, _stream()), "kx_token_logprob")
    return out


def step_logprobs(logits, token, *, out, col, skip=None, top_n=0, top_out=None, top_ids=None):
    """Kernel-level wrapper of kx_step_logprobs (include/kosmosx_hip.h, "Per-token log-probs of a generation step"): one launch
    writes out[b, col] = log softmax(logits[b])[token[b]] and, with ``top_n`` > 0, the row's top_n (log-prob, id) pairs — value
    descending, the lowest id first among equal values — into top_out[b, col] / top_ids[b, col].  logits fp32 [B, V] with unit
    column stride (any row pitch >= V); token int64 [B]; ``out`` fp32 [B, N] contiguous, ``col`` in [0, N); ``skip`` uint8 [B] or
    None: rows that get exact zeros (ids -1) and read no logits; ``top_out`` fp32 / ``top_ids`` int64 [B, N, top_n] contiguous.
    A token outside [0, V) gives exactly 0.0.  Nothing but column ``col`` is written.  Returns ``out``."""
    _need_cuda(logits, token, out, skip, top_out, top_ids)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise TypeError("step_logprobs: logits is a non-empty fp32 [B, V] tensor with unit column stride")
    B, V = logits.shape
    if B > 1 and logits.stride(0) < V:
        raise TypeError(f"step_logprobs: logits rows overlap (row stride {logits.stride(0)} < V = {V})")
    if token.dtype != torch.int64 or tuple(token.shape) != (B,) or not token.is_contiguous():
        raise TypeError(f"step_logprobs: token is a contiguous int64 [{B}] tensor")
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or not out.is_contiguous():
        raise TypeError(f"step_logprobs: out is a contiguous fp32 [{B}, N] tensor")
    N = out.shape[1]
    if isinstance(col, bool) or not isinstance(col, int) or not 0 <= col < N:
        raise ValueError(f"step_logprobs: col = {col!r} is outside the {N} columns of out")
    if skip is not None and (skip.dtype != torch.uint8 or tuple(skip.shape) != (B,) or not skip.is_contiguous()):
        raise TypeError(f"step_logprobs: skip is a contiguous uint8 [{B}] tensor")
    if isinstance(top_n, bool) or not isinstance(top_n, int) or not 0 <= top_n <= 16:
        raise ValueError(f"step_logprobs: top_n = {top_n!r} is outside 0..16")
    if top_n > 0:
        for name, t, dt in (("top_out", top_out, torch.float32), ("top_ids", top_ids, torch.int64)):
            if t is None or t.dtype != dt or tuple(t.shape) != (B, N, top_n) or not t.is_contiguous():
                raise TypeError(f"step_logprobs: {name} is a contiguous {dt} [{B}, {N}, {top_n}] tensor")
    H.check(H.load().kx_step_logprobs(logits.data_ptr(), logits.stride(0) if B > 1 else max(logits.stride(0), V), B, V,
                                      token.data_ptr(), H.ptr(skip), out.data_ptr(), N, col, top_n,
                                      H.ptr(top_out) if top_n else 0, H.ptr(top_ids) if top_n else 0, _stream()), "kx_step_logprobs")
    return out


def spec_accept(picked, *, fed=None, rows_per_sequence, positions, prefill_len=0, history, hist_len, out_tokens, n_out, finished,
                next_tokens, max_new_tokens, step, ngram_max=2, eos_token_id=None, pad_token_id=1, out_src=None, emitted=None,
                draft_from=None):
    """The accept-and-draft launch of a speculative verify step (kx_spec_accept in include/kosmosx_hip.h).  ``picked`` int64
    [B * Kin]: the greedy picks of the step's logits block, Kin = 1 (the prefill's row; ``fed`` unused, ``prefill_len`` read) or
    K = ``rows_per_sequence``; ``fed`` int64 [B * Kin]: what those rows were fed.  Per sequence it accepts the drafts the picks
    confirm, appends the emitted tokens to ``out_tokens`` [B, >= max_new_tokens] / ``history`` [B, n] (int64) and advances
    ``n_out`` / ``hist_len`` [B] and ``positions`` [B * K] (int32), keeps ``finished`` [B] uint8, and writes the next block's
    tokens to ``next_tokens`` int64 [B * K]: the last emitted token, then drafts from ``draft_from`` int64 [B, n] (per output
    slot) or from the lookup of the sequence's last n-gram (n <= ``ngram_max``) in its own history.  Optional ``out_src`` int32
    [B, out_ld] and ``emitted`` int32 [B, >= step + 1].  Everything stays on the device.  Returns None."""
    _need_cuda(picked, fed, positions, history, hist_len, out_tokens, n_out, finished, next_tokens, out_src, emitted, draft_from)
    K = int(rows_per_sequence)
    for name, t, dt in (("picked", picked, torch.int64), ("fed", fed, torch.int64), ("positions", positions, torch.int32),
                        ("history", history, torch.int64), ("hist_len", hist_len, torch.int32), ("out_tokens", out_tokens, torch.int64),
                        ("n_out", n_out, torch.int32), ("finished", finished, torch.uint8), ("next_tokens", next_tokens, torch.int64),
                        ("out_src", out_src, torch.int32), ("emitted", emitted, torch.int32), ("draft_from", draft_from, torch.int64)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise TypeError(f"spec_accept: {name} must be a contiguous {dt} tensor")
    B = finished.shape[0]
    Kin = picked.numel() // max(B, 1)
    if picked.dim() != 1 or picked.numel() != B * Kin or Kin not in (1, K):
        raise ValueError(f"spec_accept: picked must be [B] or [B * {K}] for B = {B}")
    if Kin == K and (fed is None or tuple(fed.shape) != (B * K,)):
        raise ValueError(f"spec_accept: fed must be [{B * K}] alongside picked [{B * K}]")
    for name, t, shape in (("positions", positions, (B * K,)), ("next_tokens", next_tokens, (B * K,)), ("hist_len", hist_len, (B,)),
                           ("n_out", n_out, (B,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"spec_accept: {name} must have shape {list(shape)}")
    for name, t in (("history", history), ("out_tokens", out_tokens), ("out_src", out_src), ("emitted", emitted), ("draft_from", draft_from)):
        if t is not None and (t.dim() != 2 or t.shape[0] != B):
            raise ValueError(f"spec_accept: {name} must be [{B}, n]")
    if out_src is not None and out_src.shape[1] != out_tokens.shape[1]:
        raise ValueError("spec_accept: out_src has the shape of out_tokens")
    a = H.SpecArgs()
    a.ngram_max, a.B, a.K, a.Kin = int(ngram_max), B, K, Kin
    a.fed, a.picked, a.positions, a.prefill_len = (H.ptr(fed) if Kin == K else None), picked.data_ptr(), positions.data_ptr(), int(prefill_len)
    a.history, a.hist_ld, a.hist_len = history.data_ptr(), history.shape[1], hist_len.data_ptr()
    a.out_tokens, a.out_ld, a.n_out = out_tokens.data_ptr(), out_tokens.shape[1], n_out.data_ptr()
    a.finished = finished.data_ptr()
    a.max_new, a.eos_id, a.pad_id = int(max_new_tokens), (-1 if eos_token_id is None else int(eos_token_id)), int(pad_token_id)
    a.step = int(step)
    a.out_src = H.ptr(out_src)
    a.emitted, a.emitted_ld = H.ptr(emitted), (0 if emitted is None else emitted.shape[1])
    a.draft_from, a.draft_ld = H.ptr(draft_from), (0 if draft_from is None else draft_from.shape[1])
    a.next_tokens = next_tokens.data_ptr()
    H.check(H.load().kx_spec_accept(C.byref(a), _stream()), "kx_spec_accept")


def beam_step(logits, scores_in, *, num_beams, step, pool, done, scores_out, next_token, parent, src_row, scratch,
              length_penalty=1.0, early_stopping=False, eos_token_id=None, pad_token_id=1):
    """One beam-search step (kx_beam_step in include/kosmosx_hip.h) over fp32 `logits` [B * Win, V] (row stride >= V), Win = 1 at
    ``step`` 0 and ``num_beams`` (W) afterwards, with the input beams' fp32 ``scores_in`` [B * Win].

    Caller-owned state and outputs, all on the device: ``pool`` = (score fp32, end int32, parent int32, each [B, W]; count int32
    [B]), ``done`` uint8 [B] (count and done zeroed before step 0); ``scores_out`` fp32, ``next_token`` int64, ``parent`` int32,
    ``src_row`` int32, each [B * W]; ``scratch`` int64 with at least B * Win * 2W elements.  Returns None."""
    ps, pe, pp, pc = pool
    _need_cuda(logits, scores_in, ps, pe, pp, pc, done, scores_out, next_token, parent, src_row, scratch)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise TypeError("beam_step: logits must be fp32 [B * Win, V] with unit column stride")
    W = int(num_beams)
    rows, V = logits.shape
    Win = 1 if int(step) == 0 else W
    if W < 1 or rows % Win:
        raise ValueError(f"beam_step: {rows} logits rows are not a multiple of Win = {Win}")
    B = rows // Win
    for name, t, dt, n in (("scores_in", scores_in, torch.float32, B * Win), ("scores_out", scores_out, torch.float32, B * W),
                           ("next_token", next_token, torch.int64, B * W), ("parent", parent, torch.int32, B * W),
                           ("src_row", src_row, torch.int32, B * W), ("pool score", ps, torch.float32, B * W),
                           ("pool end", pe, torch.int32, B * W), ("pool parent", pp, torch.int32, B * W),
                           ("pool count", pc, torch.int32, B), ("done", done, torch.uint8, B)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != n:
            raise TypeError(f"beam_step: {name} must be a contiguous {dt} tensor of {n} elements")
    if scratch.dtype != torch.int64 or not scratch.is_contiguous() or scratch.numel() < B * Win * 2 * W:
        raise TypeError(f"beam_step: scratch must be a contiguous int64 tensor of at least {B * Win * 2 * W} elements")
    a = H.BeamArgs()
    a.early_stopping = int(bool(early_stopping))
    a.logits, a.ld, a.B, a.Win, a.W, a.V = logits.data_ptr(), (logits.stride(0) if rows > 1 else max(logits.stride(0), V)), B, Win, W, V
    a.step, a.length_penalty = int(step), float(length_penalty)
    a.eos_id, a.pad_id = (-1 if eos_token_id is None else int(eos_token_id)), int(pad_token_id)
    a.scores_in, a.scores_out = scores_in.data_ptr(), scores_out.data_ptr()
    a.next_token, a.parent, a.src_row = next_token.data_ptr(), parent.data_ptr(), src_row.data_ptr()
    a.pool_score, a.pool_end, a.pool_parent, a.pool_count = ps.data_ptr(), pe.data_ptr(), pp.data_ptr(), pc.data_ptr()
    a.done, a.scratch = done.data_ptr(), scratch.data_ptr()
    H.check(H.load().kx_beam_step(C.byref(a), _stream()), "kx_beam_step")


def beam_finalize(scores_live, done, pool, parent, token, n, *, num_return_sequences=1, length_penalty=1.0, eos_token_id=None,
                  pad_token_id=1, out_tokens=None, out_scores=None):
    """kx_beam_finalize: offer the live beams of the rows that are not done to the pool, then backtrack the R best hypotheses of
    every row through the ``parent`` int32 / ``token`` int64 [>= n, B * W] backpointers of ``n`` steps.
    Returns (out_tokens int64 [B, R, >= n] — columns 0:n written —, out_scores fp32 [B, R])."""
    ps, pe, pp, pc = pool
    _need_cuda(scores_live, done, ps, pe, pp, pc, parent, token, out_tokens, out_scores)
    B, W = ps.shape
    R, n = int(num_return_sequences), int(n)
    if (parent.dtype != torch.int32 or token.dtype != torch.int64 or parent.dim() != 2 or tuple(parent.shape) != tuple(token.shape)
            or parent.shape[0] < n or parent.shape[1] != B * W or not (parent.is_contiguous() and token.is_contiguous())):
        raise TypeError(f"beam_finalize: parent int32 / token int64 must be contiguous [>= {n}, {B * W}] tensors")
    for name, t, dt, m in (("scores_live", scores_live, torch.float32, B * W), ("done", done, torch.uint8, B),
                           ("pool score", ps, torch.float32, B * W), ("pool end", pe, torch.int32, B * W),
                           ("pool parent", pp, torch.int32, B * W), ("pool count", pc, torch.int32, B)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != m:
            raise TypeError(f"beam_finalize: {name} must be a contiguous {dt} tensor of {m} elements")
    if out_tokens is None:
        out_tokens = torch.empty((B, max(R, 1), n), dtype=torch.int64, device=ps.device)
    if out_scores is None:
        out_scores = torch.empty((B, max(R, 1)), dtype=torch.float32, device=ps.device)
    if (out_tokens.dtype != torch.int64 or not out_tokens.is_contiguous() or out_tokens.dim() != 3
            or tuple(out_tokens.shape[:2]) != (B, R) or out_scores.dtype != torch.float32 or not out_scores.is_contiguous()
            or tuple(out_scores.shape) != (B, R)):
        raise TypeError(f"beam_finalize: out_tokens int64 [{B}, {R}, >= n] and out_scores fp32 [{B}, {R}], contiguous")
    H.check(H.load().kx_beam_finalize(scores_live.data_ptr(), done.data_ptr(), ps.data_ptr(), pe.data_ptr(), pp.data_ptr(),
                                      pc.data_ptr(), parent.data_ptr(), token.data_ptr(), parent.shape[1], B, W, R, n,
                                      float(length_penalty), -1 if eos_token_id is None else int(eos_token_id), int(pad_token_id),
                                      out_tokens.data_ptr(), out_tokens.shape[2], out_scores.data_ptr(), _stream()),
            "kx_beam_finalize")
    return out_tokens, out_scores


def kv_cache_gather(src_k, src_v, dst_k, dst_v, t, src_row, error_word, layout="head_major"):
    """kx_kv_cache_gather: dst[l, r, h, :t] = src[l, src_row[r], h, :t] for the two caches ([L, B, heads, Tmax, 64], fp32 or bf16,
    contiguous), ``src_row`` int32 [B_dst] on the device.  An entry outside [0, B_src) copies nothing for that row and sets
    KX_RAGGED_ERR_GATHER in ``error_word`` (int32 [1], sticky).  src and dst must not overlap.
    ``layout`` "row_major": the tensors are shaped [L, B, Tmax, heads, 64] (dst[l, r, :t] = src[l, src_row[r], :t]), the layout
    the library copies under tuning key 9 = 1; the argument only names the shape that is checked, the caller sets the key."""
    _need_cuda(src_k, src_v, dst_k, dst_v, src_row, error_word)
    if layout not in ("head_major", "row_major"):
        raise ValueError("kv_cache_gather: layout is 'head_major' or 'row_major'")
    if layout == "row_major":
        L, Bs, Tmax, nh, hd = src_k.shape
    else:
        L, Bs, nh, Tmax, hd = src_k.shape
    Bd = dst_k.shape[1]
    if hd != 64 or tuple(src_v.shape) != tuple(src_k.shape) or tuple(dst_k.shape) != (L, Bd, *src_k.shape[2:]) or tuple(dst_v.shape) != tuple(dst_k.shape):
        raise ValueError("kv_cache_gather: caches are [L, B, heads, Tmax, 64], k and v alike, src and dst differing in B only")
    if len({src_k.dtype, src_v.dtype, dst_k.dtype, dst_v.dtype}) != 1 or src_k.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("kv_cache_gather: the four caches share one dtype, fp32 or bf16")
    if not all(c.is_contiguous() for c in (src_k, src_v, dst_k, dst_v)):
        raise ValueError("kv_cache_gather: the caches must be contiguous")
    if src_row.dtype != torch.int32 or tuple(src_row.shape) != (Bd,) or not src_row.is_contiguous():
        raise TypeError(f"kv_cache_gather: src_row must be a contiguous int32 [{Bd}] tensor")
    if error_word is None or error_word.dtype != torch.int32 or error_word.numel() != 1:
        raise TypeError("kv_cache_gather: error_word must be an int32 [1] tensor on the device (the kernel's sticky word)")
    H.check(H.load().kx_kv_cache_gather(src_k.data_ptr(), src_v.data_ptr(), dst_k.data_ptr(), dst_v.data_ptr(), L, Bs, Bd, nh,
                                        Tmax, int(t), src_k.element_size(), src_row.data_ptr(), error_word.data_ptr(), _stream()),
            "kx_kv_cache_gather")


# ---- contrastive search on the device (include/kosmosx_hip.h, "Contrastive search on the device") ----

def _contrast_tensor(fn, name, t, dtype, shape=None, optional=False):
    if t is None:
        if optional:
            return
        raise TypeError(f"{fn}: {name} is missing")
    if t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise TypeError(f"{fn}: {name} is a contiguous {dtype} tensor" + (f" of shape {list(shape)}" if shape is not None else ""))


def _contrast_k(fn, k):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 16:
        raise ValueError(f"{fn}: k = {k!r} is outside 1..16")
    return k


def contrast_candidates(logits, *, k, step_tokens, prob, chosen=None, k_prev=1, finished=None, cand_id=None, cand_prob=None, col=0):
    """kx_contrast_candidates: the k most likely ids of every sequence's current logits row and their probabilities.  ``logits``
    fp32 [rows, V] with unit column stride; sequence b reads row b * k_prev + chosen[b] (``chosen`` int32 [B]) or, without ``chosen``,
    row b.  Writes ``step_tokens`` int64 [B * k], ``prob`` fp32 [B * k] and, when given, column ``col`` of ``cand_id`` int64 /
    ``cand_prob`` fp32 [B, N, k]: the ids and expf(log-prob) of step_logprobs(top_n=k) on that row, bit for bit.  Rows with
    ``finished`` [B] uint8 set write nothing.  Returns None."""
    fn = "contrast_candidates"
    _need_cuda(logits, step_tokens, prob, chosen, finished, cand_id, cand_prob)
    k = _contrast_k(fn, k)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise TypeError(f"{fn}: logits is a non-empty fp32 [rows, V] tensor with unit column stride")
    rows, V = logits.shape
    if rows > 1 and logits.stride(0) < V:
        raise TypeError(f"{fn}: logits rows overlap (row stride {logits.stride(0)} < V = {V})")
    if k > V:
        raise ValueError(f"{fn}: k = {k} exceeds the vocabulary of {V}")
    if step_tokens is None or step_tokens.dim() != 1 or step_tokens.shape[0] % k:
        raise TypeError(f"{fn}: step_tokens is a contiguous int64 [B * k] tensor")
    B = step_tokens.shape[0] // k
    _contrast_tensor(fn, "step_tokens", step_tokens, torch.int64, (B * k,))
    _contrast_tensor(fn, "prob", prob, torch.float32, (B * k,))
    _contrast_tensor(fn, "chosen", chosen, torch.int32, (B,), optional=True)
    _contrast_tensor(fn, "finished", finished, torch.uint8, (B,), optional=True)
    if chosen is None:
        k_prev = 1
    if isinstance(k_prev, bool) or not isinstance(k_prev, int) or not 1 <= k_prev <= 16:
        raise ValueError(f"{fn}: k_prev = {k_prev!r} is outside 1..16")
    if rows < B * k_prev:
        raise ValueError(f"{fn}: logits has {rows} rows, fewer than B * k_prev = {B * k_prev}")
    N = 1
    if (cand_id is None) != (cand_prob is None):
        raise TypeError(f"{fn}: cand_id and cand_prob are given together")
    if cand_id is not None:
        if cand_id.dim() != 3:
            raise TypeError(f"{fn}: cand_id is a contiguous int64 [{B}, N, {k}] tensor")
        N = cand_id.shape[1]
        _contrast_tensor(fn, "cand_id", cand_id, torch.int64, (B, N, k))
        _contrast_tensor(fn, "cand_prob", cand_prob, torch.float32, (B, N, k))
        if isinstance(col, bool) or not isinstance(col, int) or not 0 <= col < N:
            raise ValueError(f"{fn}: col = {col!r} is outside the {N} columns of cand_id")
    H.check(H.load().kx_contrast_candidates(logits.data_ptr(), logits.stride(0) if rows > 1 else max(logits.stride(0), V), rows, B, V, k,
                                            H.ptr(chosen), k_prev, H.ptr(finished), step_tokens.data_ptr(), prob.data_ptr(),
                                            H.ptr(cand_id), H.ptr(cand_prob), N, int(col) if cand_id is not None else 0, _stream()),
            "kx_contrast_candidates")


def contrast_hidden(weights, x, out, *, workspace=None, prec=None, lengths=None, residual_out=None):
    """kx_contrast_hidden: the fp32 unit vectors u = h / ||h||, h = decoder.layer_norm of the rows of the final residual stream.
    ``weights``: the decoder's bound kx_decoder_weights.  ``x`` fp32 [M, 1, D] or [M, D] with ``workspace`` (the tensor the step ran
    in) and ``prec`` (the step's precision id): the rows of the decode step that has just run, ``out`` fp32 [M, D].  Without
    ``workspace``: ``x`` fp32 [B, T, D] rows as they are (a prefill's), written to out[b, t] of ``out`` fp32 [B, cap >= T, D];
    ``lengths`` int32 [B]: rows t >= lengths[b] are not written.  ``residual_out`` fp32, as many elements as ``x``: the residual rows
    the kernel normalised (x, or the pair x + xb of a step that ran its two-workgroup form).  Returns ``out``."""
    fn = "contrast_hidden"
    _need_cuda(x, out, workspace, lengths, residual_out)
    if residual_out is not None and (residual_out.dtype != torch.float32 or not residual_out.is_contiguous() or residual_out.numel() != x.numel()):
        raise TypeError(f"{fn}: residual_out is a contiguous fp32 tensor of x's size")
    D = int(weights.dim)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.shape[-1] != D or out.dtype != torch.float32 or not out.is_contiguous() \
            or out.shape[-1] != D:
        raise TypeError(f"{fn}: x and out are contiguous fp32 tensors whose last dimension is the model's {D}")
    if workspace is not None:
        M = x.numel() // D
        if prec is None or lengths is not None or out.numel() != M * D:
            raise TypeError(f"{fn}: a step's rows take prec, no lengths and out [{M}, {D}]")
        B, T, step, ld, ws = M, 1, 1, D, workspace.data_ptr()
    else:
        if x.dim() != 3 or out.dim() != 3 or out.shape[0] != x.shape[0] or out.shape[1] < x.shape[1]:
            raise TypeError(f"{fn}: x is [B, T, {D}] and out [B, cap >= T, {D}]")
        B, T, step, ld, ws, prec = x.shape[0], x.shape[1], 0, out.shape[1] * D, 0, 0
        _contrast_tensor(fn, "lengths", lengths, torch.int32, (B,), optional=True)
    H.check(H.load().kx_contrast_hidden(C.byref(weights), x.data_ptr(), ws, B, T, int(prec), step, H.ptr(lengths), out.data_ptr(), ld,
                                        H.ptr(residual_out), _stream()), "kx_contrast_hidden")
    return out


def contrast_scratch(B, k, cap, device):
    """The fp32 scratch contrast_select takes for B sequences, k candidates and ``cap`` history rows (partial maxima)."""
    return torch.empty(max(H.load().kx_contrast_scratch_bytes(B, k, cap) // 4, 1), dtype=torch.float32, device=device)


def contrast_select(u, prob, history, *, hist_rows, hist_len, alpha, step_tokens, finished, next_token, chosen, scratch, error_word,
                    p_stride=1, eos_token_id=None, pad_token_id=1, out_tokens=None, cand_penalty=None, chosen_trace=None, col=0):
    """kx_contrast_select: the degeneration penalty and the choice.  ``u`` fp32 [B * k, D] unit vectors of the candidates, ``prob``
    fp32 [B * k], ``history`` fp32 [B, cap, D]; P_b = hist_rows[b * p_stride] (int32).  penalty_j = max over i < P_b of
    dot(u[b * k + j], history[b, i]); score_j = fp32(1 - alpha) * p_j - alpha * penalty_j; the largest score wins, the lowest j among
    equal ones.  Writes next_token [B] int64, chosen [B] int32, history[b, P_b], hist_len[b] = P_b + 1, finished[b] on the EOS and
    column ``col`` of out_tokens int64 [B, N], chosen_trace int32 [B, N], cand_penalty fp32 [B, N, k] (each optional).  A finished row
    writes its pad token only.  Returns None."""
    import ctypes
    fn = "contrast_select"
    _need_cuda(u, prob, history, hist_rows, hist_len, step_tokens, finished, next_token, chosen, scratch, error_word, out_tokens,
               cand_penalty, chosen_trace)
    if history is None or history.dim() != 3:
        raise TypeError(f"{fn}: history is a contiguous fp32 [B, cap, D] tensor")
    B, cap, D = history.shape
    if u is None or u.dim() != 2 or u.shape[1] != D or u.shape[0] % B or not 1 <= u.shape[0] // B <= 16:
        raise TypeError(f"{fn}: u is a contiguous fp32 [B * k, {D}] tensor, k in 1..16")
    k = u.shape[0] // B
    _contrast_tensor(fn, "history", history, torch.float32)
    _contrast_tensor(fn, "u", u, torch.float32)
    _contrast_tensor(fn, "prob", prob, torch.float32, (B * k,))
    _contrast_tensor(fn, "step_tokens", step_tokens, torch.int64, (B * k,))
    _contrast_tensor(fn, "hist_len", hist_len, torch.int32, (B,))
    _contrast_tensor(fn, "finished", finished, torch.uint8, (B,))
    _contrast_tensor(fn, "next_token", next_token, torch.int64, (B,))
    _contrast_tensor(fn, "chosen", chosen, torch.int32, (B,))
    _contrast_tensor(fn, "scratch", scratch, torch.float32)
    if isinstance(p_stride, bool) or not isinstance(p_stride, int) or p_stride < 1:
        raise ValueError(f"{fn}: p_stride = {p_stride!r} must be a positive integer")
    _contrast_tensor(fn, "hist_rows", hist_rows, torch.int32)
    if hist_rows.numel() < (B - 1) * p_stride + 1:
        raise TypeError(f"{fn}: hist_rows holds fewer than (B - 1) * p_stride + 1 = {(B - 1) * p_stride + 1} words")
    if error_word is None or error_word.dtype != torch.int32 or error_word.numel() != 1:
        raise TypeError(f"{fn}: error_word must be an int32 [1] tensor on the device (the kernels' sticky word)")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= alpha <= 1.0:
        raise ValueError(f"{fn}: alpha = {alpha!r} must be a number in [0, 1]")
    a32 = ctypes.c_float(alpha).value
    oma = ctypes.c_float(1.0 - a32).value                 # 1 - alpha, computed on the host in fp32
    N = 1
    for name, t, dt, tail in (("out_tokens", out_tokens, torch.int64, ()), ("chosen_trace", chosen_trace, torch.int32, ()),
                              ("cand_penalty", cand_penalty, torch.float32, (k,))):
        if t is not None:
            if t.dim() != 2 + len(tail):
                raise TypeError(f"{fn}: {name} is a contiguous {dt} [{B}, N{', k' if tail else ''}] tensor")
            N = t.shape[1]
    for name, t, dt, tail in (("out_tokens", out_tokens, torch.int64, ()), ("chosen_trace", chosen_trace, torch.int32, ()),
                              ("cand_penalty", cand_penalty, torch.float32, (k,))):
        _contrast_tensor(fn, name, t, dt, (B, N, *tail), optional=True)
    if isinstance(col, bool) or not isinstance(col, int) or not 0 <= col < N:
        raise ValueError(f"{fn}: col = {col!r} is outside the {N} output columns")
    H.check(H.load().kx_contrast_select(u.data_ptr(), prob.data_ptr(), history.data_ptr(), B, k, D, cap, hist_rows.data_ptr(), p_stride,
                                        hist_len.data_ptr(), a32, oma, step_tokens.data_ptr(), finished.data_ptr(),
                                        -1 if eos_token_id is None else int(eos_token_id), int(pad_token_id), next_token.data_ptr(),
                                        chosen.data_ptr(), H.ptr(out_tokens), N, col, H.ptr(cand_penalty), H.ptr(chosen_trace),
                                        scratch.data_ptr(), scratch.numel() * 4, error_word.data_ptr(), _stream()), "kx_contrast_select")


def kv_cache_commit(ktail, vtail, kcache, vcache, chosen, positions, error_word, *, finished=None, layout="head_major"):
    """kx_kv_cache_commit: cache[l, b, h, P_b] = tail[l, b * k + chosen[b], h, 0] for the k and v caches ([L, B, heads, Tmax, 64]) and
    tails ([L, B * k, heads, Ttail, 64]; fp32 or bf16, contiguous), P_b = positions[b * k]; then positions[b * k : b * k + k] = P_b + 1.
    ``chosen`` int32 [B], ``positions`` int32 [B * k]; rows with ``finished`` [B] uint8 set are skipped.  A chosen index outside
    [0, k) or a P_b outside [0, Tmax) writes nothing and sets KX_RAGGED_ERR_COMMIT in ``error_word`` (int32 [1], sticky).
    ``layout`` "row_major": the tensors are shaped [L, B, Tmax, heads, 64] / [L, B * k, Ttail, heads, 64], what the library copies
    under tuning key 9 = 1; the argument only names the shape that is checked, the caller sets the key."""
    fn = "kv_cache_commit"
    _need_cuda(ktail, vtail, kcache, vcache, chosen, positions, error_word, finished)
    if layout not in ("head_major", "row_major"):
        raise ValueError(f"{fn}: layout is 'head_major' or 'row_major'")
    if kcache.dim() != 5 or ktail.dim() != 5:
        raise ValueError(f"{fn}: caches and tails are five-dimensional")
    if layout == "row_major":
        (L, B, Tmax, nh, hd), (Lt, M, Ttail, nht, hdt) = kcache.shape, ktail.shape
    else:
        (L, B, nh, Tmax, hd), (Lt, M, nht, Ttail, hdt) = kcache.shape, ktail.shape
    if hd != 64 or hdt != 64 or Lt != L or nht != nh or M % B or not 1 <= M // B <= 16 or tuple(vcache.shape) != tuple(kcache.shape) \
            or tuple(vtail.shape) != tuple(ktail.shape):
        raise ValueError(f"{fn}: caches are [L, B, heads, Tmax, 64] and tails [L, B * k, heads, Ttail, 64], k and v alike, k in 1..16")
    k = M // B
    if len({ktail.dtype, vtail.dtype, kcache.dtype, vcache.dtype}) != 1 or kcache.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{fn}: the four tensors share one dtype, fp32 or bf16")
    if not all(c.is_contiguous() for c in (ktail, vtail, kcache, vcache)):
        raise ValueError(f"{fn}: the caches and tails must be contiguous")
    _contrast_tensor(fn, "chosen", chosen, torch.int32, (B,))
    _contrast_tensor(fn, "positions", positions, torch.int32, (M,))
    _contrast_tensor(fn, "finished", finished, torch.uint8, (B,), optional=True)
    if error_word is None or error_word.dtype != torch.int32 or error_word.numel() != 1:
        raise TypeError(f"{fn}: error_word must be an int32 [1] tensor on the device (the kernel's sticky word)")
    H.check(H.load().kx_kv_cache_commit(ktail.data_ptr(), vtail.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), L, B, k, nh, Tmax,
                                        Ttail, kcache.element_size(), chosen.data_ptr(), positions.data_ptr(), H.ptr(finished),
                                        error_word.data_ptr(), _stream()), "kx_kv_cache_commit")
