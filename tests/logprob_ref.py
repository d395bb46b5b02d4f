"""Float64 CPU reference of kx_step_logprobs (include/kosmosx_hip.h, "Per-token log-probs of a generation step").

  log_softmax_ref: x - logsumexp(x) per row in float64 (-inf entries stay -inf).
  top_ref: a row's top n (ids, log-probs): candidates ordered by np.lexsort((ids, -values)) on the fp32 VALUES — value descending,
           the lowest id first among equal values, -inf last — and, with V < n, padded with (-1, -inf).
  step_ref: both for a [B, V] block and the tokens drawn from it: (token_logprob [B], top_logprob [B, n], top_id [B, n]); a token
           outside [0, V) gives 0.0.
"""
import numpy as np
import torch


def log_softmax_ref(x: torch.Tensor) -> torch.Tensor:
    return torch.log_softmax(x.detach().cpu().double(), dim=-1)


def top_ref(row: torch.Tensor, n: int):
    """``row`` fp32 [V] -> (ids int64 [n], log-probs float64 [n])."""
    v = row.detach().cpu().float().numpy()
    V = v.shape[0]
    order = np.lexsort((np.arange(V), -v))[:n]
    lsm = log_softmax_ref(row.detach().cpu().float()).numpy()
    ids = np.full(n, -1, dtype=np.int64)
    lps = np.full(n, -np.inf, dtype=np.float64)
    ids[:len(order)] = order
    lps[:len(order)] = lsm[order]
    return torch.from_numpy(ids), torch.from_numpy(lps)


def step_ref(x: torch.Tensor, token: torch.Tensor, n: int):
    """``x`` fp32 [B, V], ``token`` int64 [B] -> (token_logprob float64 [B], top_logprob float64 [B, n], top_id int64 [B, n])."""
    x, token = x.detach().cpu().float(), token.detach().cpu()
    B, V = x.shape
    lsm = log_softmax_ref(x)
    lp = torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        t = int(token[b])
        if 0 <= t < V:
            lp[b] = lsm[b, t]
    tops = [top_ref(x[b], n) for b in range(B)]
    return lp, torch.stack([t[1] for t in tops]).view(B, n), torch.stack([t[0] for t in tops]).view(B, n)
