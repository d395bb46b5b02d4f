"""Autoregressive generation on top of the KV-cache decode step (Kosmos.generate / KosmosLanguage.generate).

The loop stays on the device: kx_sample_logits reads the logits row a step has just written and leaves the next token in
device memory, kx_embed_step gathers its embedding for the next step.  The host only enqueues; its one read is the stop
poll, every ``eos_poll`` steps and only when an ``eos_token_id`` is given.

Not offered: ragged prompts / padding masks, beam search, compaction of finished rows, replaying the step
as a captured graph.
"""
from __future__ import annotations

import torch

from . import ops


def generate_loop(decoder, prec: str, state: dict, logits: torch.Tensor, prompt_tokens: torch.Tensor, max_new_tokens: int,
                  *, pos_shift: int = 0, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0,
                  seed=0, eos_token_id=None, pad_token_id=1, sequence_ids=None, eos_poll=8, output_logits=False):
    """``logits`` [B, T, V]: the prefill's output, ``state`` the incremental state it filled (state["len"] == T).
    ``prompt_tokens`` [B, Tt] int64: what the repetition penalty sees before the first new token.  ``pos_shift`` > 0: the
    prompt holds that many spliced rows that are not tokens and text rows carry two position rows (the multimodal prompt
    under u1_inplace_alias): a token at sequence position t is embedded with pos[2 + t - pos_shift] + pos[2 + t]."""
    B, T, V = logits.shape
    dev = logits.device
    out = torch.full((B, max_new_tokens), int(pad_token_id), dtype=torch.int64, device=dev)
    nxt = torch.empty(B, dtype=torch.int64, device=dev)
    finished = torch.zeros(B, dtype=torch.uint8, device=dev)
    history = None
    Tt = prompt_tokens.shape[1]
    if float(repetition_penalty) != 1.0:
        history = torch.empty((B, Tt + max_new_tokens), dtype=torch.int64, device=dev)
        history[:, :Tt] = prompt_tokens
    if sequence_ids is not None:
        sequence_ids = sequence_ids.to(device=dev, dtype=torch.int64).contiguous()
    kept = []
    row = logits[:, -1]                                                   # [B, V] view, row stride T * V
    n = 0
    for g in range(max_new_tokens):
        ops.sample_logits(row, temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty,
                          do_sample=do_sample, seed=seed, position=T + g, sequence_ids=sequence_ids, history=history,
                          hist_len=Tt + g, finished=finished, eos_token_id=eos_token_id, pad_token_id=pad_token_id,
                          out=nxt, out_tokens=out, out_col=g)
        if output_logits:
            kept.append(row.clone())
        n = g + 1
        if n == max_new_tokens:
            break
        if eos_token_id is not None and eos_poll > 0 and n % eos_poll == 0 and bool(finished.all()):
            break                                                         # the loop's only device-to-host read
        t = T + g
        pos = (t - pos_shift, t) if pos_shift else (t, -1)
        row = decoder._forward_incremental(None, state, None, prec, next_token=nxt, next_pos=pos)[:, 0]
    out = out[:, :n]
    if output_logits:
        return out, torch.stack(kept, dim=1)
    return out


def check_budget(decoder, T: int, max_new_tokens: int):
    """IndexError before any launch when prompt + new tokens overrun the position table / cache."""
    if not isinstance(max_new_tokens, int) or max_new_tokens < 1:
        raise ValueError(f"max_new_tokens must be a positive integer, got {max_new_tokens!r}")
    rows = decoder.embed_positions.weight.shape[0] - 2
    # (conservative by one token: the last generated token is never embedded, so it would not need a row of its own)
    if T + max_new_tokens > rows:
        raise IndexError(f"index out of range in self: {T} prompt positions + {max_new_tokens} new tokens exceed the "
                         f"{rows}-row position table / cache")
