"""Autoregressive generation on top of the KV-cache decode step (Kosmos.generate / KosmosLanguage.generate).

The loop stays on the device: kx_sample_logits reads the logits row a step has just written and leaves the next token in
device memory, kx_embed_step gathers its embedding for the next step.  The host only enqueues; its one read is the stop
poll, every ``eos_poll`` steps and only when an ``eos_token_id`` is given.

Options: a public generate() takes its keyword arguments by name (_keywords) and run_generate validates every one of them once, in
one fixed order, each check_* function being handed the keywords its own signature names (_own).  What the plain loop was asked for
then travels as one LoopOptions — validated, resolved, frozen — to generate_loop and to everything that runs it: parallel_loop, the
guided call, a session's turns.  loop_options is the one internal place that names the plain loop's keywords and their defaults, and
where each of them is described; Session.generate and the tests that drive the loops directly call it.  The loops check nothing again.

Ragged batches (``prompt_lengths``): every row has its own position, an int32 word in device memory that the sampler
advances (kx_sample_logits_ragged) and the decode step reads (kx_decoder_decode_step_ragged) — a step's launch arguments are
then the same for every token.  Each row generates what it would generate alone.

Beam search (``num_beams`` > 1, beam_loop): the prefill runs once per batch row; kx_beam_step ranks the beams x vocab candidates
of every batch row, keeps the pool of finished hypotheses and the row's done byte and leaves tokens, scores and backpointers in
device memory; kx_kv_cache_gather re-parents the cache rows into the other of two B * num_beams-row caches; the decode step is the
uniform one at B * num_beams rows.  kx_beam_finalize backtracks the best hypotheses after the last step.

Constraints (``no_repeat_ngram_size``, ``bad_words_ids``, ``min_new_tokens``, ``stop_sequences``): one kx_constrain_logits launch
in front of the sampler (or the beam step) sets the banned ids' logits to -inf in place and marks rows that met a stop sequence
finished; the sampler and the beam step already never pick -inf.  It reads the history buffer the sampler appends to, so the token
still never leaves the device.  With every constraint at its default the launch is not issued.

Prompt-lookup speculative decoding (``prompt_lookup_num_tokens`` = D > 0, lookup_loop): every step runs K = D + 1 rows per sequence
through one pass over the weights (kx_decoder_decode_step_block: the last confirmed token and D drafts at consecutive positions of
the sequence's cache), kx_sample_logits picks greedily on all of them and kx_spec_accept keeps the picks the drafts led up to
correctly, appends them, moves the positions and copies the next drafts from where the row's last n-gram occurred before.  Exact
for greedy decoding; the host reads only the stop poll.

Scoring (``score()``, score_loop): the log-likelihood of C candidate continuations over B prefilled prompts — column 0 from the
prefill's rows, every later column from ONE step of C * (L - 1) rows in which the candidates read their prompt's cache rows and
nobody appends (kx_decoder_score_step), the log-probs taken row by row without a softmax (kx_token_logprob).

Sessions (``return_session``, Session): the plain loop's state kept after the call.  A later turn's ids — behind the row's pending
token, the last one sampled and never fed — are appended at every row's own device-resident position in one ragged extend pass
(kx_decoder_extend_ragged via Decoder._extend_ragged), then the same loop runs on; the host reads the error word and the rows'
valid token counts once per turn.

Parallel sampling (``num_return_sequences`` = n > 1 with ``do_sample`` and no beams, parallel_loop): the prefill runs once at B rows;
the B * n samples then run the ragged loop, every row reading its prompt's cache rows — shared and read only — and appending its own
tokens' keys to a private tail cache of ``max_new_tokens`` rows (kx_decoder_decode_step_prefix).  Row b * n + i is sample i of prompt b,
drawn from the Philox stream ``sequence_ids[b * n + i]``: the tokens of the same call on the prompt repeated n times.

Log-probs (``output_logprobs``, ``top_logprobs`` = k; generate_loop and everything that runs it): one kx_step_logprobs launch after
each sampler launch writes the log-prob of the token just drawn under the model's own logits — kx_token_logprob's arithmetic — and
the row's k most likely (log-prob, id) pairs into column g of buffers allocated before the loop; rows that entered the sampler launch
finished keep exact zeros.  No logits row is kept and the host reads nothing more.

Token automata (``token_automaton``, ``automaton_start``; every loop but lookup_loop): every row carries a state of a
kosmosx.automaton.TokenAutomaton in device memory; one kx_automaton_step launch in front of the sampler (or the beam step), after
the constraint launch, advances it on the token just emitted — under beams through the beam step's src_row, so the states follow the
backpointers — and sets the logits of the ids the new state bans to -inf.  Two state buffers alternate.  A state with no way out bans
the whole row: the sampler pads and finishes it, so the stop poll also runs whenever an automaton is given.  Without one: no
buffer, no launch, no further host read.

Logit shaping (``logit_bias``, ``presence_penalty``, ``frequency_penalty``, ``min_p``; generate_loop and everything that runs it): the
request fields a completion API passes through.  One kx_shape_logits launch in front of the sampler, after the constraint and
automaton launches, counts the token just emitted in an int32 [B, V] table that starts at zero with every call (and every turn of a
session), adds the per-id biases (-inf = a ban) and subtracts frequency * count + presence where the count is positive — single fp32
operations an outside reference can restate bit for bit.  ``min_p`` is one more threshold inside the sampler, after top-p
(kx_sample_logits_min_p).  With the four at their defaults: no buffer, no launch, the sampler's old entry points.

Truncation sampling (``typical_p``, ``epsilon_cutoff``, ``eta_cutoff``; generate_loop and everything that runs it): the three
`transformers` truncation samplers as further stages inside the sampler launch, behind min-p and in that order, each over what the
stage before it kept (kx_sample_logits_truncate).  Only when sampling; no buffer, no further launch, and with the three at their
defaults the entry points above.

Classifier-free guidance (``guidance_scale`` = s with ``negative_prompt_ids`` / ``negative_prompt_lengths`` / ``negative_images``;
run_generate and generate_loop): every sequence runs as two rows of one 2B-row ragged batch — rows 0..B-1 read the prompt (the
conditional rows), rows B..2B-1 a negative prompt or a negative image (the unconditional rows) — prefilled through _prefill unchanged
and stepped by the ragged decode step at 2B rows.  One kx_guidance_logits launch per token, in front of the constraint, automaton and
shaping launches, writes lu + s * (lc - lu) over the two raw rows' log-softmaxes onto the conditional row — kx_token_logprob's
arithmetic, then three single fp32 operations an outside reference restates bit for bit — and moves the unconditional positions on;
the sampler and every row editor see the first B rows; one device-to-device copy feeds the sampled token to both rows.  With the scale
at 1.0: no buffer, no launch, no further host read, nothing doubled.

Per-row options (``row_options``; generate_loop and everything that runs it): B dicts of overrides, resolved against the call's own
keywords by check_row_options into one table (LoopOptions.rows).  The table is packed by the library (kx_sample_rows_pack), uploaded
once, and read by one more instantiation of the sampler's kernel (kx_sample_logits_rows): its workgroup takes greedy-or-not, the
repetition penalty, temperature, top-k, top-p, min-p, the three cut-offs and the Philox seed from its row's record, so row b of a
mixed batch gets the bits of a call of its own.  Presence and frequency penalties travel as two fp32 [B] arrays
(kx_shape_logits_rows); a row's ``max_new_tokens`` is a budget the sampler launch itself enforces through ``finished``.  Without the
keyword, or with B empty dicts: no buffer, no upload, the entry points above.

Contrastive search (``penalty_alpha`` = a with ``top_k`` = k candidates, ``output_contrast``; contrast_loop): every step takes the k most
likely next tokens of each sequence (kx_contrast_candidates: kx_step_logprobs' selection on the row the previous choice addresses), steps
them as B * k rows over the sequences' own caches — the prefix step, prefix = the sequence so far, tail = one row — takes the unit
hidden rows (kx_contrast_hidden), chooses per sequence the candidate with the largest (1 - a) * p - a * max similarity to a history of
unit vectors that starts with the prefill's rows (kx_contrast_select) and commits its K/V row (kx_kv_cache_commit).  Five launches
beside the step; the host reads only the stop poll.  A mode of its own: with None nothing of it exists.

Not offered: contrastive search with any sampler, processor, constraint, automaton, guidance, beams, sessions, speculation or
chunked prefill, ``top_k`` above 16; per-row ``eos_token_id``, constraints and stop sequences, row options with beams or prompt lookup; guidance with beams, prompt lookup, parallel sampling or sessions, an unconditional row without the spliced
image, log-probs of the guided distribution; the shaping keywords with beams or prompt lookup, penalties over the prompt, counts that survive a session
turn; the truncation samplers with beams or prompt lookup, ``min_tokens_to_keep`` above 1, log-probs of the truncated distribution; token automata with prompt lookup, per-row tables other than through TokenAutomaton.union, an automaton
that reads the prompt, stop strings and regular expressions (the tokenizer); log-probs with beams or prompt lookup, of the processed distribution, or top-k out of ``score()``; beams that share their prompt's cache rows, forking a session, parallel sampling with prompt lookup or
sessions, sessions under beams or prompt lookup, compaction of finished rows, replaying the step as a captured graph, padding masks in
``Decoder.forward`` (``self_attn_padding_mask``); speculation with sampling, beams, constraints or ragged prompts, a draft model; with beams: ragged prompts, penalties, sampling and the constraints that read a per-beam history
(n-grams, multi-token bad words, stop sequences).
"""
from __future__ import annotations

import dataclasses
import functools
import inspect
import operator

import torch

from . import _hip as H
from . import ops


def _keywords(scope: dict, *positional) -> dict:
    """A function's keyword arguments by name: ``scope`` is its locals(), taken as the first statement of its body, ``positional``
    the parameters that are not among them.  The signature stays the one place that spells them."""
    return {k: v for k, v in scope.items() if k not in positional}


@functools.lru_cache(maxsize=None)
def _keyword_names(fn) -> tuple:
    return tuple(n for n, p in inspect.signature(fn).parameters.items() if p.kind is p.KEYWORD_ONLY)


def _own(fn, kw: dict) -> dict:
    """The entries of ``kw`` that ``fn`` declares as keyword-only arguments: a check or a loop is handed what its signature names."""
    return {n: kw[n] for n in _keyword_names(fn) if n in kw}


@dataclasses.dataclass(frozen=True)
class LoopOptions:
    """What generate_loop was asked for, validated and resolved: loop_options builds it, or run_generate from its own checks."""
    do_sample: bool
    temperature: float
    top_k: int
    top_p: float
    repetition_penalty: float
    seed: int
    sequence_ids: object
    eos_token_id: object
    pad_token_id: int
    eos_poll: int
    output_logits: bool
    output_logprobs: bool
    top_logprobs: int
    constraints: object                 # check_constraint_args' dict, or None: no kx_constrain_logits launch
    automaton: object                   # (the TokenAutomaton, check_automaton_args' host list of start states), or None
    shape: object                       # check_shape_args' dict, or None
    sampler: dict                       # what the sampler launch takes beyond its old arguments: min_p, check_truncation_args' keywords
    guidance: object                    # check_guidance_args' scale, or None
    contrast: object = None             # check_contrast_args' dict (alpha, k, trace), or None: contrast_loop runs the call when set
    rows: object = None                 # check_row_options' table: B dicts holding every ROW_KEYS entry resolved, or None

    @classmethod
    def resolved(cls, kw: dict, cons, starts, shape, truncation: dict, guide, rows=None, contrast=None):
        """From the keyword arguments by name and what the checks returned for them."""
        min_p = {} if shape is None or shape["min_p"] == 0.0 else dict(min_p=shape["min_p"])
        return cls(**{f.name: kw[f.name] for f in dataclasses.fields(cls) if f.name in kw}, constraints=cons, shape=shape,
                   automaton=None if starts is None else (kw["token_automaton"], starts), sampler={**min_p, **truncation},
                   guidance=None if guide is None else guide["scale"], rows=rows, contrast=contrast)


def loop_options(vocab: int, batch: int, *, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seed=0,
                 eos_token_id=None, pad_token_id=1, sequence_ids=None, eos_poll=8, output_logits=False, no_repeat_ngram_size=0,
                 bad_words_ids=None, min_new_tokens=0, stop_sequences=None, output_logprobs=False, top_logprobs=0,
                 token_automaton=None, automaton_start=None, logit_bias=None, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0,
                 guidance_scale=1.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, row_options=None, max_new_tokens=None,
                 penalty_alpha=None, output_contrast=False) -> LoopOptions:
    """The plain loop's keyword arguments -> the LoopOptions generate_loop takes, or the ValueError of the first check that refuses
    one: check_constraint_args, check_logprob_args, check_automaton_args, check_shape_args, check_truncation_args,
    check_row_options, in this order (then the scale through check_guidance_args); host only.  ``vocab``: the model's; ``batch``: the rows B the per-row values are
    given for.  What generate_loop does with each of them:
    Constraints (check_constraint_args): kx_constrain_logits runs on the row immediately before each sampler launch.  Its
    history is ``prompt_tokens`` followed by the generated tokens — the TEXT ids only: spliced image rows contribute no ids, so
    an n-gram, a bad word or a stop sequence may span the splice point.  ``text_lengths`` (ragged batches; default ``lengths``):
    row b's number of prompt TOKENS, where ``lengths`` counts the spliced rows too.  ``output_logits`` keeps returning the
    model's own logits, taken before the bans.
    ``output_logprobs`` / ``top_logprobs`` = k (check_logprob_args): one kx_step_logprobs launch after each sampler launch writes
    column g of token_logprobs [B, max_new_tokens] — the log-prob of the token just drawn under the model's own logits, the rows
    ``output_logits`` returns — and with k > 0 of top_logprobs / top_ids [B, max_new_tokens, k].  On a step with a constraint launch
    the raw row is a clone taken before it (the one ``output_logits`` keeps, when on).  A row that enters the sampler launch finished
    emits a pad: the ``finished`` bytes of that moment (what ``pad_launches`` counts) are snapshotted into a uint8 buffer and passed
    as the launch's ``skip``, its slots stay 0.0 / -1; when nothing can finish a row no snapshot is taken.
    ``token_automaton`` / ``automaton_start`` (check_automaton_args): two [B] int32 state buffers, the first holding the start states,
    are allocated before the loop and alternate; one kx_automaton_step launch per token on the row the sampler is about to read — after
    the step's constraint launch, so a row a stop sequence just finished is left alone — advances the states on ``nxt`` (step 0: no
    advance) and bans what the new state does not allow.  The bans add up with the constraints'; the raw row ``output_logits`` and
    ``output_logprobs`` use is taken before both.  A state with no way out bans the whole row: the sampler emits a pad and finishes
    the row (its rule 6), so rows end without an EOS and the stop poll runs whenever an automaton is given.  That pad is no token of
    the row: a row that the sampler launch finished on a token other than the EOS is counted in ``pad_launches`` and added to the
    launch's ``skip`` of ``output_logprobs`` (three small torch launches per step, only with an automaton and one of the two).
    Without an automaton: no buffer, no launch, no further host read.
    ``logit_bias`` / ``presence_penalty`` / ``frequency_penalty`` / ``min_p`` (check_shape_args; the biases are given for the B rows of
    this call): the bias table is uploaded and the int32 [B, V] counts are zeroed once before the loop (the counts only with a
    penalty); one kx_shape_logits launch per token on the row the sampler is about to read — after the constraint and automaton
    launches, before ``pad_launches`` is taken — counts ``nxt`` (step 0: nothing to count; finished rows are left alone, so pads do
    not count), adds the biases and applies the penalties over what THIS call emitted for the row: the prompt does not count, and a
    session's turn starts from zero.  ``min_p`` goes to the sampler launch (kx_sample_logits_min_p), after top-p.  The raw row
    ``output_logits`` and ``output_logprobs`` use is taken before the launch.  With the four at their defaults: no buffer, no
    launch, the sampler's old entry points.
    ``typical_p`` / ``epsilon_cutoff`` / ``eta_cutoff`` (check_truncation_args): the ones switched on go to the sampler launch
    (kx_sample_logits_truncate, ``min_p`` with them), behind min-p in that order.  No buffer and no further launch; with the three at
    their defaults the entry points are the ones named above.
    ``guidance_scale`` = s other than 1.0 (check_guidance_args): ``logits``, ``prompt_tokens``, ``lengths`` and ``text_lengths`` are the
    2B rows run_generate prefilled — rows 0..B-1 conditional, rows B..2B-1 unconditional, always a ragged batch; the negatives are
    already those rows, so the loop takes the scale alone.  The step runs at 2B rows
    (``positions`` int32 [2B], ``nxt`` int64 [2B], _ragged_scratch at 2B); the sampler and every row editor see B rows — the first
    B of ``positions`` / ``nxt`` and the conditional logits rows, with ``finished``, the histories (the conditional prompts' text ids,
    then the output), the counts, the automaton states and ``out`` at B rows.  Per token one kx_guidance_logits launch comes first:
    it reads the two raw rows, writes the guided row over the conditional one and advances the unconditional positions with the
    sampler's own ``advance``; after the sampler one device-to-device copy nxt[B:] = nxt[:B] feeds the token to both rows.  Row b
    draws at the conditional row's Philox position with ``sequence_ids[b]``: the stream of the unguided ragged call.  No host read is
    added: the error word covers all 2B rows and is read where it already is.  ``output_logits`` keeps the conditional rows' raw
    logits and, returned directly after them, the unconditional rows', both taken before the launch; ``output_logprobs`` reads the
    conditional rows' raw logits.  ``pad_launches`` (sessions) is refused.  With the scale at 1.0 nothing of this happens.
    ``row_options`` (check_row_options; B dicts, one per row of this call, each naming any of ROW_KEYS; ``max_new_tokens``: the call's
    own, the budgets' upper bound — None: not checked here): the resolved table travels as ``LoopOptions.rows``.  Before the first
    step the loop packs and uploads it once (ops.SampleRowTable), allocates ``history`` when any row has a repetition penalty and
    the counts when any row has a presence or frequency penalty, and uploads those two penalties as fp32 [B] arrays.  Per token the
    launch list is the one above, the sampler entry point being kx_sample_logits_rows and — only when the shaping launch runs and a
    row has a penalty — the shaping one kx_shape_logits_rows: row b gets what a call of its own with its resolved scalars gets, bit
    for bit, at the Philox address (row b's seed; position, ``sequence_ids[b]``).  A row with a budget m_b is finished by the sampler
    launch that writes its m_b-th token and emits ``pad_token_id`` from then on, exactly like a row that drew an EOS: budgets make
    the loop able to finish, so the stop poll runs; ``pad_launches`` then counts m_b valid tokens with no further bookkeeping, and
    the ``skip`` snapshot keeps the log-prob slots behind the budget at 0.0 / -1.  With an automaton a spent budget is told from
    a dead end by the launch's kept count (0: no candidate), also when both fall into one launch.  With ``row_options`` the presence
    and frequency penalties are the rows' resolved ones alone: the shaping launch runs for a bias or a row's penalty, never for the
    call's scalar that every row overrode.  None, or B empty dicts: no buffer, no upload, the entry points above.
    ``penalty_alpha`` / ``output_contrast`` (check_contrast_args): contrastive search; the resolved dict travels as
    ``LoopOptions.contrast`` and it is contrast_loop, not generate_loop, that runs such a call.  None: nothing of it exists."""
    kw = _keywords(locals(), "vocab", "batch")
    cons = check_constraint_args(vocab, **_own(check_constraint_args, kw))
    check_logprob_args(vocab, **_own(check_logprob_args, kw))
    starts = check_automaton_args(vocab, batch, **_own(check_automaton_args, kw))
    shape = check_shape_args(vocab, batch, **_own(check_shape_args, kw))
    truncation = check_truncation_args(**_own(check_truncation_args, kw))
    contrast = check_contrast_args(vocab, **_own(check_contrast_args, kw))
    rows = check_row_options(vocab, batch, **_own(check_row_options, kw))
    return LoopOptions.resolved(kw, cons, starts, shape, truncation, check_guidance_args(batch, **_own(check_guidance_args, kw)), rows,
                                contrast)


def generate_loop(decoder, prec: str, state: dict, logits: torch.Tensor, prompt_tokens: torch.Tensor, max_new_tokens: int,
                  opts: LoopOptions, *, pos_shift: int = 0, lengths=None, text_lengths=None, prompt_rows=None, pad_launches=None):
    """The plain loop on a prefilled state; ``opts``: what the caller asked for, resolved (LoopOptions; loop_options says what the
    loop does with each option).  Nothing is validated here but the shape of a guided batch.
    ``logits`` [B, T, V]: the prefill's output, ``state`` the incremental state it filled (state["len"] == T).
    ``prompt_rows`` = T (a chunked prefill, _prefill): ``logits`` is [B, 1, V] instead and holds only the row each sequence
    reads — the last position, or lengths[b] - 1 of a ragged row.
    ``prompt_tokens`` [B, Tt] int64: what the repetition penalty sees before the first new token.  ``pos_shift`` > 0: the
    prompt holds that many spliced rows that are not tokens and text rows carry two position rows (the multimodal prompt
    under u1_inplace_alias): a token at sequence position t is embedded with pos[2 + t - pos_shift] + pos[2 + t].
    ``lengths`` (host ints, validated by resolve_prompt_lengths): the ragged batch — row b's sequence has lengths[b] <= T
    positions (spliced rows included), the rest of its prompt is right padding whose ids mask_padding replaced.
    ``text_lengths`` (ragged batches; default ``lengths``): row b's number of prompt TOKENS, what the constraints' history holds.
    ``pad_launches`` (sessions; ragged batches only): an int32 [B] device tensor, zero on entry.  Before every sampler launch — after
    the step's constraint launch — the ``finished`` bytes are added to it, so that row b entered n - pad_launches[b] of the n
    sampler launches unfinished: its valid tokens, an EOS or the last token of a stop sequence included.  It is read back once,
    after the loop, in the same copy as the step kernels' error word, and left in state["turn"] = (n, [pad launches per row]).
    Under guidance (``opts.guidance``) ``logits``, ``prompt_tokens``, ``lengths`` and ``text_lengths`` hold 2B rows.
    Returns the tokens int64 [B, n]; then the fp32 [B, n, V] logits with ``output_logits`` (under guidance followed by the fp32
    [B, n, V] unconditional logits); then with ``output_logprobs`` the fp32
    [B, n] token_logprobs and, k > 0, the fp32 [B, n, k] top_logprobs and int64 [B, n, k] top_ids."""
    eos_token_id, pad_token_id, eos_poll, sequence_ids = opts.eos_token_id, opts.pad_token_id, opts.eos_poll, opts.sequence_ids
    output_logits, output_logprobs, k = opts.output_logits, opts.output_logprobs, int(opts.top_logprobs)
    cons, shape, guide, rows = opts.constraints, opts.shape, opts.guidance, opts.rows
    token_automaton, auto = opts.automaton or (None, None)
    R, T, V = logits.shape                                                # R: the rows of the step; B: the rows of the sampler
    B = R if guide is None else R // 2
    if guide is not None and (R % 2 or lengths is None or len(lengths) != R or pad_launches is not None):
        raise ValueError(f"guidance_scale = {guide!r} takes the 2B-row ragged batch of run_generate: conditional rows, then "
                         "unconditional rows, ``lengths`` for all of them, no ``pad_launches``")
    gathered = prompt_rows is not None
    if gathered:
        T = prompt_rows
    dev = logits.device
    budgets = rows is not None and any(r["max_new_tokens"] for r in rows)
    row_penalties = rows is not None and any(r["presence_penalty"] != 0.0 or r["frequency_penalty"] != 0.0 for r in rows)
    can_finish = eos_token_id is not None or (cons is not None and cons["stop"]) or auto is not None or budgets
    if rows is None:
        shaping = shape is not None and shape["launch"]
    else:                                                                 # the penalties are the rows' own: the call's scalars are resolved into them
        shaping = row_penalties or (shape is not None and shape["bias"] is not None)
    out = torch.full((B, max_new_tokens), int(pad_token_id), dtype=torch.int64, device=dev)
    nxt = torch.empty(R, dtype=torch.int64, device=dev)
    finished = torch.zeros(B, dtype=torch.uint8, device=dev)
    history = None
    prompt_tokens = prompt_tokens[:B]                                     # (guidance: the histories see the conditional prompts)
    Tt = prompt_tokens.shape[1]
    if (float(opts.repetition_penalty) != 1.0 or (cons is not None and cons["reads_history"])
            or (rows is not None and any(r["repetition_penalty"] != 1.0 for r in rows))):
        history = torch.empty((B, Tt + max_new_tokens), dtype=torch.int64, device=dev)           # (the sampler appends with r == 1 too)
        history[:, :Tt] = prompt_tokens
    if sequence_ids is not None:
        sequence_ids = sequence_ids.to(device=dev, dtype=torch.int64).contiguous()
    kept, kept_u = [], []
    lp = top_lp = top_ids = snap = None
    if output_logprobs:                                                   # every buffer before the first step
        lp = torch.zeros((B, max_new_tokens), dtype=torch.float32, device=dev)
        if k > 0:
            top_lp = torch.zeros((B, max_new_tokens, k), dtype=torch.float32, device=dev)
            top_ids = torch.full((B, max_new_tokens, k), -1, dtype=torch.int64, device=dev)
        if can_finish:
            snap = torch.empty(B, dtype=torch.uint8, device=dev)          # ``finished`` as the sampler launch met it
    if auto is not None and pad_launches is not None and snap is None:
        snap = torch.empty(B, dtype=torch.uint8, device=dev)
    positions = None
    if lengths is not None:
        # Row b's first token comes from logits[b, lengths[b] - 1]; from here on its position lives on the device.  The padded
        # history slots already hold the row's own first prompt token (mask_padding): the penalty is applied once per distinct
        # id, so the duplicates change nothing and every row keeps the common hist_len.
        last = torch.tensor([l - 1 for l in lengths], dtype=torch.int64, device=dev)
        row = logits[:, 0] if gathered else logits[torch.arange(R, device=dev), last]   # [R, V]
        positions = torch.tensor(lengths, dtype=torch.int32, device=dev)
        state.update(positions=positions, pos_max=max(lengths))
        decoder._ragged_scratch(state, dev, rows=R)                       # (before the first sampler launch: no fill between steps)
        err = state["error"]                                              # the step kernels' sticky error word
    else:
        row = logits[:, -1]                                               # [B, V] view, row stride T * V
    if cons is not None:                                                  # the one upload: CSR tables and the rows' text lengths
        bad, stop = (ops.SequenceTable(cons[k], dev) if cons[k] else None for k in ("bad", "stop"))
        plens = None
        if lengths is not None:
            plens = torch.tensor((lengths if text_lengths is None else text_lengths)[:B], dtype=torch.int32, device=dev)
    if auto is not None:                                                  # the one upload: the automaton's tables and the start states
        table = ops.AutomatonTable(*token_automaton.tables(), dev)
        states = (torch.tensor(auto, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        not_eos = -1 if eos_token_id is None else int(eos_token_id)
    if shaping:                                                           # the one upload: the bias table; the counts start at zero
        bias = ops.BiasTable(shape["bias"], dev) if shape is not None and shape["bias"] is not None else None
        if rows is None:
            shaper = dict(frequency_penalty=shape["frequency"], presence_penalty=shape["presence"])
            penalised = shape["frequency"] != 0.0 or shape["presence"] != 0.0
        else:
            shaper, penalised = {}, row_penalties                         # (every row resolved to 0: a bias alone, zero scalars)
        counts = torch.zeros((B, V), dtype=torch.int32, device=dev) if penalised else None
        if row_penalties:                                                 # the rows' own penalties, uploaded once
            shaper = dict(frequency_rows=torch.tensor([r["frequency_penalty"] for r in rows], dtype=torch.float32, device=dev),
                          presence_rows=torch.tensor([r["presence_penalty"] for r in rows], dtype=torch.float32, device=dev))
    # what the sampler and every row editor see: all R rows, or under guidance the first B of them (views, taken once)
    spos, snxt = (positions, nxt) if guide is None else (positions[:B], nxt[:B])
    # the sampler launch's arguments that every token shares (opts.sampler: what it takes beyond its old arguments)
    sampler = dict(temperature=opts.temperature, top_k=opts.top_k, top_p=opts.top_p, repetition_penalty=opts.repetition_penalty,
                   do_sample=opts.do_sample, seed=opts.seed, sequence_ids=sequence_ids, history=history, finished=finished,
                   eos_token_id=eos_token_id, pad_token_id=pad_token_id, out_tokens=out, **opts.sampler)
    if rows is not None:                                                  # the one upload: the rows' records, packed by the library
        sampler["rows"] = ops.SampleRowTable([{k: r[k] for k in ops.SampleRowTable.FIELDS} for r in rows], V, dev)
        if budgets and auto is not None and snap is not None:             # a dead end and a spent budget both finish a row on a non-EOS token:
            sampler["kept_count"] = live = torch.empty(B, dtype=torch.int32, device=dev)   # the launch's kept count tells them apart
    n = 0
    for g in range(max_new_tokens):
        constrained = cons is not None and (cons["every_step"] or g < cons["min_new"])
        step_rows = row
        if guide is not None:
            row = step_rows[:B]                                           # the conditional rows; step_rows[B:] are the unconditional ones
        raw = row
        if output_logits:
            kept.append(row.clone())                                      # the model's own logits: before any ban (the sampler only reads the row)
            raw = kept[-1]
            if guide is not None:
                kept_u.append(step_rows[B:].clone())
        elif output_logprobs and (constrained or auto is not None or shaping or guide is not None):
            raw = row.clone()                                             # (the guidance, constraint, automaton and shaping launches edit the row in place)
        if guide is not None:                                             # the guided row over the conditional one; the unconditional positions move on
            ops.guidance_logits(row, step_rows[B:], scale=guide, finished=finished, positions=positions[B:], advance=int(g > 0))
        if constrained:
            ops.constrain_logits(row, history=history, hist_len=Tt + g if history is not None else 0, prompt_width=Tt,
                                 prompt_lens=plens if history is not None else None, new_tokens=g,
                                 no_repeat_ngram_size=cons["ngram"], bad_words=bad, stop_sequences=stop,
                                 min_new_tokens=cons["min_new"], eos_token_id=eos_token_id, finished=finished)
        if auto is not None:
            ops.automaton_step(row, table, states[g & 1], states[1 - (g & 1)], last_token=snxt if g else None, finished=finished)
        if shaping:
            ops.shape_logits(row, bias=bias, counts=counts, last_token=snxt if g else None, finished=finished, **shaper)
        if pad_launches is not None:
            pad_launches.add_(finished)                                   # (rows that enter this launch finished: it writes their pad)
        if snap is not None:
            snap.copy_(finished)
        if positions is not None:                                         # Philox position lengths[b] + g, kept in positions[b]
            ops.sample_logits(row, positions=spos, advance=int(g > 0), hist_len=Tt + g, out=snxt, out_col=g, **sampler)
            if guide is not None:
                nxt[B:].copy_(snxt)                                       # both rows of a pair are fed the token just sampled
        else:
            ops.sample_logits(row, position=T + g, hist_len=Tt + g, out=nxt, out_col=g, **sampler)
        if auto is not None and snap is not None:
            # a row this launch finished on a token other than the EOS had no candidate: what it emitted is a pad, no token of the row
            dead = (finished - snap) * (snxt != not_eos)
            if budgets:
                dead = dead * (live == 0)                                 # (a row its budget finished drew from at least one candidate)
            if pad_launches is not None:
                pad_launches.add_(dead)
            if output_logprobs:
                snap.add_(dead)                                           # (its log-prob slots stay 0.0 / -1)
        if output_logprobs:
            ops.step_logprobs(raw, snxt, out=lp, col=g, skip=snap, top_n=k, top_out=top_lp, top_ids=top_ids)
        n = g + 1
        if n == max_new_tokens:
            break
        if can_finish and eos_poll > 0 and n % eos_poll == 0:
            if positions is None:
                if bool(finished.all()):
                    break                                                 # the loop's only device-to-host read
            else:                                                         # ... which also brings the step kernels' error word
                done, word = torch.stack([finished.min().to(torch.int32), err[0]]).tolist()
                _raise_position_error(word, state)
                if done:
                    break
        if positions is not None:
            row = decoder._forward_incremental(None, state, None, prec, next_token=nxt, pos_shift=pos_shift)[:, 0]
            continue
        t = T + g
        pos = (t - pos_shift, t) if pos_shift else (t, -1)
        row = decoder._forward_incremental(None, state, None, prec, next_token=nxt, next_pos=pos)[:, 0]
    if pad_launches is not None:                                          # the turn's one read: the error word and the counts
        word, *pads = torch.cat([err, pad_launches]).tolist()
        _raise_position_error(word, state)
        state["turn"] = (n, pads)
    elif positions is not None:
        _raise_position_error(int(err.item()), state)                     # device positions are validated by the kernels, not here
    res = [out[:, :n]]
    if output_logits:
        res.append(torch.stack(kept, dim=1))
        if guide is not None:
            res.append(torch.stack(kept_u, dim=1))                        # the unconditional rows' raw logits, directly after
    if output_logprobs:
        res.append(lp[:, :n])
        if k > 0:
            res += [top_lp[:, :n], top_ids[:, :n]]
    return res[0] if len(res) == 1 else tuple(res)


MAX_BEAMS = 16
MAX_NGRAM = MAX_SEQUENCE = 64           # kx_constrain_logits' limits
FP32_MAX = 3.4028234663852886e38


def _finite_fp32(v) -> bool:
    """Whether ``v`` is a number (a bool is none) that is finite in fp32."""
    return not isinstance(v, bool) and isinstance(v, (int, float)) and abs(v) <= FP32_MAX


def _host_ints(v, count: int, name: str, per: str, joint: bool = False) -> list:
    """``v``, a sequence of ``count`` integers or an integer tensor -> the host list, or ValueError naming ``name``.  ``per``: what
    an entry stands for; ``joint``: a tensor's dtype and shape are refused in one message.  Host data is taken as it is; a device
    tensor is read back once."""
    if isinstance(v, torch.Tensor):
        integers = not (v.is_floating_point() or v.is_complex() or v.dtype == torch.bool)
        if joint and not (integers and v.dim() == 1):
            raise ValueError(f"{name} must be {count} integers, got a {v.dtype} tensor of shape {tuple(v.shape)}")
        if not integers:
            raise ValueError(f"{name} must hold integers, got a {v.dtype} tensor")
        if v.dim() != 1:
            raise ValueError(f"{name} must have {count} entries, got shape {tuple(v.shape)}")
        out = v.tolist()                                   # (the one read of a device tensor)
    else:
        try:
            out = [operator.index(i) for i in v]
        except TypeError:
            raise ValueError(f"{name} must be a sequence of {count} integers or an integer tensor, got {v!r}") from None
    if len(out) != count:
        raise ValueError(f"{name} must have {count} entries (one per {per}), got {len(out)}")
    return out


def _check_sequences(name: str, seqs, vocab: int) -> list:
    if seqs is None:
        return []
    if isinstance(seqs, (str, bytes)) or not hasattr(seqs, "__iter__"):
        raise ValueError(f"{name} must be a list of non-empty lists of token ids, got {seqs!r}")
    out = []
    for k, s in enumerate(seqs):
        try:
            ids = [operator.index(t) for t in s]
        except TypeError:
            raise ValueError(f"{name}[{k}] must be a list of integer token ids, got {s!r}") from None
        if not ids:
            raise ValueError(f"{name}[{k}] is empty: a sequence holds at least one token id")
        if len(ids) > MAX_SEQUENCE:
            raise ValueError(f"{name}[{k}] holds {len(ids)} ids, more than {MAX_SEQUENCE}")
        for t in ids:
            if not 0 <= t < vocab:
                raise ValueError(f"{name}[{k}] holds the id {t}, outside the vocabulary [0, {vocab})")
        out.append(ids)
    return out


def check_constraint_args(vocab: int, *, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0, stop_sequences=None,
                          eos_token_id=None, num_beams=None):
    """ValueError (naming the argument) for what generate() refuses of the constraint arguments, before anything is launched.
    ``num_beams``: given (not None) when the call runs beam search, which offers the history-free constraints only.
    Returns None when every constraint is at its default (no kx_constrain_logits launch is issued), else a dict: ngram, bad,
    stop, min_new, reads_history (a history buffer is needed), every_step (something besides the minimum length is on)."""
    for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
    if no_repeat_ngram_size > MAX_NGRAM:
        raise ValueError(f"no_repeat_ngram_size = {no_repeat_ngram_size} exceeds {MAX_NGRAM}")
    bad = _check_sequences("bad_words_ids", bad_words_ids, vocab)
    stop = _check_sequences("stop_sequences", stop_sequences, vocab)
    if min_new_tokens > 0 and eos_token_id is None:
        raise ValueError(f"min_new_tokens = {min_new_tokens} needs an eos_token_id: it is the token the minimum length bans")
    if num_beams is not None:
        for name, on in (("no_repeat_ngram_size", no_repeat_ngram_size > 0), ("bad_words_ids", any(len(s) > 1 for s in bad)),
                         ("stop_sequences", bool(stop))):
            if on:
                raise ValueError(f"{name}{' with more than one id per entry' if name == 'bad_words_ids' else ''} is not offered "
                                 f"together with beam search (num_beams = {num_beams}): it needs a per-beam history; see DESIGN.md §7b")
    if not (no_repeat_ngram_size or bad or stop or min_new_tokens):
        return None
    reads = bool(no_repeat_ngram_size or stop or any(len(s) > 1 for s in bad))
    return dict(ngram=no_repeat_ngram_size, bad=bad, stop=stop, min_new=min_new_tokens, reads_history=reads,
                every_step=bool(no_repeat_ngram_size or bad or stop))


MAX_TOP_LOGPROBS = 16                   # kx_step_logprobs' top_n limit


def check_logprob_args(vocab: int, *, output_logprobs=False, top_logprobs=0, beams=False, drafts=0) -> int:
    """ValueError (naming the argument) for what generate() refuses of the log-prob arguments, before the device check and any
    launch.  ``beams``: the call runs beam search; ``drafts``: its prompt-lookup drafts per step.  Returns ``top_logprobs``."""
    k = top_logprobs
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= MAX_TOP_LOGPROBS:
        raise ValueError(f"top_logprobs must be an integer in 0..{MAX_TOP_LOGPROBS}, got {k!r}")
    if k > vocab:
        raise ValueError(f"top_logprobs = {k} exceeds the vocabulary of {vocab}")
    if k > 0 and not output_logprobs:
        raise ValueError(f"top_logprobs = {k} lists the alternatives next to each token's log-prob: it needs output_logprobs=True")
    if output_logprobs and beams:
        raise ValueError("output_logprobs is not offered together with beam search (num_beams > 1): beams report output_scores; "
                         "see DESIGN.md §8")
    if output_logprobs and drafts:
        raise ValueError(f"output_logprobs is not offered together with prompt-lookup speculation (prompt_lookup_num_tokens = {drafts}): "
                         "a verify step emits a varying number of tokens per row; see DESIGN.md §8")
    return k


def check_automaton_args(vocab: int, batch: int, *, token_automaton=None, automaton_start=None, prompt_lookup_num_tokens=0):
    """ValueError (naming ``token_automaton`` or ``automaton_start``) for what generate() refuses of the automaton arguments, before
    the device check and any launch.  ``batch``: the prompts of the call.  Returns None without an automaton (no buffer, no launch),
    else the host list of the rows' start states [batch]."""
    from .automaton import TokenAutomaton
    if token_automaton is None:
        if automaton_start is not None:
            raise ValueError("automaton_start gives every row's start state in a token_automaton: it needs one")
        return None
    if not isinstance(token_automaton, TokenAutomaton):
        raise ValueError(f"token_automaton must be a kosmosx.automaton.TokenAutomaton (or None), got {type(token_automaton).__name__}")
    try:
        token_automaton.check_vocab(vocab)
    except ValueError as e:
        raise ValueError(f"token_automaton: {e}") from None
    if prompt_lookup_num_tokens not in (0, None):
        raise ValueError(f"token_automaton is not offered together with prompt-lookup speculation (prompt_lookup_num_tokens = "
                         f"{prompt_lookup_num_tokens}): a verify step emits a varying number of tokens per row, the state would have to "
                         "advance by as many; see DESIGN.md §8")
    S = token_automaton.num_states
    if automaton_start is None:
        return [token_automaton.start] * batch
    starts = _host_ints(automaton_start, batch, "automaton_start", "row", joint=True)
    for b, s in enumerate(starts):
        if not 0 <= s < S:
            raise ValueError(f"automaton_start[{b}] = {s} is outside the automaton's {S} states")
    return starts


def check_shape_args(vocab: int, batch: int, *, logit_bias=None, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0, num_beams=1,
                     prompt_lookup_num_tokens=0):
    """ValueError (naming ``logit_bias``, ``presence_penalty``, ``frequency_penalty`` or ``min_p``) for what generate() refuses of
    the shaping arguments, before the device check and any launch.  ``batch``: the rows the biases are given for.  Returns None
    with everything at its default (no buffer, no launch, the sampler's old entry points), else a dict: ``bias`` (None, or
    ``batch`` lists of (id, value) sorted by id — one dict is repeated for every row), ``frequency``, ``presence``, ``min_p``
    (floats) and ``launch`` (whether a bias or a penalty asks for the kx_shape_logits launch; min_p alone does not)."""
    import math
    out = dict(bias=None)
    for name, v in (("presence_penalty", presence_penalty), ("frequency_penalty", frequency_penalty), ("min_p", min_p)):
        if not _finite_fp32(v):
            raise ValueError(f"{name} must be a finite number (in fp32), got {v!r}")
        out[name.split("_")[0] if name != "min_p" else name] = float(v)
    if not 0.0 <= out["min_p"] <= 1.0:
        raise ValueError(f"min_p = {min_p!r} must be in [0, 1] (0 = off)")
    if logit_bias is not None:
        rows = [logit_bias] * batch if hasattr(logit_bias, "items") else list(logit_bias)
        if len(rows) != batch:
            raise ValueError(f"logit_bias must be one dict {{id: value}} or a sequence of {batch} dicts (one per row), got {len(rows)}")
        bias = []
        for b, r in enumerate(rows):
            if not hasattr(r, "items"):
                raise ValueError(f"logit_bias[{b}] must be a dict {{id: value}}, got {type(r).__name__}")
            ent = {}
            for i, v in r.items():
                try:
                    i, v = operator.index(i), float(v)
                except (TypeError, ValueError):
                    raise ValueError(f"logit_bias[{b}]: {i!r}: {v!r} is no (integer id, number) pair") from None
                if not 0 <= i < vocab:
                    raise ValueError(f"logit_bias[{b}]: id {i} is outside the vocabulary of {vocab}")
                if i in ent:
                    raise ValueError(f"logit_bias[{b}]: id {i} is listed twice")
                if not (v == -math.inf or _finite_fp32(v)):
                    raise ValueError(f"logit_bias[{b}][{i}] = {v} must be finite (in fp32) or -inf (a ban)")
                ent[i] = v
            bias.append(sorted(ent.items()))
        if any(bias):
            out["bias"] = bias
    names = [n for n, on in (("logit_bias", out["bias"] is not None), ("presence_penalty", out["presence"] != 0.0),
                             ("frequency_penalty", out["frequency"] != 0.0), ("min_p", out["min_p"] != 0.0)) if on]
    if not names:
        return None
    if num_beams not in (1, None):
        raise ValueError(f"{', '.join(names)}: not offered together with num_beams = {num_beams}: beams rank log-probs, and how a "
                         "bias or a penalty enters that score is a decision of its own; see DESIGN.md §8")
    if prompt_lookup_num_tokens not in (0, None):
        raise ValueError(f"{', '.join(names)}: not offered together with prompt-lookup speculation (prompt_lookup_num_tokens = "
                         f"{prompt_lookup_num_tokens}): a verify step emits a varying number of tokens per row; see DESIGN.md §8")
    out["launch"] = names != ["min_p"]
    return out


def check_truncation_args(*, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, num_beams=1, prompt_lookup_num_tokens=0):
    """ValueError (naming ``typical_p``, ``epsilon_cutoff`` or ``eta_cutoff``) for what generate() refuses of the truncation
    samplers, before the device check and any launch: ``typical_p`` outside (0, 1] (1 = off), a cut-off outside [0, 1) (0 = off), a
    bool or a non-number, and any of them together with beams or prompt lookup.  Returns the keywords ops.sample_logits takes for
    the ones that are switched on — an empty dict at the defaults: the sampler's old entry points."""
    given, out = locals(), {}
    for name, off, low_open in (("typical_p", 1.0, True), ("epsilon_cutoff", 0.0, False), ("eta_cutoff", 0.0, False)):
        v = given[name]
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{name} must be a number, got {v!r}")
        v = float(v)
        if low_open and not 0.0 < v <= 1.0:
            raise ValueError(f"typical_p = {v!r} must be in (0, 1] (1 = off)")
        if not low_open and not 0.0 <= v < 1.0:
            raise ValueError(f"{name} = {v!r} must be in [0, 1) (0 = off)")
        if v != off:
            out[name] = v
    if not out:
        return out
    if num_beams not in (1, None):
        raise ValueError(f"{', '.join(out)}: not offered together with num_beams = {num_beams}: beams rank log-probs and do not "
                         "sample; see DESIGN.md §8")
    if prompt_lookup_num_tokens not in (0, None):
        raise ValueError(f"{', '.join(out)}: not offered together with prompt-lookup speculation (prompt_lookup_num_tokens = "
                         f"{prompt_lookup_num_tokens}): its verify step is greedy; see DESIGN.md §8")
    return out


ROW_KEYS = ("do_sample", "temperature", "top_k", "top_p", "repetition_penalty", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff",
            "seed", "presence_penalty", "frequency_penalty", "max_new_tokens")


def _row_value(key: str, v, vocab: int, limit):
    """One value of a row's dict under the rules of the scalar keyword ``key`` -> the value as the table holds it, or ValueError.
    ``limit``: the call's ``max_new_tokens`` (None: no upper bound is checked)."""
    import ctypes
    if key == "do_sample":
        if not isinstance(v, bool):
            raise ValueError(f"must be True or False, got {v!r}")
        return v
    if key in ("top_k", "seed", "max_new_tokens"):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"must be an integer, got {v!r}")
        if key == "top_k" and not -2 ** 31 <= v < 2 ** 31:
            raise ValueError(f"{v} does not fit 32 bits")
        if key == "max_new_tokens" and (v < 1 or (limit is not None and v > limit)):
            raise ValueError(f"{v} must be in 1..{limit if limit is not None else 'max_new_tokens'}, the call's max_new_tokens: a row "
                             "may end early, not run longer")
        return v
    if key in ("presence_penalty", "frequency_penalty", "min_p"):        # check_shape_args' own rules, on a batch of one
        out = check_shape_args(vocab, 1, **{key: v}, num_beams=None, prompt_lookup_num_tokens=None)
        return 0.0 if out is None else out[key.split("_")[0] if key != "min_p" else key]
    if key in ("typical_p", "epsilon_cutoff", "eta_cutoff"):             # check_truncation_args' own rules
        check_truncation_args(**{key: v}, num_beams=None, prompt_lookup_num_tokens=None)
        return float(v)
    # temperature, top_p, repetition_penalty: what kx_sample_logits asks of them, on the value the fp32 field will hold
    if not _finite_fp32(v):
        raise ValueError(f"must be a finite number (in fp32), got {v!r}")
    f = ctypes.c_float(v).value
    if key == "temperature" and not f >= 0.0:
        raise ValueError(f"{v!r} must be >= 0 (0 = greedy)")
    if key != "temperature" and not f > 0.0:
        raise ValueError(f"{v!r} must be > 0 (in fp32)")
    return float(v)


def check_row_options(vocab: int, batch: int, *, row_options=None, max_new_tokens=None, num_beams=1, prompt_lookup_num_tokens=0,
                      num_return_sequences=1, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seed=0,
                      min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, presence_penalty=0.0, frequency_penalty=0.0):
    """ValueError (naming ``row_options``, and ``row_options[b]['key']`` for a value) for what generate() refuses of the per-row
    options, before the device check and any launch; after check_truncation_args, so the call's own scalars are already known to be
    good.  ``row_options``: None, or ``batch`` dicts — row b's overrides of any of ROW_KEYS; a key a row does not name takes the
    call's own keyword (``max_new_tokens``: the call's positional value, i.e. no budget).  A value is refused exactly where the
    scalar keyword refuses it — the same ranges, the same bool / non-number / non-finite rules — and for temperature, top_p and
    repetition_penalty, which the scalar path hands to the library unchecked, where kx_sample_logits refuses the fp32 value.
    ``max_new_tokens`` = m_b needs 1 <= m_b <= the call's (``max_new_tokens``, when an integer is given).  Not offered with
    ``num_beams`` > 1 or ``prompt_lookup_num_tokens`` > 0, and a row resolved to greedy is refused under ``num_return_sequences`` > 1
    as scalar greedy is.
    Returns None when there is nothing to do (None, or every dict empty: no buffer, no upload, the old entry points), else the
    resolved table: ``batch`` dicts holding every ROW_KEYS entry, ``max_new_tokens`` 0 where the row has no budget."""
    if row_options is None:
        return None
    if isinstance(row_options, (str, bytes)) or hasattr(row_options, "items") or not hasattr(row_options, "__iter__"):
        raise ValueError(f"row_options must be a sequence of {batch} dicts (one per row) or None, got {type(row_options).__name__}")
    given = list(row_options)
    if len(given) != batch:
        raise ValueError(f"row_options must have {batch} entries (one dict per row), got {len(given)}")
    for b, r in enumerate(given):
        if not hasattr(r, "items"):
            raise ValueError(f"row_options[{b}] must be a dict of overrides, got {type(r).__name__}")
        for key in r:
            if key not in ROW_KEYS:
                raise ValueError(f"row_options[{b}][{key!r}]: unknown key; a row may name {', '.join(ROW_KEYS)}")
    if num_beams not in (1, None):
        raise ValueError(f"row_options is not offered together with num_beams = {num_beams}: beams rank log-probs and do not sample; see "
                         "DESIGN.md §8")
    if prompt_lookup_num_tokens not in (0, None):
        raise ValueError(f"row_options is not offered together with prompt-lookup speculation (prompt_lookup_num_tokens = "
                         f"{prompt_lookup_num_tokens}): its verify step is greedy and emits a varying number of tokens per row; see "
                         "DESIGN.md §8")
    # (a call's max_new_tokens that is no positive integer is refused by its own check, in its own words: no bound is taken from it)
    limit = max_new_tokens if isinstance(max_new_tokens, int) and not isinstance(max_new_tokens, bool) and max_new_tokens >= 1 else None
    call = dict(do_sample=bool(do_sample), temperature=float(temperature), top_k=int(top_k), top_p=float(top_p),
                repetition_penalty=float(repetition_penalty), min_p=float(min_p), typical_p=float(typical_p),
                epsilon_cutoff=float(epsilon_cutoff), eta_cutoff=float(eta_cutoff), seed=int(seed),
                presence_penalty=float(presence_penalty), frequency_penalty=float(frequency_penalty), max_new_tokens=0)
    rows = []
    for b, r in enumerate(given):
        row = dict(call)
        for key, v in r.items():
            try:
                row[key] = _row_value(key, v, vocab, limit)
            except ValueError as e:
                raise ValueError(f"row_options[{b}][{key!r}]: {e}") from None
        if num_return_sequences not in (1, None) and (not row["do_sample"] or row["temperature"] == 0.0):
            raise ValueError(f"row_options[{b}] resolves to greedy (do_sample = {row['do_sample']}, temperature = {row['temperature']}) "
                             f"under num_return_sequences = {num_return_sequences}: greedy copies of one prompt would all be equal")
        rows.append(row)
    return rows if any(given) else None


def check_guidance_args(batch: int, *, guidance_scale=1.0, negative_prompt_ids=None, negative_prompt_lengths=None, negative_images=None,
                        min_len: int = 1, multimodal: bool = False, num_beams=1, prompt_lookup_num_tokens=0, num_return_sequences=1,
                        return_session=False):
    """ValueError (naming ``guidance_scale``, ``negative_prompt_ids``, ``negative_prompt_lengths`` or ``negative_images``) for what
    generate() refuses of the guidance arguments; host only, before the device check and any launch.  ``batch``: the sequences B
    (the step then runs 2B rows); ``min_len``: the model's shortest prompt; ``multimodal``: Kosmos, which takes ``negative_images``
    and needs at least one negative.  Returns None with the scale at 1.0 (no launch, no buffer, nothing doubled), else a dict:
    ``scale`` (float) and ``lengths`` (the negative prompts' host lengths where they could be checked without a device read, else
    None: an integer tensor is resolved after the device check, as ``prompt_lengths`` is)."""
    s = guidance_scale
    if not _finite_fp32(s):
        raise ValueError(f"guidance_scale must be a finite number (in fp32; 1.0 = off), got {s!r}")
    given = [n for n, v in (("negative_prompt_ids", negative_prompt_ids), ("negative_prompt_lengths", negative_prompt_lengths),
                            ("negative_images", negative_images)) if v is not None]
    if float(s) == 1.0:
        if given:
            raise ValueError(f"{', '.join(given)}: given without a guidance_scale other than 1.0 (1.0 turns guidance off)")
        return None
    for name, on in ((f"num_beams = {num_beams}", num_beams not in (1, None)),
                     (f"prompt-lookup speculation (prompt_lookup_num_tokens = {prompt_lookup_num_tokens})",
                      prompt_lookup_num_tokens not in (0, None)),
                     (f"num_return_sequences = {num_return_sequences}", num_return_sequences not in (1, None)),
                     ("return_session", bool(return_session))):
        if on:
            raise ValueError(f"guidance_scale = {s!r}: guidance is not offered together with {name}: every sequence runs as a "
                             "conditional and an unconditional row of one ragged batch; see DESIGN.md §8")
    if negative_images is not None:
        if not multimodal:
            raise ValueError("negative_images: this model takes no images")
        if not isinstance(negative_images, torch.Tensor) or not negative_images.is_floating_point() or negative_images.dim() != 4 \
                or negative_images.shape[0] != batch:
            raise ValueError(f"negative_images must be a floating-point [{batch}, 3, H, W] tensor like images, got "
                             f"{tuple(negative_images.shape) if isinstance(negative_images, torch.Tensor) else type(negative_images).__name__}")
    if negative_prompt_ids is None and negative_prompt_lengths is not None:
        raise ValueError("negative_prompt_lengths: given without negative_prompt_ids")
    if multimodal and negative_prompt_ids is None and negative_images is None:
        raise ValueError(f"guidance_scale = {s!r} needs negative_prompt_ids or negative_images (or both): without either the "
                         "unconditional rows would repeat the conditional ones")
    lengths = None
    if negative_prompt_ids is not None:
        t = negative_prompt_ids
        if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError("negative_prompt_ids must be an integer tensor [batch, seq], got "
                             f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.dim() != 2 or t.shape[0] != batch:
            raise ValueError(f"negative_prompt_ids must be [batch, seq] with batch {batch} (one negative prompt per row), got {tuple(t.shape)}")
        if t.shape[1] < min_len:
            raise ValueError(f"negative_prompt_ids holds {t.shape[1]} token{'s' if t.shape[1] != 1 else ''} per row: a negative prompt "
                             f"has at least {min_len}" + (" (the image is spliced after two text tokens)" if min_len == 2 else ""))
        if isinstance(negative_prompt_lengths, torch.Tensor):
            p = negative_prompt_lengths
            if p.is_floating_point() or p.is_complex() or p.dtype == torch.bool:
                raise ValueError(f"negative_prompt_lengths must hold integers, got a {p.dtype} tensor")
            if tuple(p.shape) != (batch,):
                raise ValueError(f"negative_prompt_lengths must have {batch} entries, got shape {tuple(p.shape)}")
        elif negative_prompt_lengths is not None:
            lengths = resolve_prompt_lengths(negative_prompt_lengths, batch, t.shape[1], min_len=min_len, name="negative_prompt_lengths")
    return dict(scale=float(s), lengths=lengths)


def _guided_prompt(prompt: dict, prompt_lengths, guide: dict, *, negative_prompt_ids=None, negative_prompt_lengths=None):
    """The 2B-row prompt of a guided call: rows 0..B-1 are ``prompt``'s own (the conditional rows), rows B..2B-1 the unconditional
    ones — ``negative_prompt_ids``, or by default what prompt["negative_default"] names: the row's last prompt token ("last_token",
    the text model, as `transformers` does) or the row's own text ("own_text", the multimodal model under ``negative_images``) —
    right-padded to the wider of the two.  Returns the prompt dict with these tokens and the 2B host lengths, which _prefill takes
    as a ragged batch.  Runs after the device check; no host read unless a length was given as a device tensor."""
    tokens = prompt["tokens"].long()
    B, Tt = tokens.shape
    lens = [Tt] * B if prompt_lengths is None else resolve_prompt_lengths(prompt_lengths, B, Tt, min_len=prompt["min_len"])
    if negative_prompt_ids is not None:
        neg = negative_prompt_ids.long()
        nlens = guide["lengths"]
        if nlens is None:
            nlens = [neg.shape[1]] * B if negative_prompt_lengths is None else resolve_prompt_lengths(
                negative_prompt_lengths, B, neg.shape[1], min_len=prompt["min_len"], name="negative_prompt_lengths")
    elif prompt["negative_default"] == "last_token":
        neg = tokens.gather(1, torch.tensor([[l - 1] for l in lens], dtype=torch.int64, device=tokens.device))
        nlens = [1] * B
    else:
        neg, nlens = tokens, lens
    W = max(max(lens), max(nlens))
    both = torch.zeros((2 * B, W), dtype=torch.int64, device=tokens.device)     # (mask_padding replaces what lies behind a row's length)
    both[:B, :min(Tt, W)] = tokens[:, :W]
    both[B:, :min(neg.shape[1], W)] = neg[:, :W]
    return dict(prompt, tokens=both), lens + nlens


def check_beam_args(vocab: int, *, num_beams, length_penalty=1.0, num_return_sequences=1, do_sample=False, temperature=1.0,
                    top_k=0, top_p=1.0, repetition_penalty=1.0, prompt_lengths=None, sequence_ids=None, output_logits=False,
                    output_scores=False, output_trace=False, beam_path=False) -> bool:
    """ValueError (naming the argument) for what generate() refuses, before anything is launched.  Returns whether the call
    runs beam_loop: ``num_beams`` > 1, or ``beam_path`` (the internal switch that sends num_beams = 1 through it)."""
    if isinstance(num_beams, bool) or not isinstance(num_beams, int) or num_beams < 1:
        raise ValueError(f"num_beams must be a positive integer, got {num_beams!r}")
    if isinstance(num_return_sequences, bool) or not isinstance(num_return_sequences, int) or num_return_sequences < 1:
        raise ValueError(f"num_return_sequences must be a positive integer, got {num_return_sequences!r}")
    if num_return_sequences > num_beams and (num_beams > 1 or beam_path):
        raise ValueError(f"num_return_sequences = {num_return_sequences} exceeds num_beams = {num_beams}")
    if not (num_beams > 1 or beam_path):
        if num_return_sequences > 1 and not do_sample:         # (with sampling: parallel_loop, see check_parallel_args)
            raise ValueError(f"num_return_sequences = {num_return_sequences} without beams draws that many samples per prompt: it needs "
                             "do_sample=True (greedy copies of one prompt would all be equal)")
        for name, on in (("output_scores", output_scores), ("output_trace", output_trace)):
            if on:
                raise ValueError(f"{name} is an output of beam search: it needs num_beams > 1")
        return False
    if num_beams > MAX_BEAMS:
        raise ValueError(f"num_beams = {num_beams} exceeds {MAX_BEAMS}")
    if not float(length_penalty) >= 0.0:
        raise ValueError(f"length_penalty must be >= 0, got {length_penalty!r}")
    if 2 * num_beams > vocab:
        raise ValueError(f"num_beams = {num_beams}: a beam step ranks 2 * num_beams candidates, more than the vocabulary of {vocab}")
    for name, bad in (("do_sample", bool(do_sample)), ("temperature", float(temperature) != 1.0), ("top_k", int(top_k) != 0),
                      ("top_p", float(top_p) != 1.0), ("repetition_penalty", float(repetition_penalty) != 1.0),
                      ("prompt_lengths", prompt_lengths is not None), ("sequence_ids", sequence_ids is not None),
                      ("output_logits", bool(output_logits))):
        if bad:
            raise ValueError(f"{name} is not offered together with beam search (num_beams = {num_beams}); see DESIGN.md §7b")
    return True


def beam_loop(decoder, prec: str, state: dict, logits: torch.Tensor, max_new_tokens: int, *, num_beams: int, pos_shift: int = 0,
              length_penalty=1.0, early_stopping=False, num_return_sequences=1, eos_token_id=None, pad_token_id=1, eos_poll=8,
              output_scores=False, output_trace=False, bad_words_ids=None, min_new_tokens=0, prompt_rows=None, token_automaton=None,
              automaton_start=None):
    """Beam search after the prefill: ``logits`` [B, T, V] and ``state`` as for generate_loop (the prefill ran once per batch row;
    ``prompt_rows`` as there: ``logits`` [B, 1, V] holds the last position alone).
    Per token: kx_beam_step on the rows the last step wrote (step 0: the B prefill rows, one input beam each), kx_kv_cache_gather
    of cache rows 0:t into the other B * W-row cache by the step's src_row, then the uniform decode step at B * W rows and
    the common host position.  Every buffer is allocated before the first step; the host reads ``done.all()`` at the stop poll
    and the gather's error word after the loop, nothing else.
    ``bad_words_ids`` (single ids only) and ``min_new_tokens``: one kx_constrain_logits launch on the rows before the beam step,
    with no history — and before the ``output_trace`` copy, so the trace holds what the beam step ranked.
    ``token_automaton`` / ``automaton_start`` (check_automaton_args): one kx_automaton_step launch after it, before the trace copy too.
    Step 0 masks the B prefill rows from the start states (one input beam each); step g >= 1 runs at B * W rows, reads the state
    buffer step g - 1 wrote through that step's ``src_row`` — the states follow the backpointers — and advances on token[g - 1].  Two
    [B * W] buffers alternate.  A frozen row's or an unfilled slot's pad token leads wherever it leads, usually to the dead state:
    such beams offer no candidates anyway.  A hypothesis ends only by ``eos_token_id``; a state with no way out kills the beam, so a
    grammar for beams ends in an EOS edge (TokenAutomaton.from_choices(..., eos_token_id=...)).
    Returns tokens int64 [B, n] (R = 1) or [B, R, n], then the fp32 [B, R] scores with ``output_scores``, then the trace dict
    with ``output_trace`` (the contract: include/kosmosx_hip.h, "Beam search on the device")."""
    B, T, V = logits.shape
    if prompt_rows is not None:
        T = prompt_rows
    dev = logits.device
    W, R, N = int(num_beams), int(num_return_sequences), int(max_new_tokens)
    BW = B * W
    pad = int(pad_token_id)
    zeros = torch.zeros(B, dtype=torch.float32, device=dev)                  # the scores step 0 starts from
    score = torch.zeros((N, BW), dtype=torch.float32, device=dev)            # row g: the live scores after step g
    parent = torch.zeros((N, BW), dtype=torch.int32, device=dev)             # rows g of parent / token: step g's backpointers
    token = torch.full((N, BW), pad, dtype=torch.int64, device=dev)
    src_row = torch.zeros(BW, dtype=torch.int32, device=dev)
    pool = (torch.full((B, W), float("-inf"), dtype=torch.float32, device=dev), torch.zeros((B, W), dtype=torch.int32, device=dev),
            torch.zeros((B, W), dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    scratch = torch.empty(BW * 2 * W, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    out_tokens = torch.empty((B, R, N), dtype=torch.int64, device=dev)
    out_scores = torch.empty((B, R), dtype=torch.float32, device=dev)
    kept = torch.zeros((N, BW, V), dtype=torch.float32, device=dev) if output_trace else None
    src = (state["kcache"], state["vcache"])                                # the B-row prefill cache, dropped after step 0
    L, _, nh, Tmax, hd = src[0].shape
    caches = [tuple(torch.empty((L, BW, nh, Tmax, hd), dtype=src[0].dtype, device=dev) for _ in range(2)) for _ in range(2)]
    row = logits[:, -1]                                                      # [B, V] view, row stride T * V
    cons = check_constraint_args(V, bad_words_ids=bad_words_ids, min_new_tokens=min_new_tokens, eos_token_id=eos_token_id,
                                 num_beams=W)
    bad = ops.SequenceTable(cons["bad"], dev) if cons is not None and cons["bad"] else None
    auto = check_automaton_args(V, B, token_automaton=token_automaton, automaton_start=automaton_start)
    if auto is not None:
        table = ops.AutomatonTable(*token_automaton.tables(), dev)
        start = torch.tensor(auto, dtype=torch.int32, device=dev)
        states = tuple(torch.empty(BW, dtype=torch.int32, device=dev) for _ in range(2))
    n = 0
    for g in range(N):
        if cons is not None and (cons["every_step"] or g < cons["min_new"]):
            ops.constrain_logits(row, new_tokens=g, bad_words=bad, min_new_tokens=cons["min_new"], eos_token_id=eos_token_id)
        if auto is not None:
            if g == 0:
                ops.automaton_step(row, table, start, states[0][:B])
            else:                                                            # (src_row still holds step g - 1's rows)
                ops.automaton_step(row, table, states[1 - (g & 1)][:B] if g == 1 else states[1 - (g & 1)], states[g & 1],
                                   src_row=src_row, last_token=token[g - 1])
        if kept is not None:
            (kept[0].view(B, W, V)[:, 0] if g == 0 else kept[g]).copy_(row)
        ops.beam_step(row, zeros if g == 0 else score[g - 1], num_beams=W, step=g, pool=pool, done=done, scores_out=score[g],
                      next_token=token[g], parent=parent[g], src_row=src_row, scratch=scratch, length_penalty=length_penalty,
                      early_stopping=early_stopping, eos_token_id=eos_token_id, pad_token_id=pad)
        n = g + 1
        if n == N:
            break
        if eos_token_id is not None and eos_poll > 0 and n % eos_poll == 0 and bool(done.all()):
            break                                                            # the loop's only device-to-host read
        t = T + g
        dst = caches[g & 1]
        ops.kv_cache_gather(src[0], src[1], dst[0], dst[1], t, src_row, err)
        state.update(kcache=dst[0], vcache=dst[1], batch=BW)
        src = dst
        pos = (t - pos_shift, t) if pos_shift else (t, -1)
        row = decoder._forward_incremental(None, state, None, prec, next_token=token[g], next_pos=pos)[:, 0]
    ops.beam_finalize(score[n - 1], done, pool, parent, token, n, num_return_sequences=R, length_penalty=length_penalty,
                      eos_token_id=eos_token_id, pad_token_id=pad, out_tokens=out_tokens, out_scores=out_scores)
    if int(err.item()):                                                      # src_row is the beam step's own output
        raise RuntimeError("beam search: kx_kv_cache_gather met a source row outside the cache (KX_RAGGED_ERR_GATHER)")
    seqs = out_tokens[:, :, :n]
    res = [seqs[:, 0] if R == 1 else seqs]
    if output_scores:
        res.append(out_scores)
    if output_trace:
        res.append(dict(logits=kept[:n], parent=parent[:n], token=token[:n], score=score[:n], pool_score=pool[0], pool_end=pool[1],
                        pool_parent=pool[2], pool_count=pool[3], done=done))
    return res[0] if len(res) == 1 else tuple(res)


def check_parallel_args(*, num_return_sequences=1, beams=False, prompt_lookup_num_tokens=0, return_session=False) -> int:
    """ValueError (naming ``num_return_sequences``) for what generate() refuses of parallel sampling, before the device check and any
    launch; after check_beam_args, which validated the number and asked for ``do_sample``.  Returns n, the samples per prompt that
    parallel_loop draws (1: the call runs the loops it always ran)."""
    n = num_return_sequences
    if beams or n == 1:
        return 1
    for name, on in (("prompt-lookup speculation (prompt_lookup_num_tokens)", prompt_lookup_num_tokens not in (0, None)),
                     ("sessions (return_session)", bool(return_session))):
        if on:
            raise ValueError(f"num_return_sequences = {n} is not offered together with {name}: the samples share their prompt's cache "
                             "rows, which neither of them reads; see DESIGN.md §8")
    return n


def parallel_loop(decoder, prec: str, state: dict, logits: torch.Tensor, prompt_tokens: torch.Tensor, max_new_tokens: int,
                  opts: LoopOptions, *, num_return_sequences: int, pos_shift: int = 0, lengths=None, text_lengths=None, prompt_rows=None):
    """n = ``num_return_sequences`` sampled continuations of each of the B prefilled prompts: ``state``, ``logits``, ``prompt_tokens``,
    ``pos_shift``, ``lengths``, ``text_lengths`` and ``prompt_rows`` as generate_loop takes them after a prefill at B rows, ``opts``
    the options resolved for those B rows.  The state's caches become the read-only prefix caches of B * n rows (state["prefix"]):
    row b * n + i reads the len_b cache rows of sequence b and appends to its own sequence of the
    [L, B * n, heads, max_new_tokens, 64] tail caches.  The rows then run generate_loop's ragged branch — the first logits row, the prompt tokens, the lengths, the automaton's start states
    ([B]: prompt b's start goes to its n samples) and the per-prompt bias rows (prompt b's go to its n samples; every sample has
    its own counts; one dict given for every row is already one list repeated) repeated n times on the resolved lists, nothing
    parsed again, the positions on the device — so row b * n + i gets what row b * n + i of generate_loop on the caches repeated
    per sample gets, bit for bit.
    Returns what generate_loop returns, at B * n rows."""
    n, N = int(num_return_sequences), int(max_new_tokens)
    B, T, _ = logits.shape
    if prompt_rows is not None:
        T = prompt_rows
    dev = logits.device
    plens = [T] * B if lengths is None else list(lengths)
    tlens = [prompt_tokens.shape[1]] * B if lengths is None else list(plens if text_lengths is None else text_lengths)
    if prompt_rows is not None:
        first = logits[:, 0]
    else:
        first = logits[torch.arange(B, device=dev), torch.tensor([l - 1 for l in plens], dtype=torch.int64, device=dev)]
    kc = state["kcache"]
    L, _, nh, _, hd = kc.shape
    seq = [b for b in range(B) for _ in range(n)]
    if opts.automaton is not None:
        opts = dataclasses.replace(opts, automaton=(opts.automaton[0], [opts.automaton[1][b] for b in seq]))
    if opts.shape is not None and opts.shape["bias"] is not None:
        opts = dataclasses.replace(opts, shape=dict(opts.shape, bias=[opts.shape["bias"][b] for b in seq]))
    if opts.rows is not None:                                             # prompt b's options go to its n samples
        opts = dataclasses.replace(opts, rows=[opts.rows[b] for b in seq])
    state["prefix"] = dict(ktail=torch.empty((L, B * n, nh, N, hd), dtype=kc.dtype, device=dev),
                           vtail=torch.empty((L, B * n, nh, N, hd), dtype=kc.dtype, device=dev),
                           prefix_seq=torch.tensor(seq, dtype=torch.int32, device=dev),
                           prefix_len=torch.tensor([plens[b] for b in seq], dtype=torch.int32, device=dev))
    return generate_loop(decoder, prec, state, first.repeat_interleave(n, dim=0).unsqueeze(1), prompt_tokens.repeat_interleave(n, dim=0),
                         N, opts, pos_shift=pos_shift, lengths=[plens[b] for b in seq], text_lengths=[tlens[b] for b in seq], prompt_rows=T)


MAX_CONTRAST_K = 16                     # kx_contrast_candidates' k limit (kx_step_logprobs' top_n)


def check_contrast_args(vocab: int, *, penalty_alpha=None, output_contrast=False, top_k=0, do_sample=False, num_beams=1,
                        prompt_lookup_num_tokens=0, num_return_sequences=1, return_session=False, guidance_scale=1.0, row_options=None,
                        token_automaton=None, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0, stop_sequences=None,
                        logit_bias=None, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0,
                        eta_cutoff=0.0, repetition_penalty=1.0, temperature=1.0, top_p=1.0, output_logprobs=False, prefill_chunk=None):
    """ValueError (naming ``penalty_alpha``, or ``output_contrast`` without it) for what generate() refuses of contrastive search,
    before the device check and any launch; after check_truncation_args, so every other keyword is already known to be good.
    ``penalty_alpha`` None: off, returns None (no buffer, no launch, no entry point fetched).  A number in [0, 1] (no bool, finite)
    turns contrastive search on and makes ``top_k`` the number of candidates, 1..16 and at most the vocabulary.  It is a
    deterministic mode of its own: together with sampling, beams, prompt lookup, parallel samples, sessions, guidance, row options,
    an automaton, a constraint, a shaping or truncation keyword, a repetition penalty, a temperature, top-p, log-probs or a chunked
    prefill it is refused.  Returns dict(alpha, k, trace)."""
    import math
    if penalty_alpha is None:
        if output_contrast:
            raise ValueError("output_contrast returns the trace of contrastive search: it needs penalty_alpha")
        return None
    a = penalty_alpha
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not math.isfinite(a) or not 0.0 <= a <= 1.0:
        raise ValueError(f"penalty_alpha must be a number in [0, 1] (or None: off), got {a!r}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= MAX_CONTRAST_K:
        raise ValueError(f"penalty_alpha = {a!r} makes top_k the number of candidates per step: it must be an integer in "
                         f"1..{MAX_CONTRAST_K}, got {top_k!r}")
    if top_k > vocab:
        raise ValueError(f"penalty_alpha = {a!r}: top_k = {top_k} candidates exceed the vocabulary of {vocab}")
    why = {
        "do_sample": "contrastive search is deterministic: it chooses among the top_k candidates by score",
        "num_beams": "beams rank whole hypotheses; a contrastive choice per beam is a search of its own",
        "prompt_lookup_num_tokens": "a verify step accepts greedy picks, which contrastive search does not make",
        "num_return_sequences": "the call is deterministic: the copies of one prompt would all be equal",
        "return_session": "a session keeps the plain loop's state; the history of unit vectors is not part of it",
        "guidance_scale": "the candidates would be taken from the guided row but stepped as unguided ones",
        "row_options": "the rows' options are the sampler's",
        "token_automaton": "the candidates are the model's own top_k: a ban would have to be applied before they are taken",
        "no_repeat_ngram_size": "the constraints edit the row the sampler reads, and no sampler runs",
        "bad_words_ids": "the constraints edit the row the sampler reads, and no sampler runs",
        "min_new_tokens": "the constraints edit the row the sampler reads, and no sampler runs",
        "stop_sequences": "the constraints edit the row the sampler reads, and no sampler runs",
        "logit_bias": "the shaping launch edits the row the sampler reads, and no sampler runs",
        "presence_penalty": "the shaping launch edits the row the sampler reads, and no sampler runs",
        "frequency_penalty": "the shaping launch edits the row the sampler reads, and no sampler runs",
        "min_p": "it is a stage of the sampler, and no sampler runs",
        "typical_p": "it is a stage of the sampler, and no sampler runs",
        "epsilon_cutoff": "it is a stage of the sampler, and no sampler runs",
        "eta_cutoff": "it is a stage of the sampler, and no sampler runs",
        "repetition_penalty": "the degeneration penalty is what contrastive search uses against repetition",
        "temperature": "candidate_prob is the model's own probability",
        "top_p": "the candidates are the top_k, nothing else",
        "output_logprobs": "the trace (output_contrast) already holds the candidates' probabilities",
        "prefill_chunk": "the history is filled from the one-piece prefill's residual rows",
    }
    on = dict(do_sample=bool(do_sample), num_beams=num_beams not in (1, None),
              prompt_lookup_num_tokens=prompt_lookup_num_tokens not in (0, None), num_return_sequences=num_return_sequences not in (1, None),
              return_session=bool(return_session), guidance_scale=guidance_scale != 1.0, row_options=row_options is not None,
              token_automaton=token_automaton is not None, no_repeat_ngram_size=no_repeat_ngram_size != 0,
              bad_words_ids=bad_words_ids is not None, min_new_tokens=min_new_tokens != 0, stop_sequences=stop_sequences is not None,
              logit_bias=logit_bias is not None, presence_penalty=presence_penalty != 0.0, frequency_penalty=frequency_penalty != 0.0,
              min_p=min_p != 0.0, typical_p=typical_p != 1.0, epsilon_cutoff=epsilon_cutoff != 0.0, eta_cutoff=eta_cutoff != 0.0,
              repetition_penalty=repetition_penalty != 1.0, temperature=temperature != 1.0, top_p=top_p != 1.0,
              output_logprobs=bool(output_logprobs), prefill_chunk=prefill_chunk is not None)
    for name, bad in on.items():
        if bad:
            raise ValueError(f"penalty_alpha = {a!r} (contrastive search) is not offered together with {name}: {why[name]}; see "
                             "DESIGN.md §8")
    return dict(alpha=float(a), k=top_k, trace=bool(output_contrast))


def contrast_loop(decoder, prec: str, state: dict, logits: torch.Tensor, max_new_tokens: int, opts: LoopOptions, *, pos_shift: int = 0,
                  lengths=None):
    """Contrastive search on a prefilled state (``opts.contrast``: check_contrast_args' dict): ``logits`` [B, T, V] the one-piece
    prefill's output, ``state`` the incremental state it filled with the final residual rows kept (state["residual"], [B, T, D]),
    ``lengths`` the ragged batch's rows per sequence (spliced rows included; None: T for every row), ``pos_shift`` as in generate_loop.
    Sequence b has P_b cache rows, an int32 device word repeated k times ([B * k]: the positions AND the prefix lengths of the step).
    Every buffer is allocated before the first step.  Per token, five launches beside the step:
    kx_contrast_candidates (the k ids and probabilities of the sequence's current logits row — row b * k + chosen[b] of the previous
    step's [B * k, V] logits, addressed, not copied — written as the step's tokens), kx_decoder_decode_step_prefix at M = B * k rows
    (prefix = the sequence's own caches, prefix_seq[r] = r // k, tails [L, M, heads, 1, 64]), kx_contrast_hidden (the M unit hidden
    rows), kx_contrast_select (two launches: the partial maxima over the history, then the choice, which also appends the chosen
    unit vector to the history, writes the token and the trace and sets ``finished`` on the EOS) and kx_kv_cache_commit (the chosen
    tail row into cache row P_b; P_b += 1).  ``output_logits`` adds one indexed copy per token.  The host reads the stop poll (every
    ``eos_poll`` tokens, with an ``eos_token_id``) and, once after the last step, the kernels' sticky error word.
    Returns the tokens int64 [B, n]; then the fp32 [B, n, V] logits with ``output_logits`` — column g the model's own row step g's
    candidates were taken from; then with the trace a dict: candidate_id int64 / candidate_prob / candidate_penalty fp32 [B, n, k],
    chosen int32 [B, n], history fp32 [B, cap, D] (the unit vectors), history_len int32 [B]."""
    c = opts.contrast
    k, alpha, trace = c["k"], c["alpha"], c["trace"]
    eos, pad, N = opts.eos_token_id, int(opts.pad_token_id), int(max_new_tokens)
    B, T, V = logits.shape
    dev = logits.device
    M = B * k
    plens = [T] * B if lengths is None else list(lengths)
    kc, vc = state["kcache"], state["vcache"]
    L, _, nh, cap, hd = kc.shape
    D = nh * hd
    w = decoder._pack(state["prec"])[0]
    resid = state.pop("residual")
    state.pop("keep_residual", None)
    # every buffer before the first step
    lens_dev = torch.tensor(plens, dtype=torch.int32, device=dev)
    history = torch.zeros((B, cap, D), dtype=torch.float32, device=dev)
    ops.contrast_hidden(w, resid, history, lengths=lens_dev)
    del resid
    hist_len = lens_dev.clone()
    positions = lens_dev.repeat_interleave(k).contiguous()                # P_b, k times: the step's positions and prefix lengths
    seq = torch.arange(M, dtype=torch.int32, device=dev) // k
    state.update(positions=positions, pos_max=max(plens))
    state["prefix"] = dict(ktail=torch.empty((L, M, nh, 1, hd), dtype=kc.dtype, device=dev),
                           vtail=torch.empty((L, M, nh, 1, hd), dtype=kc.dtype, device=dev), prefix_seq=seq.to(torch.int32), prefix_len=positions)
    decoder._ragged_scratch(state, dev, rows=M)
    err = state["error"]
    out = torch.full((B, N), pad, dtype=torch.int64, device=dev)
    step_tokens = torch.zeros(M, dtype=torch.int64, device=dev)
    prob = torch.zeros(M, dtype=torch.float32, device=dev)
    u = torch.empty((M, D), dtype=torch.float32, device=dev)
    nxt = torch.full((B,), pad, dtype=torch.int64, device=dev)
    chosen = torch.zeros(B, dtype=torch.int32, device=dev)
    finished = torch.zeros(B, dtype=torch.uint8, device=dev)
    scratch = ops.contrast_scratch(B, k, cap, dev)
    step_logits = torch.empty((M, V), dtype=torch.float32, device=dev)
    cand_id = cand_prob = cand_pen = chosen_tr = None
    if trace:
        cand_id = torch.full((B, N, k), -1, dtype=torch.int64, device=dev)
        cand_prob = torch.zeros((B, N, k), dtype=torch.float32, device=dev)
        cand_pen = torch.zeros((B, N, k), dtype=torch.float32, device=dev)
        chosen_tr = torch.full((B, N), -1, dtype=torch.int32, device=dev)
    kept = torch.empty((B, N, V), dtype=torch.float32, device=dev) if opts.output_logits else None
    rows_b = torch.arange(B, device=dev) * k
    first = logits[torch.arange(B, device=dev), lens_dev.long() - 1] if lengths is not None else logits[:, -1]     # [B, V]
    n = 0
    for g in range(N):
        if g == 0:
            if kept is not None:
                kept[:, 0] = first
            ops.contrast_candidates(first, k=k, step_tokens=step_tokens, prob=prob, finished=finished, cand_id=cand_id,
                                    cand_prob=cand_prob, col=0)
        else:
            if kept is not None:
                kept[:, g] = step_logits[rows_b + chosen.long()]
            ops.contrast_candidates(step_logits, k=k, step_tokens=step_tokens, prob=prob, chosen=chosen, k_prev=k, finished=finished,
                                    cand_id=cand_id, cand_prob=cand_prob, col=g)
        decoder._forward_incremental(None, state, None, prec, next_token=step_tokens, pos_shift=pos_shift, logits_out=step_logits)
        ops.contrast_hidden(w, state["x_step"], u, workspace=state["step_ws"], prec=state["step_pid"])
        ops.contrast_select(u, prob, history, hist_rows=positions, p_stride=k, hist_len=hist_len, alpha=alpha, step_tokens=step_tokens,
                            finished=finished, next_token=nxt, chosen=chosen, scratch=scratch, error_word=err, eos_token_id=eos,
                            pad_token_id=pad, out_tokens=out, cand_penalty=cand_pen, chosen_trace=chosen_tr, col=g)
        ops.kv_cache_commit(state["prefix"]["ktail"], state["prefix"]["vtail"], kc, vc, chosen, positions, err, finished=finished)
        n = g + 1
        if n == N:
            break
        if eos is not None and opts.eos_poll > 0 and n % opts.eos_poll == 0:
            done, word = torch.stack([finished.min().to(torch.int32), err[0]]).tolist()      # the loop's only device-to-host read
            _raise_position_error(word, state)
            if done:
                break
    _raise_position_error(int(err.item()), state)
    res = [out[:, :n]]
    if kept is not None:
        res.append(kept[:, :n])
    if trace:
        res.append(dict(candidate_id=cand_id[:, :n], candidate_prob=cand_prob[:, :n], candidate_penalty=cand_pen[:, :n],
                        chosen=chosen_tr[:, :n], history=history, history_len=hist_len))
    return res[0] if len(res) == 1 else tuple(res)


MAX_STEP_ROWS = 16                      # the weight-streaming step's rows: B * (D + 1) of a lookup step


def check_lookup_args(batch: int, *, prompt_lookup_num_tokens=0, max_matching_ngram_size=2, output_acceptance=False, draft_from=None,
                      do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, num_beams=1,
                      prompt_lengths=None, sequence_ids=None, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0,
                      stop_sequences=None, eos_poll=8) -> int:
    """ValueError (naming the argument) for what generate() refuses of prompt-lookup speculation, before anything is launched.
    Returns D, the number of drafts per step (0: the call runs the loops it always ran)."""
    D = prompt_lookup_num_tokens
    if isinstance(D, bool) or not isinstance(D, int) or D < 0:
        raise ValueError(f"prompt_lookup_num_tokens must be a non-negative integer, got {D!r}")
    if D == 0:
        if output_acceptance:
            raise ValueError("output_acceptance is an output of prompt-lookup speculation: it needs prompt_lookup_num_tokens > 0")
        if draft_from is not None:
            raise ValueError("_draft_from needs prompt_lookup_num_tokens > 0")
        return 0
    n = max_matching_ngram_size
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_NGRAM:
        raise ValueError(f"max_matching_ngram_size must be an integer in 1..{MAX_NGRAM}, got {n!r}")
    for name, bad in (("do_sample", bool(do_sample)), ("temperature", float(temperature) != 1.0), ("top_k", int(top_k) != 0),
                      ("top_p", float(top_p) != 1.0), ("repetition_penalty", float(repetition_penalty) != 1.0),
                      ("num_beams", num_beams != 1), ("prompt_lengths", prompt_lengths is not None),
                      ("sequence_ids", sequence_ids is not None), ("no_repeat_ngram_size", no_repeat_ngram_size != 0),
                      ("bad_words_ids", bool(bad_words_ids)), ("min_new_tokens", min_new_tokens != 0),
                      ("stop_sequences", bool(stop_sequences))):
        if bad:
            raise ValueError(f"{name} is not offered together with prompt-lookup speculation (prompt_lookup_num_tokens = {D}): it is "
                             "exact for plain greedy decoding only; see DESIGN.md §7b")
    if batch * (D + 1) > MAX_STEP_ROWS:
        raise ValueError(f"prompt_lookup_num_tokens = {D}: {batch} sequences x {D + 1} rows exceed the {MAX_STEP_ROWS} rows of a "
                         "weight-streaming step (the drafts would cost a tile GEMM)")
    if isinstance(eos_poll, bool) or not isinstance(eos_poll, int) or eos_poll <= 0:
        raise ValueError(f"eos_poll must be a positive integer with prompt_lookup_num_tokens = {D} (the poll is how the loop ends), "
                         f"got {eos_poll!r}")
    return D


def lookup_loop(decoder, prec: str, state: dict, logits: torch.Tensor, prompt_tokens: torch.Tensor, max_new_tokens: int, *,
                num_drafts: int, ngram_max: int = 2, pos_shift: int = 0, eos_token_id=None, pad_token_id=1, eos_poll=8,
                output_logits=False, output_acceptance=False, draft_from=None, prompt_rows=None):
    """Greedy decoding with prompt-lookup speculation after the prefill: ``logits`` [B, T, V] and ``state`` as for generate_loop
    (``prompt_rows`` as there: ``logits`` [B, 1, V] holds the last position alone)
    (state["max_len"] >= T + max_new_tokens + num_drafts), ``prompt_tokens`` [B, Tt] int64 the ids the lookup starts from (the
    TEXT ids: spliced image rows contribute none).  Per verify step g: kx_sample_logits (greedy) on the step's [B * Kin, V] block
    (Kin = 1: the prefill's last row; K = num_drafts + 1 afterwards), kx_spec_accept (the contract: include/kosmosx_hip.h,
    "Speculative decoding by prompt lookup"), then kx_decoder_decode_step_block on the B * K rows it wrote.  Every buffer is
    allocated before the first step; the host reads ``finished.all()`` with the step kernels' error word at the poll and once
    after the loop (there with the longest row's length), nothing else.  At most max_new_tokens steps: an unfinished row emits
    at least one token per step.  ``draft_from`` int64 [B, max_new_tokens] (tests, benchmark): the draft for output slot i is
    draft_from[b, i] instead of the lookup's.
    Returns tokens int64 [B, n]; then with ``output_logits`` the fp32 [B, n, V] rows the tokens were picked from (zeros after a
    row's end); then with ``output_acceptance`` the int32 [B, steps] tokens emitted per step, for the steps in which some row still
    emitted (the steps issued after the last row finished and before the poll noticed are not listed)."""
    B, T, V = logits.shape
    if prompt_rows is not None:
        T = prompt_rows
    dev = logits.device
    D, N = int(num_drafts), int(max_new_tokens)
    K = D + 1
    M = B * K
    pad = int(pad_token_id)
    Tt = prompt_tokens.shape[1]
    if draft_from is not None:
        if not isinstance(draft_from, torch.Tensor) or draft_from.dtype != torch.int64 or tuple(draft_from.shape) != (B, N):
            raise ValueError(f"_draft_from must be an int64 [{B}, {N}] tensor")
        draft_from = draft_from.to(dev).contiguous()
    out = torch.full((B, N), pad, dtype=torch.int64, device=dev)
    n_out = torch.zeros(B, dtype=torch.int32, device=dev)
    history = torch.empty((B, Tt + N), dtype=torch.int64, device=dev)
    history[:, :Tt] = prompt_tokens
    hist_len = torch.full((B,), Tt, dtype=torch.int32, device=dev)
    finished = torch.zeros(B, dtype=torch.uint8, device=dev)
    positions = torch.zeros(M, dtype=torch.int32, device=dev)              # kx_spec_accept initialises them at step 0
    picked = torch.empty(M, dtype=torch.int64, device=dev)
    cur, nxt = (torch.empty(M, dtype=torch.int64, device=dev) for _ in range(2))   # the block a step was fed / the next one
    emitted = torch.zeros((B, N), dtype=torch.int32, device=dev)
    kept = out_src = None
    if output_logits:
        kept = torch.zeros((N, M, V), dtype=torch.float32, device=dev)       # row [g, b * K + j]: step g's logits
        out_src = torch.zeros((B, N), dtype=torch.int32, device=dev)
    else:
        block_buf = torch.empty((M, V), dtype=torch.float32, device=dev)
    # the furthest row any step can touch, for the host-side table / cache check of the step (the budget covers it)
    state.update(positions=positions, block=K, pos_max=T + N + D - 1)
    decoder._ragged_scratch(state, dev, rows=M)                             # (before the first launch: no fill between steps)
    err = state["error"]
    block = logits[:, -1]                                                   # [B, V] view, row stride T * V
    if kept is not None:
        kept[0].view(B, K, V)[:, 0].copy_(block)
    steps = 0
    for g in range(N):
        Kin = 1 if g == 0 else K
        ops.sample_logits(block, do_sample=False, pad_token_id=pad, out=picked[:B * Kin])
        ops.spec_accept(picked[:B * Kin], fed=cur if g else None, rows_per_sequence=K, positions=positions, prefill_len=T,
                        history=history, hist_len=hist_len, out_tokens=out, n_out=n_out, finished=finished, next_tokens=nxt,
                        max_new_tokens=N, step=g, ngram_max=ngram_max, eos_token_id=eos_token_id, pad_token_id=pad,
                        out_src=out_src, emitted=emitted, draft_from=draft_from)
        steps = g + 1
        if steps == N:
            break
        if steps % eos_poll == 0:                                           # the loop's only device-to-host read
            done, word = torch.stack([finished.min().to(torch.int32), err[0]]).tolist()
            _raise_position_error(word, state)
            if done:
                break
        block = decoder._forward_incremental(None, state, None, prec, next_token=nxt, pos_shift=pos_shift,
                                             logits_out=kept[g + 1] if kept is not None else block_buf)[:, 0]
        cur, nxt = nxt, cur
    # (the steps that emitted something are a prefix of the steps issued: the poll's granularity does not show in the outputs)
    done, word, n, used = torch.stack([finished.min().to(torch.int32), err[0], n_out.max(),
                                       (emitted.max(0).values > 0).sum().to(torch.int32)]).tolist()
    _raise_position_error(word, state)
    if not done:                                                            # cannot happen: max_new_tokens steps finish every row
        raise RuntimeError("prompt-lookup speculation ended with an unfinished row")
    res = [out[:, :n]]
    if output_logits:
        flat = kept[:steps].view(steps * M, V)
        src = out_src[:, :n].to(torch.int64)
        idx = (src // K) * M + torch.arange(B, device=dev)[:, None] * K + src % K
        live = torch.arange(n, device=dev)[None, :] < n_out[:, None]
        res.append(torch.where(live[:, :, None], flat[idx], torch.zeros((), dtype=torch.float32, device=dev)))
    if output_acceptance:
        res.append(emitted[:, :used])
    return res[0] if len(res) == 1 else tuple(res)


MAX_SCORE_LEN = 16                      # kx_decoder_score_step's K rows per candidate: a continuation feeds L - 1 <= 16 of them


def check_score_args(batch: int, continuations, continuation_lengths=None, prompt_index=None):
    """ValueError (naming the argument) for what score() refuses, before the device check and any launch.  Returns the host lists
    (continuation lengths [C], prompt of every candidate [C])."""
    if not isinstance(continuations, torch.Tensor) or continuations.dtype != torch.int64 or continuations.dim() != 2:
        what = (f"a {continuations.dtype} tensor of shape {tuple(continuations.shape)}" if isinstance(continuations, torch.Tensor)
                else repr(type(continuations)))
        raise ValueError(f"continuations must be an int64 [candidates, length] tensor, got {what}")
    C, L = continuations.shape
    if not 1 <= L <= MAX_SCORE_LEN:
        raise ValueError(f"continuations holds {L} tokens per candidate: 1..{MAX_SCORE_LEN} are offered, the limit of the K-row decode "
                         "step that scores them in one pass over the weights")
    if C < 1:
        raise ValueError("continuations holds no candidate")
    if continuation_lengths is None:
        lens = [L] * C
    else:
        lens = _host_ints(continuation_lengths, C, "continuation_lengths", "candidate", joint=True)
        for c, l in enumerate(lens):
            if not 1 <= l <= L:
                raise ValueError(f"continuation_lengths[{c}] = {l} is outside 1..{L}")
    if prompt_index is None:
        if batch < 1 or C % batch:
            raise ValueError(f"continuations holds {C} candidates for {batch} prompts: without a prompt_index the candidates are "
                             "split evenly, so their number must be a multiple of the prompts'")
        pidx = [c // (C // batch) for c in range(C)]
    else:
        if isinstance(prompt_index, torch.Tensor):
            raise ValueError("prompt_index must be host integers (a list), not a tensor: the cache map is built on the host")
        try:
            pidx = [operator.index(b) for b in prompt_index]
        except TypeError:
            raise ValueError(f"prompt_index must be a sequence of {C} integers, got {prompt_index!r}") from None
        if len(pidx) != C:
            raise ValueError(f"prompt_index must have {C} entries (one per candidate), got {len(pidx)}")
        for c, b in enumerate(pidx):
            if not 0 <= b < batch:
                raise ValueError(f"prompt_index[{c}] = {b} is outside the {batch} prompts")
    return lens, pidx


def score_loop(decoder, prec: str, state: dict, logits: torch.Tensor, continuations: torch.Tensor, clens: list, pidx: list,
               plens: list, *, pos_shift: int = 0, output_logits=False, prompt_rows=None):
    """The log-probs of C candidates after the prefill: ``logits`` [B, T, V] and ``state`` as for generate_loop (state["max_len"] >=
    T + L - 1; ``prompt_rows`` as there: ``logits`` [B, 1, V] holds row len_b - 1 of every prompt alone), ``continuations`` int64 [C, L] on the device, ``clens`` / ``pidx`` the host lists check_score_args returned and
    ``plens`` [B] the prompts' positions (spliced rows included).  Column 0: kx_token_logprob on the prefill's rows, addressed
    through a row index (row len_b - 1 of the candidate's prompt; no [C, V] copy).  Columns 1..L-1: ONE kx_decoder_score_step with
    M = C * (L - 1) rows — candidate c's row j is fed continuations[c, j] at position len_b + j, its last token is never fed — and one
    kx_token_logprob on its rows.  L = 1 launches no step.  The positions [M] and the candidate -> cache sequence map [C] are built
    on the host and uploaded once; the host reads the deferred id check and the step kernels' error word at the end, nothing else.
    Returns token_logprobs fp32 [C, L] (0.0 at padded slots), and with ``output_logits`` the fp32 [C, L, V] rows."""
    from .model import _begin_token_id_check
    B, T, V = logits.shape
    dev = logits.device
    C, L = continuations.shape
    K = L - 1
    col = torch.arange(L, device=dev)[None, :]
    live = col < torch.tensor(clens, dtype=torch.int64, device=dev)[:, None]                     # [C, L]
    # padding -> the candidate's own first id: whatever it held is never range-checked or embedded (as mask_padding)
    tokens = torch.where(live, continuations, continuations[:, :1]).contiguous()
    check = None
    if getattr(decoder, "validate_token_ids", True):
        check = _begin_token_id_check(tokens, decoder.embed_tokens.weight.shape[0])              # finished after the launches
    target = torch.where(live, tokens, torch.full((), -1, dtype=torch.int64, device=dev))       # -1: kx_token_logprob leaves 0.0
    if prompt_rows is not None:                                                                  # one row per prompt: its own
        rows0 = torch.tensor(pidx, dtype=torch.int32, device=dev)
    else:
        rows0 = torch.tensor([pidx[c] * T + plens[pidx[c]] - 1 for c in range(C)], dtype=torch.int32, device=dev)
    flat = logits.view(B * T, V)
    out = torch.empty((C, L), dtype=torch.float32, device=dev)
    lp0 = ops.token_logprob(flat, target[:, 0].contiguous(), row_index=rows0)
    out[:, 0] = lp0
    kept = None
    if output_logits:
        kept = torch.zeros((C, L, V), dtype=torch.float32, device=dev)
        kept[:, 0] = flat[rows0.long()]
    if K > 0:
        M = C * K
        positions = torch.tensor([plens[pidx[c]] + j for c in range(C) for j in range(K)], dtype=torch.int32, device=dev)
        cache_seq = torch.tensor(pidx, dtype=torch.int32, device=dev)
        # the furthest position fed, for the host-side table / cache check of the step (the budget covers it)
        state.update(positions=positions, score=(K, cache_seq), pos_max=max(plens[b] for b in pidx) + K - 1)
        decoder._ragged_scratch(state, dev, rows=M)
        fed = tokens[:, :K].reshape(M).contiguous()                                              # (K = 1: reshape alone is a strided view)
        step = decoder._forward_incremental(None, state, None, prec, next_token=fed, pos_shift=pos_shift)[:, 0]   # [M, V]
        out[:, 1:] = ops.token_logprob(step, target[:, 1:].reshape(M).contiguous()).view(C, K)
        if kept is not None:
            kept[:, 1:] = torch.where(live[:, 1:, None], step.view(C, K, V), torch.zeros((), dtype=torch.float32, device=dev))
    if check is not None:
        check()                                                                                  # IndexError: an id outside the vocabulary
    if K > 0:
        _raise_position_error(int(state["error"].item()), state)
    if kept is not None:
        return out, kept
    return out


def check_prefill_chunk(prefill_chunk):
    """ValueError for a ``prefill_chunk`` that is not None or a positive int (bool excluded); host only."""
    if prefill_chunk is None:
        return None
    if isinstance(prefill_chunk, bool) or not isinstance(prefill_chunk, int) or prefill_chunk < 1:
        raise ValueError(f"prefill_chunk must be a positive integer (the rows prefilled per pass) or None, got {prefill_chunk!r}")
    return prefill_chunk


def _prefill(model, prompt: dict, prompt_lengths, new_rows: int, spare: int = 0, budget: bool = True, chunk=None, capacity=None,
             keep_residual: bool = False):
    """The prompt's prefill, under torch.no_grad(): ``prompt`` as run_generate takes it, ``new_rows`` (+ ``spare``) the positions the
    caller will add, checked against the tables when ``budget``.  Returns the tokens as prefilled (trimmed to the longest prompt, the
    padding masked), the host lengths (None: a uniform batch), T (prefix rows included), the state, the prefill's logits and the
    loops' ``prompt_rows``: None with the [B, T, V] logits of the one-piece prefill.
    ``chunk`` C < T (check_prefill_chunk): the rows are embedded once and prefilled C at a time — rows [0, C) by the prefill call,
    with the XPos centring of the whole T (state["xpos_centre"]), every later slice by Decoder._extend — the first slice always
    writes its C logits rows, a later one only if it holds a row the loops read, last position or len_b - 1; those rows are
    returned as [B, 1, V] with ``prompt_rows`` = T.
    ``capacity`` (sessions): the cache rows per sequence instead of T + ``new_rows``; the budget is checked against it too.
    ``keep_residual`` (contrastive search; one-piece prefill only): the prefill's final residual rows stay in state["residual"]."""
    tokens, lens = prompt["tokens"], None
    if prompt_lengths is not None:
        lens = resolve_prompt_lengths(prompt_lengths, tokens.shape[0], tokens.shape[1], min_len=prompt["min_len"])
        tokens = tokens[:, :max(lens)]                                      # columns no row uses
    T = tokens.shape[1] + prompt["prefix_rows"]
    if budget:
        check_budget(model.decoder, T, new_rows, spare=spare, rows=capacity)
    if lens is not None:
        tokens = mask_padding(tokens.long(), lens)
    # Ragged prompts go through the ordinary prefill, right-padded, with no padding mask and no new kernel: attention is
    # causal, so a real position (< len_b) never has a padded key (>= len_b) among the keys it sees, and every other
    # operation of the decoder works on a row alone.  The padded rows compute finite values (their ids are the row's first
    # token, mask_padding) that nobody uses: the first token is drawn from logits[b, len_b - 1], and cache row
    # len_b + g of sequence b is overwritten by the row's own g-th generated token in the very launch whose query is the
    # first that could see it (kx_attention_decode_ragged appends row positions[b] and reads that key from the qkv row);
    # a score() candidate reads cache rows < len_b only.
    passed_x = prompt["passed_x"](tokens)                                   # (the prompt's ids are range-checked here or in the prefill, once)
    state = {"max_len": T + new_rows + spare if capacity is None else capacity}   # (rejected drafts still occupy table and cache rows)
    if keep_residual:
        state["keep_residual"] = True
    if chunk is None or chunk >= T:
        logits = model.decoder._forward_incremental(tokens if passed_x is None else None, state, passed_x, model.precision)
        return tokens, lens, T, state, logits, None
    decoder = model.decoder
    x = decoder.embed(tokens, model.precision) if passed_x is None else passed_x               # [B, T, D], embedded once
    B = x.shape[0]
    last = [T - 1] * B if lens is None else [prompt["prefix_rows"] + l - 1 for l in lens]      # the row every sequence reads
    rows = None
    state["xpos_centre"] = T
    for s0 in range(0, T, chunk):
        s1 = min(s0 + chunk, T)
        want = [b for b in range(B) if s0 <= last[b] < s1]
        if s0 == 0:
            logits = decoder._forward_incremental(None, state, x[:, :s1], model.precision)
        else:
            logits = decoder._extend(x[:, s0:s1], state, model.precision, output_logits=bool(want))
        if want:
            if rows is None:
                rows = torch.empty((B, 1, logits.shape[2]), dtype=torch.float32, device=logits.device)
            idx = torch.tensor(want, dtype=torch.int64, device=logits.device)
            rows[idx, 0] = logits[idx, torch.tensor([last[b] - s0 for b in want], dtype=torch.int64, device=logits.device)]
    return tokens, lens, T, state, rows, T


def run_generate(model, prompt: dict, max_new_tokens: int, kw: dict):
    """What Kosmos.generate and KosmosLanguage.generate share, ``kw`` being their keyword arguments by name.  ``prompt`` describes
    the model's prompt: ``tokens`` (the [B, Tt] ids), ``check`` (a callable: the model's device and shape checks, run after the
    argument checks), ``passed_x`` (a callable: the tokens as prefilled -> the [B, T, D] rows the prefill takes, or None for the
    tokens alone), ``min_len`` (the shortest ragged prompt), ``prefix_rows`` (the rows passed_x adds to the tokens') and
    ``pos_shift`` (as in generate_loop)."""
    decoder, prec, vocab, tokens = model.decoder, model.precision, model.embed.weight.shape[0], prompt["tokens"]
    batch = tokens.shape[0] if tokens.dim() else 0
    # every check once, in this order (the first refusal is the one a caller sees), each with the keywords its signature names
    guide = check_guidance_args(batch, min_len=prompt["min_len"], multimodal="negative_images" in kw, **_own(check_guidance_args, kw))
    beams = check_beam_args(vocab, beam_path=kw["_beam_path"], **_own(check_beam_args, kw))
    samples = check_parallel_args(beams=beams, **_own(check_parallel_args, kw))
    cons = check_constraint_args(vocab, **dict(_own(check_constraint_args, kw), num_beams=kw["num_beams"] if beams else None))
    drafts = check_lookup_args(batch, draft_from=kw["_draft_from"], **_own(check_lookup_args, kw))
    check_logprob_args(vocab, beams=beams, drafts=drafts, **_own(check_logprob_args, kw))
    starts = check_automaton_args(vocab, batch, **_own(check_automaton_args, kw))
    shape = check_shape_args(vocab, batch, **_own(check_shape_args, kw))
    truncation = check_truncation_args(**_own(check_truncation_args, kw))
    contrast = check_contrast_args(vocab, **_own(check_contrast_args, kw))
    rows = check_row_options(vocab, batch, max_new_tokens=max_new_tokens, **_own(check_row_options, kw))
    chunk = check_prefill_chunk(kw["prefill_chunk"])
    capacity = check_session_args(decoder, beams=beams, drafts=drafts, **_own(check_session_args, kw))
    prompt["check"](**({} if guide is None or kw["negative_prompt_ids"] is None else dict(negative_prompt_ids=kw["negative_prompt_ids"])))
    opts = LoopOptions.resolved(kw, cons, starts, shape, truncation, guide, rows, contrast)   # what the plain-loop paths below take
    with torch.no_grad():
        if contrast is not None:                                          # (everything below but ragged prompts was refused with it)
            tokens, lens, T, state, logits, _ = _prefill(model, prompt, kw["prompt_lengths"], max_new_tokens, keep_residual=True)
            return contrast_loop(decoder, prec, state, logits, max_new_tokens, opts, pos_shift=prompt["pos_shift"],
                                 lengths=None if lens is None else [prompt["prefix_rows"] + l for l in lens])
        if guide is not None:
            # every sequence as two rows of one ragged batch: the prompt (rows 0..B-1) and its negative (rows B..2B-1), prefilled
            # through _prefill unchanged; generate_loop gives the sampler the first B rows and feeds both halves the same token
            prompt, lengths2 = _guided_prompt(prompt, kw["prompt_lengths"], guide, **_own(_guided_prompt, kw))
            tokens, lens, _, state, logits, prompt_rows = _prefill(model, prompt, lengths2, max_new_tokens, chunk=chunk)
            return generate_loop(decoder, prec, state, logits, tokens.long(), max_new_tokens, opts, pos_shift=prompt["pos_shift"],
                                 prompt_rows=prompt_rows, lengths=[prompt["prefix_rows"] + l for l in lens], text_lengths=lens)
        tokens, lens, _, state, logits, prompt_rows = _prefill(model, prompt, kw["prompt_lengths"], max_new_tokens, spare=drafts,
                                                               chunk=chunk, capacity=capacity)
        if capacity is not None:
            return _first_turn(model, prompt, state, logits, tokens.long(), lens, prompt_rows, max_new_tokens, capacity, opts)
        common = dict(pos_shift=prompt["pos_shift"], prompt_rows=prompt_rows)
        if drafts:
            return lookup_loop(decoder, prec, state, logits, tokens.long(), max_new_tokens, num_drafts=drafts,
                               ngram_max=kw["max_matching_ngram_size"], draft_from=kw["_draft_from"], **common, **_own(lookup_loop, kw))
        if beams:
            return beam_loop(decoder, prec, state, logits, max_new_tokens, **common, **_own(beam_loop, kw))
        common.update(lengths=None if lens is None else [prompt["prefix_rows"] + l for l in lens], text_lengths=lens)
        if samples > 1:
            return parallel_loop(decoder, prec, state, logits, tokens.long(), max_new_tokens, opts, num_return_sequences=samples, **common)
        return generate_loop(decoder, prec, state, logits, tokens.long(), max_new_tokens, opts, **common)


def run_score(model, prompt: dict, continuations, kw: dict):
    """What Kosmos.score and KosmosLanguage.score share: ``prompt`` as in run_generate, ``kw`` their keyword arguments by name."""
    tokens = prompt["tokens"]
    B = tokens.shape[0] if tokens.dim() else 0
    clens, pidx = check_score_args(B, continuations, kw["continuation_lengths"], kw["prompt_index"])
    chunk = check_prefill_chunk(kw["prefill_chunk"])
    prompt["check"](continuations=continuations)
    L = continuations.shape[1]
    with torch.no_grad():
        _, lens, T, state, logits, prompt_rows = _prefill(model, prompt, kw["prompt_lengths"], L - 1, budget=L > 1, chunk=chunk)
        return score_loop(model.decoder, model.precision, state, logits, continuations, clens, pidx,
                          [T] * B if lens is None else [prompt["prefix_rows"] + l for l in lens], pos_shift=prompt["pos_shift"],
                          output_logits=kw["output_logits"], prompt_rows=prompt_rows)


def check_budget(decoder, T: int, max_new_tokens: int, spare: int = 0, rows=None):
    """IndexError before any launch when prompt + new tokens (+ ``spare`` rows: the drafts of a lookup step) overrun the position
    table / cache (``rows``: a session's cache rows, at most the table's)."""
    if not isinstance(max_new_tokens, int) or max_new_tokens < 1:
        raise ValueError(f"max_new_tokens must be a positive integer, got {max_new_tokens!r}")
    if rows is None:
        rows = decoder.embed_positions.weight.shape[0] - 2
    # (conservative by one token: the last generated token is never embedded, so it would not need a row of its own)
    if T + max_new_tokens + spare > rows:
        raise IndexError(f"index out of range in self: {T} prompt positions + {max_new_tokens} new tokens"
                         + (f" + {spare} draft rows" if spare else "") + f" exceed the {rows}-row position table / cache")


def _raise_position_error(word: int, state: dict):
    """The sticky word of the ragged step kernels (kx_ragged_error): a row's device position left the table / the cache."""
    if word:
        what = " and ".join(name for bit, name in ((H.KX_RAGGED_ERR_TABLE, "the position / XPos tables"),
                                                   (H.KX_RAGGED_ERR_CACHE, "the KV cache"),
                                                   (H.KX_RAGGED_ERR_COMMIT, "the rows a cache commit may write")) if word & bit)
        raise IndexError(f"index out of range in self: a row's device position left {what} (host-side maximum "
                         f"{state.get('pos_max')}, cache of {state.get('max_len')} rows); that row's step wrote nothing")


def resolve_prompt_lengths(prompt_lengths, B: int, width: int, min_len: int = 1, name: str = "prompt_lengths") -> list:
    """``prompt_lengths`` (a sequence of B ints or an integer tensor) -> a host list of B ints in [min_len, width], or
    ValueError naming ``name``.  Host data is taken as it is; a device tensor is read back once."""
    lens = _host_ints(prompt_lengths, B, name, "row")
    for b, l in enumerate(lens):
        if l < min_len:
            raise ValueError(f"{name}[{b}] = {l}: a prompt has at least {min_len} token" + ("s" if min_len > 1 else "")
                             + (" (the image is spliced after two text tokens)" if min_len == 2 else ""))
        if l > width:
            raise ValueError(f"{name}[{b}] = {l} exceeds the padded width {width}")
    return lens


def mask_padding(tokens: torch.Tensor, lengths: list) -> torch.Tensor:
    """``tokens`` [B, T] int64 with the columns at and after lengths[b] replaced by the row's own first token: whatever the
    padding held is never embedded or range-checked, and the repetition penalty's history sees no id the prompt lacks."""
    T = tokens.shape[1]
    lens = torch.tensor(lengths, dtype=torch.int64, device=tokens.device)
    return torch.where(torch.arange(T, device=tokens.device)[None, :] < lens[:, None], tokens, tokens[:, :1])


# ---- sessions: generate() that keeps its KV cache and takes further turns ----

def check_session_args(decoder, *, return_session=False, session_capacity=None, num_beams=1, prompt_lookup_num_tokens=0, beams=False,
                       drafts=0):
    """ValueError (naming the argument) for what generate() refuses of the session arguments, before the device check and any
    launch.  Returns the cache rows per sequence of the session, or None when none was asked for."""
    if not return_session:
        if session_capacity is not None:
            raise ValueError("session_capacity is the cache size of a session: it needs return_session=True")
        return None
    if beams:
        raise ValueError(f"return_session is not offered together with beam search (num_beams = {num_beams}): its caches are gathered "
                         "per beam, no row of them is one conversation; see DESIGN.md §8")
    if drafts:
        raise ValueError(f"return_session is not offered together with prompt-lookup speculation (prompt_lookup_num_tokens = "
                         f"{prompt_lookup_num_tokens}): its caches hold draft rows; see DESIGN.md §8")
    rows = decoder.embed_positions.weight.shape[0] - 2
    if session_capacity is None:
        return rows
    if isinstance(session_capacity, bool) or not isinstance(session_capacity, int) or session_capacity < 1:
        raise ValueError(f"session_capacity must be a positive integer (cache rows per sequence) or None, got {session_capacity!r}")
    if session_capacity > rows:
        raise ValueError(f"session_capacity = {session_capacity} exceeds the {rows}-row position table")
    return session_capacity


def session_after_turn(cached: list, block_lens: list, n_valid: list):
    """A turn's bookkeeping, host lists in and out.  Row b's cache held cached[b] valid rows, the turn appended its block of
    block_lens[b] rows (a pending token and the new ids) and generated n_valid[b] valid tokens, of which all but the last were fed
    back.  Returns (logical lengths, valid cache rows, index of the pending token among the row's generated ones or -1): the last
    valid token was sampled but never fed — or fed at the very row the next turn rewrites — so it is pending and its row is not
    counted as cached."""
    lengths = [c + bl + nv for c, bl, nv in zip(cached, block_lens, n_valid)]
    rows = [c + bl + max(nv - 1, 0) for c, bl, nv in zip(cached, block_lens, n_valid)]
    return lengths, rows, [nv - 1 for nv in n_valid]


def _loop_turn(session, rows, history, hist_lens, starts, max_new_tokens, opts):
    """generate_loop on a session's state: ``rows`` [B, 1, V] the logits every sequence draws its first token from, ``history``
    [B, W] the conversation's text ids (mask_padding-ed), ``hist_lens`` their lengths, ``starts`` the positions the first new
    tokens take = the valid cache rows.  Returns (what generate_loop returns, n_valid per row)."""
    dev = rows.device
    pads = torch.zeros(len(starts), dtype=torch.int32, device=dev)
    res = generate_loop(session._decoder, session._model.precision, session._state, rows, history, max_new_tokens, opts,
                        pos_shift=session._pos_shift, lengths=list(starts), text_lengths=list(hist_lens), prompt_rows=max(starts),
                        pad_launches=pads)
    n, padded = session._state.pop("turn")
    return res, [n - p for p in padded]


def _first_turn(model, prompt, state, logits, tokens, lens, prompt_rows, max_new_tokens, capacity, opts):
    """The generate() call that opens a session: the plain ragged loop on the prefilled state (a uniform batch as a ragged one of
    equal lengths: the same Philox positions, the same bits), then the Session around what it left."""
    B, Tt = tokens.shape
    text_lens = [Tt] * B if lens is None else list(lens)
    starts = [prompt["prefix_rows"] + l for l in text_lens]
    if prompt_rows is None:                                               # the row every sequence reads, as a chunked prefill returns it
        idx = torch.tensor([s - 1 for s in starts], dtype=torch.int64, device=logits.device)
        logits = logits[torch.arange(B, device=logits.device), idx][:, None]
    session = Session(model, state, capacity, prompt["pos_shift"], prompt["prefix_rows"])
    res, n_valid = _loop_turn(session, logits, tokens, text_lens, starts, max_new_tokens, opts)
    out = res[0] if isinstance(res, tuple) else res
    session._advance([tokens[b, :l] for b, l in enumerate(text_lens)], starts, [0] * B, out, n_valid)
    return (*res, session) if isinstance(res, tuple) else (res, session)


class Session:
    """A batch of conversations whose KV cache outlives generate(): ``generate(..., return_session=True)`` returns one after its
    usual outputs.  After any number of turns row b behaves like a fresh ragged generate() whose prompt is the row's whole logical
    sequence so far — its first prompt (spliced image rows included), every turn's valid output and every appended turn — with the
    XPos tables centred on the first call's T (rounding only).  Later turns are text only.

    ``lengths``: host list, every row's logical length in positions.  ``capacity``: the cache rows per sequence.
    A row's last valid token of a turn was sampled but never fed: it is pending, and the next turn's block for the row is that
    token followed by the new ids, right-padded to the widest block (padding ids as mask_padding), appended at the row's own
    position by one ragged extend (Decoder._extend_ragged).  Cache rows at or after a row's valid length hold leftovers from pad
    steps and padding; every launch that could read them rewrites them first (the argument of _prefill's comment)."""

    def __init__(self, model, state: dict, capacity: int, pos_shift: int = 0, prefix_rows: int = 0):
        self._model, self._decoder, self._state = model, model.decoder, state
        self.capacity = int(capacity)
        self._pos_shift = int(pos_shift)
        self.prefix_rows = int(prefix_rows)           # spliced image rows of the first prompt: counted in ``lengths``, not text ids
        self.batch = int(state["batch"])
        self.lengths = [0] * self.batch
        self._cached = [0] * self.batch               # valid cache rows per sequence
        self._text = [None] * self.batch              # the conversation's text ids per row (device, int64 [n])
        self._pending = [None] * self.batch           # the sampled-but-unfed token per row (device, int64 [1]) or None

    # -- host-side checks: before the device check and any launch --
    def _check_turn(self, x, prompt_lengths):
        if not isinstance(x, torch.Tensor):
            raise TypeError("x must be an instance of torch.Tensor")
        if x.dim() != 2 or x.shape[1] < 1:
            raise ValueError(f"x must be [batch, new tokens] with at least one token, got {tuple(x.shape)}")
        if x.shape[0] != self.batch:
            raise ValueError(f"x holds {x.shape[0]} rows, the session {self.batch}: a session keeps its batch size")
        if prompt_lengths is None:
            return [x.shape[1]] * self.batch
        return resolve_prompt_lengths(prompt_lengths, self.batch, x.shape[1])

    def _check_room(self, block_width: int, new_tokens: int):
        """The conservative budget: the padded block's rows need cache room too (there is no per-row row count on the device)."""
        need = max(self._cached) + block_width + new_tokens
        if need > self.capacity:
            raise IndexError(f"index out of range in self: {max(self._cached)} cached rows + a block of {block_width} rows + "
                             f"{new_tokens} new tokens exceed the session's {self.capacity}-row cache")

    def _advance(self, new_text, cached, block_lens, out, n_valid):
        """After a turn: ``new_text`` per row the ids the turn brought in (device), ``out`` [B, n] what it generated (or None)."""
        self.lengths, self._cached, pend = session_after_turn(cached, block_lens, n_valid)
        for b in range(self.batch):
            parts = [t for t in (self._text[b], new_text[b]) if t is not None]
            if out is not None and n_valid[b] > 0:
                parts.append(out[b, :n_valid[b]])
                self._pending[b] = out[b, pend[b]:pend[b] + 1].clone()
            else:
                self._pending[b] = None
            self._text[b] = torch.cat(parts)

    def _block(self, x, lens):
        """The turn's block [B, W] (pending token, then the row's new ids; right-padded with the row's first id), its lengths and
        the conversation's text ids with the new ones [B, Wt] (padded the same way) with their lengths."""
        rows = [x[b, :l] if self._pending[b] is None else torch.cat([self._pending[b], x[b, :l]]) for b, l in enumerate(lens)]
        block_lens = [int(r.shape[0]) for r in rows]
        hist = [torch.cat([self._text[b], x[b, :l]]) for b, l in enumerate(lens)]
        hist_lens = [int(h.shape[0]) for h in hist]
        pad = torch.nn.utils.rnn.pad_sequence
        return (mask_padding(pad(rows, batch_first=True), block_lens), block_lens,
                mask_padding(pad(hist, batch_first=True), hist_lens), hist_lens)

    def _extend(self, block, block_lens, chunk, want_logits: bool):
        """The block through Decoder._extend_ragged, ``chunk`` columns at a time; a slice computes logits only if it holds a row's
        last position.  Returns the [B, 1, V] rows the loop reads (None without ``want_logits``).  Moves the device positions to
        the rows' new valid lengths."""
        state, dec, prec = self._state, self._decoder, self._model.precision
        dev, B, W = block.device, self.batch, block.shape[1]
        base = torch.tensor(self._cached, dtype=torch.int32, device=dev)
        state["positions"], state["pos_max"] = base, max(self._cached)
        step = W if chunk is None else min(chunk, W)
        rows = None
        for s0 in range(0, W, step):
            s1 = min(s0 + step, W)
            want = [b for b in range(B) if s0 <= block_lens[b] - 1 < s1] if want_logits else []
            logits = dec._extend_ragged(block[:, s0:s1], state, base if s0 == 0 else base + s0, prec, output_logits=bool(want),
                                        pos_shift=self._pos_shift)
            if want:
                if rows is None:
                    rows = torch.empty((B, 1, logits.shape[2]), dtype=torch.float32, device=dev)
                idx = torch.tensor(want, dtype=torch.int64, device=dev)
                rows[idx, 0] = logits[idx, torch.tensor([block_lens[b] - 1 - s0 for b in want], dtype=torch.int64, device=dev)]
        return rows

    def generate(self, x: torch.Tensor, max_new_tokens: int, *, prompt_lengths=None, do_sample=False, temperature=1.0, top_k=0,
                 top_p=1.0, repetition_penalty=1.0, seed=0, eos_token_id=None, pad_token_id=1, sequence_ids=None, eos_poll=8,
                 output_logits=False, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0, stop_sequences=None,
                 prefill_chunk=None, output_logprobs=False, top_logprobs=0, token_automaton=None, automaton_start=None,
                 logit_bias=None, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0,
                 row_options=None):
        """One more turn: ``x`` [B, Tn] int64 holds the new turn's ids only (``prompt_lengths``: row b's are x[b, :prompt_lengths[b]],
        at least one), the other arguments are the plain loop's, as in generate().  Returns what generate() returns and advances the
        session in place.  The Philox position of a token is the absolute position it will occupy; the repetition penalty and the
        constraints see the text ids of the whole conversation.  A turn that does not fit — the longest row's cached rows + the
        padded block's width + ``max_new_tokens`` > capacity — raises IndexError before any launch and leaves the session where it
        was.  An error after the first launch (an id outside the vocabulary) leaves it where it was too: the rows the turn wrote
        lie at or after every row's valid length.
        ``token_automaton`` / ``automaton_start``: this turn's own automaton, every row beginning in its start state — the states of
        an earlier turn are not kept, and the automaton reads the turn's output only.
        ``logit_bias`` / ``presence_penalty`` / ``frequency_penalty`` / ``min_p``: as in generate(); the penalties count what THIS turn
        emitted — every turn starts from zero counts, and neither the prompt nor an earlier turn's output counts.
        ``typical_p`` / ``epsilon_cutoff`` / ``eta_cutoff``: as in generate().
        ``row_options``: this turn's own per-row options, as in generate(); a row's budget ends its turn after that many tokens."""
        kw = _keywords(locals(), "self", "x", "prompt_lengths", "prefill_chunk")
        lens = self._check_turn(x, prompt_lengths)
        opts = loop_options(self._model.embed.weight.shape[0], self.batch, **kw)
        chunk = check_prefill_chunk(prefill_chunk)
        if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or max_new_tokens < 1:
            raise ValueError(f"max_new_tokens must be a positive integer, got {max_new_tokens!r}")
        width = max(l + (self._pending[b] is not None) for b, l in enumerate(lens))
        self._check_room(width, max_new_tokens)
        _need_device(x)
        with torch.no_grad():
            x = x.long()
            block, block_lens, history, hist_lens = self._block(x, lens)
            cached = list(self._cached)
            try:
                rows = self._extend(block, block_lens, chunk, True)
                starts = [c + bl for c, bl in zip(cached, block_lens)]
                res, n_valid = _loop_turn(self, rows, history, hist_lens, starts, max_new_tokens, opts)
            finally:
                self._state["pos_max"] = max(self._cached)
            out = res[0] if isinstance(res, tuple) else res
            self._advance([x[b, :l] for b, l in enumerate(lens)], cached, block_lens, out, n_valid)
            self._state["pos_max"] = max(self._cached)
        return res

    def append(self, x: torch.Tensor, *, prompt_lengths=None, prefill_chunk=None):
        """Known tokens — a tool result, a system turn — into every row's cache; nothing is generated and no logits are computed.
        ``x`` and ``prompt_lengths`` as in generate().  IndexError before any launch when the padded block does not fit."""
        lens = self._check_turn(x, prompt_lengths)
        chunk = check_prefill_chunk(prefill_chunk)
        width = max(l + (self._pending[b] is not None) for b, l in enumerate(lens))
        self._check_room(width, 0)
        _need_device(x)
        with torch.no_grad():
            x = x.long()
            block, block_lens, _, _ = self._block(x, lens)
            cached = list(self._cached)
            try:
                self._extend(block, block_lens, chunk, False)
                word = int(self._state["error"].item())
                _raise_position_error(word, self._state)
            finally:
                self._state["pos_max"] = max(self._cached)
            # every id of the block was fed: the rows are cached, nothing is pending (n_valid = 0 rows keep lengths = cached)
            self._advance([x[b, :l] for b, l in enumerate(lens)], cached, block_lens, None, [0] * self.batch)
            self._state["pos_max"] = max(self._cached)


def _need_device(x):
    from .model import _require_cuda
    _require_cuda(x, "x")
