"""The contract of kx_spec_accept (include/kosmosx_hip.h, "Speculative decoding by prompt lookup") in plain Python, one sequence at a
time, and a simulation of the whole lookup loop over a deterministic next-token function.  No torch, no numpy: lists of ints."""


def accept_count(fed, picked):
    """a = the largest value with fed[j] == picked[j - 1] for all 1 <= j <= a (0 for a one-row block)."""
    a = 0
    while a + 1 < len(picked) and fed[a + 1] == picked[a]:
        a += 1
    return a


def lookup(s, n_drafts, ngram_max):
    """The drafts after the logical sequence s: for n = ngram_max down to 1 with len(s) > n, the LARGEST i <= len - n - 1 with
    s[i:i+n] == s[len-n:len]; the drafts continue the match and wrap at the sequence's end.  No match: the last token repeated."""
    L = len(s)
    for n in range(min(ngram_max, L - 1), 0, -1):
        suffix = s[L - n:]
        for i in range(L - n - 1, -1, -1):
            if s[i:i + n] == suffix:
                p = L - (i + n)
                return [s[i + n + (m % p)] for m in range(n_drafts)]
    return [s[-1]] * n_drafts


def new_state(prompt, prefill_len=None):
    """Per-sequence state before step 0: history = the prompt's ids; positions are initialised by step 0."""
    return dict(history=list(prompt), out=[], out_src=[], finished=False, base=None,
                prefill_len=len(prompt) if prefill_len is None else prefill_len)


def step(st, fed, picked, *, K, max_new, step_index, ngram_max=2, eos=None, pad=1, draft_from=None):
    """One kx_spec_accept on one sequence.  ``picked``: Kin picks (Kin = 1 at step 0, K afterwards), ``fed`` the Kin tokens fed
    (unused at Kin = 1).  Mutates ``st``; returns (emitted count, next block's K tokens)."""
    Kin = len(picked)
    assert Kin in (1, K)
    if st["finished"]:                                     # emits nothing, moves nothing, is fed pad
        return 0, [pad] * K
    base = st["prefill_len"] - 1 if Kin == 1 else st["base"]
    a = accept_count(fed, picked) if Kin > 1 else 0
    e = min(a + 1, max_new - len(st["out"]))
    toks = []
    for j in range(e):
        toks.append(picked[j])
        if eos is not None and eos >= 0 and picked[j] == eos:
            st["finished"] = True
            break
    e = len(toks)
    for j, t in enumerate(toks):
        st["out"].append(t)
        st["history"].append(t)
        st["out_src"].append(step_index * K + j)
    if e > 0 or Kin == 1:
        st["base"] = base + e
    if len(st["out"]) >= max_new:
        st["finished"] = True
    if st["finished"]:
        return e, [pad] * K
    last = toks[-1]
    if draft_from is not None:
        n = len(st["out"])
        drafts = [draft_from[n + m - 1] if n + m - 1 < len(draft_from) else last for m in range(1, K)]
    else:
        drafts = lookup(st["history"], K - 1, ngram_max)
    return e, [last] + drafts


def greedy(next_token_fn, prompt, n, eos=None):
    """Plain greedy decoding: one token per call of the model."""
    out = []
    while len(out) < n:
        t = next_token_fn(list(prompt) + out)
        out.append(t)
        if eos is not None and t == eos:
            break
    return out


def run(next_token_fn, prompt, n, D, ngram=2, eos=None, draft_from=None, pad=1):
    """The lookup loop over ``next_token_fn(sequence) -> next id``: returns (tokens, emitted per step).  Row j of a block is the
    model after the confirmed sequence (which ends in the block's row 0) followed by the block's drafts 1..j."""
    K = D + 1
    st = new_state(prompt)
    emitted = []
    picked = [next_token_fn(list(prompt))]
    fed = None
    for g in range(n):
        before = len(st["history"])
        e, nxt = step(st, fed, picked, K=K, max_new=n, step_index=g, ngram_max=ngram, eos=eos, pad=pad, draft_from=draft_from)
        emitted.append(e)
        assert e >= 1 and len(st["history"]) == before + e
        if st["finished"]:
            break
        fed = nxt
        confirmed = st["history"]                           # ends in fed[0]
        picked = [next_token_fn(confirmed + fed[1:j + 1]) for j in range(K)]
    assert st["finished"]
    return st["out"], emitted
