"""Token automata for constrained decoding (``generate(..., token_automaton=...)``): host-side construction, no GPU needed.

A TokenAutomaton is a deterministic automaton over token ids.  State s lists some ids with the state each leads to (-1: the id is
banned in s) and has a default for every id it does not list (-1: every unlisted id is banned).  generate() uploads its tables()
once and kx_automaton_step (include/kosmosx_hip.h) walks them on the device: before every sampler launch or beam step the row's
state advances on the token just emitted and the ids the new state bans get -inf logits.  A state with no way out ends a row (the
sampler emits pad and marks it finished); under beam search a hypothesis ends by the EOS alone, so grammars for beams end in an
EOS edge (from_choices(..., eos_token_id=...)).

The text tokenizer stays out of scope: compiling a regular expression or a schema down to ids is the caller's business."""
from __future__ import annotations

import operator

import numpy as np


def _index(v, what: str) -> int:
    if isinstance(v, bool):
        raise ValueError(f"{what} must be an integer, got {v!r}")
    try:
        return operator.index(v)
    except TypeError:
        raise ValueError(f"{what} must be an integer, got {v!r}") from None


class TokenAutomaton:
    """``edges[s]``: a mapping id -> next state of state s (None or -1: the id is banned there).  ``default[s]``: where an id that
    state s does not list leads; -1 bans every unlisted id, and ``default=None`` means -1 everywhere.  ``start``: the state a row
    begins in unless generate() is given an ``automaton_start``.  ValueError names the field that is wrong."""

    def __init__(self, edges, default=None, start=0):
        if isinstance(edges, (str, bytes)) or not hasattr(edges, "__len__") or hasattr(edges, "keys"):
            raise ValueError(f"edges must be a sequence with one id -> next state mapping per state, got {type(edges).__name__}")
        S = len(edges)
        if S < 1:
            raise ValueError("edges is empty: an automaton has at least one state")
        self.edges = []
        for s, e in enumerate(edges):
            if not hasattr(e, "items"):
                raise ValueError(f"edges[{s}] must be a mapping id -> next state, got {type(e).__name__}")
            row = {}
            for t, nx in e.items():
                t = _index(t, f"edges[{s}]: a token id")
                if not 0 <= t < 2 ** 31:
                    raise ValueError(f"edges[{s}] lists the id {t}: token ids are non-negative (and below 2^31)")
                nx = -1 if nx is None else _index(nx, f"edges[{s}][{t}]")
                if not -1 <= nx < S:
                    raise ValueError(f"edges[{s}][{t}] = {nx} is outside the {S} states (None or -1 bans the id)")
                row[t] = nx
            self.edges.append(dict(sorted(row.items())))
        if default is None:
            self.default = [-1] * S
        else:
            if isinstance(default, (str, bytes)) or not hasattr(default, "__len__") or len(default) != S:
                raise ValueError(f"default must have one entry per state ({S}), got {default!r}")
            self.default = [_index(d, f"default[{s}]") for s, d in enumerate(default)]
            for s, d in enumerate(self.default):
                if not -1 <= d < S:
                    raise ValueError(f"default[{s}] = {d} is outside the {S} states (-1 bans every unlisted id)")
        self.start = _index(start, "start")
        if not 0 <= self.start < S:
            raise ValueError(f"start = {self.start} is outside the {S} states")

    @property
    def num_states(self) -> int:
        return len(self.edges)

    @property
    def max_token(self) -> int:
        """The largest id any state lists (-1: none does)."""
        return max((max(e) for e in self.edges if e), default=-1)

    # -- constructors --
    @classmethod
    def from_choices(cls, choices, eos_token_id=None):
        """The output must be exactly one of ``choices`` (lists of ids): a trie, shared prefixes merged.  With an ``eos_token_id``
        every choice's node gets an EOS edge to a state with no way out; without one a choice's node has no way out itself, and a
        choice that is a proper prefix of another is refused."""
        if isinstance(choices, (str, bytes)) or not hasattr(choices, "__iter__"):
            raise ValueError(f"choices must be a list of non-empty lists of token ids, got {choices!r}")
        eos = None if eos_token_id is None else _index(eos_token_id, "eos_token_id")
        if eos is not None and eos < 0:
            raise ValueError(f"eos_token_id = {eos}: token ids are non-negative")
        edges, ends = [{}], []
        for c, choice in enumerate(choices):
            if isinstance(choice, (str, bytes)) or not hasattr(choice, "__iter__"):
                raise ValueError(f"choices[{c}] must be a list of token ids, got {choice!r}")
            ids = [_index(t, f"choices[{c}]: a token id") for t in choice]
            if not ids:
                raise ValueError(f"choices[{c}] is empty: a choice holds at least one token id")
            s = 0
            for t in ids:
                if t < 0:
                    raise ValueError(f"choices[{c}] holds the id {t}: token ids are non-negative")
                if t == eos:
                    raise ValueError(f"choices[{c}] holds the eos_token_id {eos}: the EOS edge is added behind every choice")
                if t not in edges[s]:
                    edges.append({})
                    edges[s][t] = len(edges) - 1
                s = edges[s][t]
            ends.append(s)
        if not ends:
            raise ValueError("choices is empty: there is nothing the output may be")
        if eos is None:
            for c, s in enumerate(ends):
                if edges[s]:
                    raise ValueError(f"choices[{c}] is a proper prefix of another choice: without an eos_token_id nothing tells "
                                     "the two apart")
        else:
            edges.append({})                                # the state behind the EOS: no way out
            for s in ends:
                edges[s][eos] = len(edges) - 1
        return cls(edges)

    @classmethod
    def from_allowed(cls, ids):
        """One state that loops on the whitelist ``ids``."""
        if isinstance(ids, (str, bytes)) or not hasattr(ids, "__iter__"):
            raise ValueError(f"ids must be a list of token ids, got {ids!r}")
        allowed = [_index(t, "ids: a token id") for t in ids]
        if not allowed:
            raise ValueError("ids is empty: a whitelist allows at least one token id")
        for t in allowed:
            if t < 0:
                raise ValueError(f"ids holds {t}: token ids are non-negative")
        return cls([{t: 0 for t in allowed}])

    @classmethod
    def union(cls, automata):
        """Disjoint copies of ``automata`` in one table, for batches whose rows have different grammars.  Returns (automaton, starts):
        starts[i] is the start state of copy i, what ``automaton_start`` takes.  The union's own ``start`` is starts[0]."""
        automata = list(automata)
        if not automata:
            raise ValueError("automata is empty: a union holds at least one automaton")
        edges, default, starts = [], [], []
        for i, a in enumerate(automata):
            if not isinstance(a, TokenAutomaton):
                raise ValueError(f"automata[{i}] must be a TokenAutomaton, got {type(a).__name__}")
            base = len(edges)
            starts.append(base + a.start)
            edges += [{t: (nx + base if nx >= 0 else -1) for t, nx in e.items()} for e in a.edges]
            default += [d + base if d >= 0 else -1 for d in a.default]
        return cls(edges, default, starts[0]), starts

    # -- queries --
    def walk(self, ids, start=None) -> int:
        """The state after ``ids`` from ``start`` (default: the automaton's), or -1 once an id is banned."""
        s = self.start if start is None else _index(start, "start")
        if not -1 <= s < self.num_states:
            raise ValueError(f"start = {s} is outside the {self.num_states} states")
        for t in ids:
            if s < 0:
                return -1
            t = int(t)
            s = -1 if t < 0 else self.edges[s].get(t, self.default[s])
        return s

    def allowed(self, state: int, vocab_size: int) -> np.ndarray:
        """bool [vocab_size]: the ids ``state`` allows (all False in the dead state -1)."""
        out = np.zeros(int(vocab_size), dtype=bool)
        if state < 0:
            return out
        out[:] = self.default[state] >= 0
        for t, nx in self.edges[state].items():
            if t < vocab_size:
                out[t] = nx >= 0
        return out

    def accepts_eos(self, state: int, eos: int) -> bool:
        """Whether ``state`` allows the id ``eos``."""
        return state >= 0 and self.edges[state].get(int(eos), self.default[state]) >= 0

    def tables(self):
        """(edge_off int32 [S + 1], edge_tok int32 [E], edge_next int32 [E], default_next int32 [S]): the CSR form
        ops.AutomatonTable uploads, ids ascending within a state."""
        off = np.zeros(self.num_states + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(e) for e in self.edges])
        tok = np.array([t for e in self.edges for t in e], dtype=np.int32)
        nxt = np.array([nx for e in self.edges for nx in e.values()], dtype=np.int32)
        return off, tok, nxt, np.array(self.default, dtype=np.int32)

    def check_vocab(self, vocab_size: int):
        """ValueError when a state lists an id outside [0, vocab_size)."""
        for s, e in enumerate(self.edges):
            if e and max(e) >= vocab_size:
                raise ValueError(f"edges[{s}] lists the id {max(e)}, outside the vocabulary [0, {vocab_size})")
