"""What generate() launches and what it returns, pinned against a recording.

tests/golden/generate_launches.json holds, per case below, the library entry points the call fetched — in order, run-length
encoded — and the tokens it returned, recorded on the MI355X from the commit the file names (``_recorded_from``): the last one
before generate_loop took its options resolved (generation.LoopOptions).  Host-side work on how the options reach the loops must
change neither.  The cases use the public generate() / Session.generate only, so this file records from any commit:

    python tests/test_generate_launches_gpu.py OUT.json COMMIT

Shapes: the tiny text model of the other generate tests, fp32, B = 3, T = 9, 6 new tokens, eos_poll = 2 — the smallest at which
every dispatch path (uniform, ragged, prefix, guided 2B rows, session extend, beams, lookup) and the stop poll still run."""
import functools
import json
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]

from helpers import tiny_config
from kosmosx import generation as G
from kosmosx import ops
from kosmosx.automaton import TokenAutomaton
from kosmosx.model import Kosmos, KosmosLanguage

pytestmark = pytest.mark.gpu

GOLDEN = ROOT / "tests" / "golden" / "generate_launches.json"
V, B, T, N = 102, 3, 9, 6
LENS = [4, 9, 6]
COMMON = dict(pad_token_id=1, eos_poll=2)
SAMPLE = dict(do_sample=True, temperature=0.8, top_k=40, top_p=0.95, seed=21)
BIAS = [{12: 50.0, 7: -1.0}, {}, {33: 2.0, 30: float("-inf")}]
AUTO, STARTS = TokenAutomaton.union([TokenAutomaton.from_allowed(range(8, 24)), TokenAutomaton.from_allowed(range(20, 60)),
                                     TokenAutomaton.from_allowed(range(28, 40))])


class Models:
    def __init__(self):
        self.lm = KosmosLanguage(vocab_size=V, dim=128, depth=2, ffn_dim=256, decoder_heads=2, _seed=5, _perturb=0.1,
                                 _max_positions=64).eval().to("cuda")
        self.mm = Kosmos._from_config(tiny_config(), seed=1, perturb=0.1).eval().to("cuda")
        self.lm.precision = self.mm.precision = "fp32"
        g = torch.Generator().manual_seed(4)
        self.tok = torch.randint(2, V, (B, T), generator=g).cuda()
        self.neg = torch.randint(2, V, (B, 4), generator=g).cuda()
        self.turn = torch.randint(2, V, (B, 3), generator=g).cuda()
        self.mm_tok = torch.randint(2, self.mm.cfg.vocab, (2, 10), generator=g).cuda()
        self.img = torch.randn(2, 3, self.mm.cfg.vit.image, self.mm.cfg.vit.image, generator=g).cuda()
        # an EOS that row 0 reaches at its third token: the id it draws there when nothing ends a row
        self.eos = int(self.lm.generate(self.tok, N, **COMMON, **SAMPLE)[0, 2])


def _greedy(m):
    return [m.lm.generate(m.tok, N, **COMMON)]


def _sampled_eos(m):
    return [m.lm.generate(m.tok, N, eos_token_id=m.eos, **COMMON, **SAMPLE)]


def _ragged(m):
    return [m.lm.generate(m.tok, N, prompt_lengths=LENS, **COMMON)]


def _everything(m):
    return [m.lm.generate(m.tok, N, prompt_lengths=LENS, eos_token_id=5, no_repeat_ngram_size=3, bad_words_ids=[[9], [21, 22]],
                          min_new_tokens=2, stop_sequences=[[12, 12]], token_automaton=AUTO, automaton_start=STARTS,
                          logit_bias=BIAS, presence_penalty=0.4, frequency_penalty=0.7, min_p=0.05, typical_p=0.9,
                          output_logprobs=True, top_logprobs=3, output_logits=True, **COMMON, **SAMPLE)]


def _parallel(m):
    return [m.lm.generate(m.tok, N, num_return_sequences=2, logit_bias=BIAS, token_automaton=AUTO, automaton_start=STARTS,
                          **COMMON, **SAMPLE)]


def _guided(m):
    return [m.lm.generate(m.tok, N, guidance_scale=1.5, negative_prompt_ids=m.neg, **COMMON)]


def _session(m):
    out, session = m.lm.generate(m.tok, N, return_session=True, **COMMON)
    return [out, session.generate(m.turn, N, frequency_penalty=0.7, **COMMON, **SAMPLE)]


def _beams(m):
    return [m.lm.generate(m.tok, N, num_beams=3, **COMMON)]


def _lookup(m):
    return [m.lm.generate(m.tok, N, prompt_lookup_num_tokens=2, **COMMON)]


def _multimodal(m):
    return [m.mm.generate(m.mm_tok, m.img, N, prompt_lengths=[5, 10], **COMMON, **dict(SAMPLE, top_k=20))]


CASES = dict(greedy=_greedy, sampled_eos=_sampled_eos, ragged=_ragged, everything=_everything, parallel=_parallel, guided=_guided,
             session=_session, beams=_beams, lookup=_lookup, multimodal=_multimodal)


def _run(case, m):
    """-> (the entry points ``case`` fetched as [[name, times], ...], its tokens).  The case runs once before the recorded run, so
    that whatever a first call sets up (packed weights, workspaces, tables) is not part of the record."""
    case(m)
    load, real, names = ops.H.load, ops.H.load(), []

    class Spy:
        def __getattr__(self, name):
            names.append(name)
            return getattr(real, name)

    ops.H.load = lambda: Spy()
    try:
        outs = case(m)
    finally:
        ops.H.load = load
    runs = []
    for name in names:
        if runs and runs[-1][0] == name:
            runs[-1][1] += 1
        else:
            runs.append([name, 1])
    return runs, [(o[0] if isinstance(o, tuple) else o).cpu().tolist() for o in outs]


@pytest.fixture(scope="module")
def models():
    return Models()


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("name", list(CASES))
def test_the_launches_and_the_tokens_are_the_recorded_ones(name, models, golden):
    launches, tokens = _run(CASES[name], models)
    want = golden[name]
    assert tokens == want["tokens"], name
    assert launches == want["launches"], name


def test_the_cases_reach_what_they_are_there_for(models, golden):
    row = golden["sampled_eos"]["tokens"][0][0]
    assert row[2] == models.eos and row[3:] == [1] * (N - 3)                # row 0 ends at the EOS and is padded behind it
    assert golden["everything"]["tokens"][0][0][:2] == [12, 12]             # ... and at the stop sequence
    assert len(golden["parallel"]["tokens"][0]) == 2 * B and len(golden["session"]["tokens"]) == 2
    for name, entry in (("ragged", "kx_sample_logits_ragged"), ("everything", "kx_shape_logits"), ("everything", "kx_automaton_step"),
                        ("everything", "kx_constrain_logits"), ("everything", "kx_step_logprobs"), ("guided", "kx_guidance_logits"),
                        ("beams", "kx_beam_step"), ("lookup", "kx_spec_accept")):
        assert any(n == entry for n, _ in golden[name]["launches"]), (name, entry)


def test_every_option_is_validated_once_per_call(models, monkeypatch):
    """The parallel path used to parse a per-row ``logit_bias`` three times: in run_generate, parallel_loop and generate_loop."""
    calls = []
    for check in ("check_constraint_args", "check_logprob_args", "check_automaton_args", "check_shape_args", "check_truncation_args",
                  "check_guidance_args"):
        def counted(*a, _real=getattr(G, check), _name=check, **k):
            calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(G, check, functools.wraps(getattr(G, check))(counted))
    models.lm.generate(models.tok, N, logit_bias=BIAS, num_return_sequences=2, do_sample=True)
    assert calls.count("check_shape_args") == 1
    assert sorted(calls) == sorted(set(calls)), calls


if __name__ == "__main__":
    m = Models()
    rec = {"_recorded_from": sys.argv[2]}
    for name, case in CASES.items():
        launches, tokens = _run(case, m)
        rec[name] = dict(launches=launches, tokens=tokens)
    lines = ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in rec.items())
    Path(sys.argv[1]).write_text("{\n" + lines + "\n}\n")
    print(f"recorded {len(CASES)} cases from {sys.argv[2]} into {sys.argv[1]}")
