"""generate() on the full-size text decoder: ms per token of
  (a) KosmosLanguage.generate() — decode step + the fused on-device sampler, token kept on the device;
  (b) the same loop with a sampler composed from torch ops (sort / softmax / cumsum / multinomial) and a host token feed
      through the public incremental path — what a caller had to write before generate() existed;
  (c) the bare decode step (tools/bench_decode.py's loop) in the same process.
One JSON line per batch size.  --only a|b|c restricts the run to one variant (for a kernel trace of that variant alone).

--ragged: the ragged-batch leg instead of (b) and (c).  Row b's prompt has lengths[b] tokens, spread evenly over
[--min-prefix, --prefix], right-padded to --prefix:
  (a) uniform generate() over the full-width prompts, as above;
  (r) generate(prompt_lengths=lengths): ms per token after the (same-shape) prefill, and tokens per second of the whole call;
  (s) one generate() per row over its own unpadded prompt — what a caller with unequal prompts had to do before: tokens per
      second over all B calls, prefills included.
--only a|r|s restricts the run.

--num-beams W: the beam-search leg alone.  Per batch size B, alternating, best of --reps each:
  (w) generate(num_beams=W) at B rows: ms per token after the prefill (beam step + cache gather + decode step at B * W rows);
  (p) plain greedy generate() at B * W rows — the decode step of the same width without the search.
--only w|p restricts the run (for a kernel trace of one variant).

--no-repeat-ngram N and/or --bad-words K (K random entries, alternately one and two ids long): the constraints leg alone.  Per
batch size, alternating, best of --reps each:
  (a) generate() with every constraint at its default — no kx_constrain_logits launch;
  (k) generate(no_repeat_ngram_size=N, bad_words_ids=[...]) — one kx_constrain_logits launch per token in front of the sampler.
--only a|k restricts the run (for a kernel trace of one variant).

--prompt-lookup D: the prompt-lookup speculation leg alone (greedy; B * (D + 1) <= 16).  The prompt is a block of --prefix / 4
random tokens four times over.  Per batch size, alternating, best of --reps each; every leg prints ms per EMITTED token after the
prefill and the tokens emitted per verify step:
  (g) plain greedy generate() — one token per step;
  (l) generate(prompt_lookup_num_tokens=D) — the lookup proper, on whatever the (random-weight) model makes of the repeated prompt;
  (u) _draft_from = the plain run's own output: every draft is right, the upper bound;
  (x) _draft_from = that output with every id changed: every draft is wrong, the price of the K-row step when nothing is accepted.
--only g|l|u|x restricts the run (for a kernel trace of one variant)."""
import argparse, json, os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx import _hip
from kosmosx.model import KosmosLanguage

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,4,8,16")
ap.add_argument("--prefix", type=int, default=114)
ap.add_argument("--new", type=int, default=64)
ap.add_argument("--precision", default="mixed")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--only", default=None)
ap.add_argument("--ragged", action="store_true")
ap.add_argument("--min-prefix", type=int, default=16)
ap.add_argument("--num-beams", type=int, default=0)
ap.add_argument("--no-repeat-ngram", type=int, default=0)
ap.add_argument("--bad-words", type=int, default=0)
ap.add_argument("--prompt-lookup", type=int, default=0)
ap.add_argument("--ngram", type=int, default=2)
ap.add_argument("--eos-poll", type=int, default=2)   # (the lookup leg: a row that finished keeps stepping until the poll notices)
a = ap.parse_args()
constrained = bool(a.no_repeat_ngram or a.bad_words)
if a.only is None:
    a.only = "glux" if a.prompt_lookup else "wp" if a.num_beams else "ak" if constrained else "ars" if a.ragged else "abc"
dev = torch.device("cuda", 0)
V = 32002
m = KosmosLanguage(vocab_size=V, dim=2048, _seed=0).eval().to(dev)
m.precision = a.precision
KW = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, seed=1)


def torch_sample(logits, gen):
    """temperature -> top-k -> top-p -> multinomial, the usual composition (transformers' order)."""
    x = logits / 0.8
    kth = torch.topk(x, 50, dim=-1).values[:, -1:]
    x = x.masked_fill(x < kth, float("-inf"))
    srt, idx = torch.sort(x, dim=-1, descending=False)
    cum = srt.softmax(-1).cumsum(-1)
    drop = cum <= 1.0 - 0.9
    drop[:, -1] = False
    x = x.masked_fill(drop.scatter(1, idx, drop), float("-inf"))
    return torch.multinomial(x.softmax(-1), 1, generator=gen)


def run_a(tok):
    return m.generate(tok, a.new, **KW)


def run_b(tok):
    gen = torch.Generator(device=dev).manual_seed(1)
    state, seq = {"max_len": a.prefix + a.new}, tok
    out = m(seq, incremental_state=state)
    for g in range(a.new):
        nxt = torch_sample(out[:, -1], gen)
        seq = torch.cat([seq, torch.from_numpy(nxt.cpu().numpy()).to(dev)], 1)     # host token feed
        if g + 1 < a.new:
            out = m(seq, incremental_state=state)
    return seq[:, a.prefix:]


def run_c(tok_all):
    state = {"max_len": a.prefix + a.new}
    out = m(tok_all[:, : a.prefix], incremental_state=state)
    for t in range(a.prefix, a.prefix + a.new - 1):
        out = m(tok_all[:, : t + 1], incremental_state=state)
    return out


def lengths_of(B):
    return [a.prefix] if B == 1 else [a.min_prefix + round(i * (a.prefix - a.min_prefix) / (B - 1)) for i in range(B)]


def run_r(tok):
    return m.generate(tok, a.new, prompt_lengths=lengths_of(tok.shape[0]), **KW)


def run_s(tok):
    ids = torch.arange(tok.shape[0], device=dev)
    return [m.generate(tok[b:b + 1, :L].contiguous(), a.new, sequence_ids=ids[b:b + 1], **KW) for b, L in enumerate(lengths_of(tok.shape[0]))]


def timed(fn, arg):
    best = None
    for rep in range(a.reps + 1):                               # rep 0 = warm-up (packs weights, sizes workspaces)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(arg)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep:
            best = dt if best is None else min(best, dt)
    return best


def beam_leg():
    W = a.num_beams
    for B in (int(b) for b in a.batches.split(",")):
        wide = torch.randint(0, V, (B * W, a.prefix), generator=torch.Generator().manual_seed(0)).to(dev)
        tok = wide[:B].contiguous()
        mk = lambda rows: (lambda t: m(t, incremental_state={"max_len": a.prefix + a.new}), rows)
        runs = {"w": (lambda t: m.generate(t, a.new, num_beams=W), tok), "p": (lambda t: m.generate(t, a.new), wide)}
        pre = {"w": timed(*mk(tok)), "p": timed(*mk(wide))}
        best = {}
        for rep in range(a.reps):                               # alternating, so that both see the same clocks
            for k in a.only:
                dt = timed_once(*runs[k], warm=rep == 0)
                best[k] = min(best.get(k, dt), dt)
        res = {"workload": f"KosmosLanguage beam search, B={B}, num_beams={W}, prefix {a.prefix}, {a.new} new tokens, {a.precision}"}
        if "w" in best:
            res["w_beam_ms_per_token"] = round((best["w"] - pre["w"]) / (a.new - 1) * 1e3, 4)
            res["w_prefill_ms"] = round(pre["w"] * 1e3, 3)
        if "p" in best:
            res[f"p_greedy_b{B * W}_ms_per_token"] = round((best["p"] - pre["p"]) / (a.new - 1) * 1e3, 4)
            res["p_prefill_ms"] = round(pre["p"] * 1e3, 3)
        print(json.dumps(res), flush=True)


def timed_once(fn, arg, warm=False):
    for rep in range(2 if warm else 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(arg)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return dt


def constraints_leg():
    g = torch.Generator().manual_seed(2)
    words = [torch.randint(0, V, (1 + k % 2,), generator=g).tolist() for k in range(a.bad_words)]
    CONS = dict(no_repeat_ngram_size=a.no_repeat_ngram, bad_words_ids=words or None)
    for B in (int(b) for b in a.batches.split(",")):
        tok = torch.randint(0, V, (B, a.prefix), generator=torch.Generator().manual_seed(0)).to(dev)
        pre = timed(lambda t: m(t, incremental_state={"max_len": a.prefix + a.new}), tok)
        runs = {"a": lambda t: m.generate(t, a.new, **KW), "k": lambda t: m.generate(t, a.new, **KW, **CONS)}
        best = {}
        for rep in range(a.reps):                               # alternating, so that both see the same clocks
            for k in a.only:
                dt = timed_once(runs[k], tok, warm=rep == 0)
                best[k] = min(best.get(k, dt), dt)
        res = {"workload": f"KosmosLanguage generate with constraints, B={B}, prefix {a.prefix}, {a.new} new tokens, {a.precision}, "
                           f"top_k=50 top_p=0.9 temperature=0.8, no_repeat_ngram_size={a.no_repeat_ngram}, {a.bad_words} bad words",
               "prefill_ms": round(pre * 1e3, 3)}
        for k, name in (("a", "a_defaults_ms_per_token"), ("k", "k_constrained_ms_per_token")):
            if k in best:
                res[name] = round((best[k] - pre) / (a.new - 1) * 1e3, 4)
        if len(best) == 2:
            res["k_minus_a_us_per_token"] = round((best["k"] - best["a"]) / (a.new - 1) * 1e6, 2)
        print(json.dumps(res), flush=True)


def lookup_leg():
    D = a.prompt_lookup
    for B in (int(b) for b in a.batches.split(",")):
        if B * (D + 1) > 16:
            print(json.dumps({"skipped": f"B={B}: {B} x {D + 1} rows exceed the 16 rows of a weight-streaming step"}), flush=True)
            continue
        block = torch.randint(0, V, (B, max(a.prefix // 4, 1)), generator=torch.Generator().manual_seed(0))
        tok = block.repeat(1, 4).to(dev)
        T = tok.shape[1]
        pre = timed(lambda t: m(t, incremental_state={"max_len": T + a.new + D}), tok)
        plain = m.generate(tok, a.new)
        wrong = (plain + 1) % V
        LK = dict(prompt_lookup_num_tokens=D, max_matching_ngram_size=a.ngram, output_acceptance=True, eos_poll=a.eos_poll)
        runs = {"g": lambda t: m.generate(t, a.new), "l": lambda t: m.generate(t, a.new, **LK),
                "u": lambda t: m.generate(t, a.new, _draft_from=plain, **LK), "x": lambda t: m.generate(t, a.new, _draft_from=wrong, **LK)}
        best, steps, same = {}, {"g": a.new}, {}
        for k in a.only:
            if k != "g":                                        # (also the warm-up of the K-row step's packs and workspaces)
                out, acc = runs[k](tok)
                steps[k], same[k] = acc.shape[1], bool(torch.equal(out, plain))
        for rep in range(a.reps):                               # alternating, so that all see the same clocks
            for k in a.only:
                dt = timed_once(runs[k], tok, warm=rep == 0)
                best[k] = min(best.get(k, dt), dt)
        res = {"workload": f"KosmosLanguage prompt-lookup speculation, B={B}, D={D}, ngram {a.ngram}, prompt {T} (one block x 4), "
                           f"{a.new} new tokens, {a.precision}, greedy", "prefill_ms": round(pre * 1e3, 3)}
        names = {"g": "g_plain", "l": "l_lookup", "u": "u_all_right", "x": "x_all_wrong"}
        for k in a.only:
            # the first token comes from the prefill: new - 1 tokens over steps - 1 decode steps
            res[names[k] + "_ms_per_token"] = round((best[k] - pre) / (a.new - 1) * 1e3, 4)
            res[names[k] + "_tokens_per_step"] = round((a.new - 1) / max(steps[k] - 1, 1), 3)
            issued = steps[k] if k == "g" else min(a.new, -(-steps[k] // a.eos_poll) * a.eos_poll)   # up to the poll that ended the loop
            res[names[k] + "_ms_per_issued_step"] = round((best[k] - pre) / max(issued - 1, 1) * 1e3, 4)
            if k in same:
                res[names[k] + "_equals_plain"] = same[k]
        print(json.dumps(res), flush=True)


if a.prompt_lookup:
    with torch.no_grad():
        lookup_leg()
    sys.exit(0)
if a.num_beams:
    with torch.no_grad():
        beam_leg()
    sys.exit(0)
if constrained:
    with torch.no_grad():
        constraints_leg()
    sys.exit(0)

with torch.no_grad():
    for B in (int(b) for b in a.batches.split(",")):
        tok_all = torch.randint(0, V, (B, a.prefix + a.new), generator=torch.Generator().manual_seed(0)).to(dev)
        tok = tok_all[:, : a.prefix].contiguous()
        # every variant runs one prefill and new - 1 decode steps; the prefill is measured on its own and subtracted
        pre = timed(lambda t: m(t, incremental_state={"max_len": a.prefix + a.new}), tok)
        res = {"workload": f"KosmosLanguage generate, B={B}, prefix {a.prefix}, {a.new} new tokens, {a.precision}, "
                           "top_k=50 top_p=0.9 temperature=0.8", "prefill_ms": round(pre * 1e3, 3)}
        if a.ragged:
            res["lengths"] = lengths_of(B)
            if "a" in a.only:
                res["a_generate_uniform_ms_per_token"] = round((timed(run_a, tok) - pre) / (a.new - 1) * 1e3, 4)
            if "r" in a.only:
                dt = timed(run_r, tok)
                res["r_generate_ragged_ms_per_token"] = round((dt - pre) / (a.new - 1) * 1e3, 4)
                res["r_ragged_tokens_per_s"] = round(B * a.new / dt, 1)
            if "s" in a.only:
                res["s_solo_calls_tokens_per_s"] = round(B * a.new / timed(run_s, tok), 1)
        for name, fn, arg in (("a", run_a, tok), ("b", run_b, tok), ("c", run_c, tok_all)):
            if name in a.only and not a.ragged:
                res[{"a": "a_generate_fused_ms_per_token", "b": "b_torch_sampler_ms_per_token",
                     "c": "c_bare_decode_step_ms_per_token"}[name]] = round((timed(fn, arg) - pre) / (a.new - 1) * 1e3, 4)
        # launches per token, counted by the library's own per-launch records: generate(3 tokens) - generate(2 tokens) is one
        # decode step + its embedding + the sampler; the bare step is one more call of the public incremental path
        counts = []
        for n_new in (2, 3):
            _hip.prof_enable(True)
            m.generate(tok, n_new, **(dict(KW, prompt_lengths=lengths_of(B)) if a.ragged else KW))
            torch.cuda.synchronize()
            counts.append(len(_hip.prof_collect()))
        state = {"max_len": a.prefix + a.new}
        m(tok, incremental_state=state)
        torch.cuda.synchronize()
        _hip.prof_enable(True)
        m(tok_all[:, : a.prefix + 1], incremental_state=state)
        torch.cuda.synchronize()
        bare = len(_hip.prof_collect())
        _hip.prof_enable(False)
        res["launches_per_generated_token"], res["launches_per_bare_step"] = counts[1] - counts[0], bare
        print(json.dumps(res), flush=True)
