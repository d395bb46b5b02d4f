"""n sampled continuations per prompt over one shared prompt KV cache against the prompt repeated n times, on the full-size text
decoder (KosmosLanguage, the reference's 64007-token vocabulary).

For every (B, n) in --configs, a prompt of --prompt tokens and --new new tokens:
  (1) "shared":   generate(tok, do_sample=True, num_return_sequences=n) — one prefill at B rows, B * n samples over it, each with a
                  private tail cache of --new rows (kx_decoder_decode_step_prefix);
  (2) "repeated": generate(tok.repeat_interleave(n, 0), do_sample=True) — B * n prefills and B * n private caches, the uniform step
                  (one host position for every row);
  (3) "repeated_ragged": (2) with prompt_lengths = the full width for every row — the same tokens through the ragged step, the one
                  (1) is built from (device positions, kx_step_prepare): what separates the prefix form's own cost from the ragged
                  step's.
The legs alternate in one process; every call ends in a device synchronise.  Per leg: ms per call (best, median and worst of
--reps: the spread to hold a difference against), ms per decode step — (call at --new tokens - call at 1 token) / (--new - 1), best
against best: a call at 1 token is the prefill and one sampler launch, no step — and the peak device memory of one call above what was
allocated before it, as tools/bench_prefill.py measures it (torch.cuda.max_memory_allocated).

One JSON line per configuration."""
import argparse, json, os, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx.model import KosmosLanguage

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="1x4,1x8,1x16,2x8", help="B x n, comma separated")
ap.add_argument("--prompt", type=int, default=1024)
ap.add_argument("--new", type=int, default=32)
ap.add_argument("--precision", default="mixed")
ap.add_argument("--vocab", type=int, default=64007)
ap.add_argument("--dim", type=int, default=2048)
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_parallel: no GPU — a time measured anywhere else says nothing about the MI355X")
if a.new < 2:
    sys.exit("bench_parallel: --new must be at least 2 (the step time is a difference of two call times)")
dev = torch.device("cuda", 0)
V = a.vocab
m = KosmosLanguage(vocab_size=V, dim=a.dim, _seed=0).eval().to(dev)
m.precision = a.precision
g = torch.Generator().manual_seed(0)
SAMPLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.95, seed=1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_mb(fn):
    """Peak device memory of one call above what was allocated before it, the workspace re-grown inside the call."""
    m.decoder._ws.bufs.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20


def measure(legs):
    outs = {k: f() for k, f in legs.items()}                                # warm-up: packs weights, loads code objects
    ms = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, f in legs.items():                                           # alternating
            ms[k].append(timed(f)[0])
    return outs, ms


for cfg in a.configs.split(","):
    B, n = (int(x) for x in cfg.split("x"))
    tok = torch.randint(0, V, (B, a.prompt), generator=g).to(dev)
    rep = tok.repeat_interleave(n, dim=0)
    legs = {"shared": lambda N=a.new: m.generate(tok, N, num_return_sequences=n, **SAMPLE),
            "repeated": lambda N=a.new: m.generate(rep, N, **SAMPLE),
            "repeated_ragged": lambda N=a.new: m.generate(rep, N, prompt_lengths=[a.prompt] * (B * n), **SAMPLE)}
    one = {k: (lambda f=f: f(1)) for k, f in legs.items()}
    outs, full = measure(legs)
    _, first = measure(one)
    mem = {k: round(peak_mb(f), 1) for k, f in legs.items()}
    stat = lambda v: {"best": round(min(v), 2), "median": round(statistics.median(v), 2), "worst": round(max(v), 2)}
    print(json.dumps({"batch": B, "samples": n, "rows": B * n, "prompt": a.prompt, "new": a.new, "precision": a.precision, "vocab": V,
                      "reps": a.reps, "ms_per_call": {k: stat(v) for k, v in full.items()},
                      "ms_prefill_and_first_token": {k: stat(v) for k, v in first.items()},
                      "ms_per_step": {k: round((min(full[k]) - min(first[k])) / (a.new - 1), 4) for k in legs},
                      "ms_per_step_median": {k: round((statistics.median(full[k]) - statistics.median(first[k])) / (a.new - 1), 4)
                                             for k in legs},
                      "peak_mb": mem, "same_tokens": all(bool(torch.equal(outs["shared"], outs[k])) for k in legs)}), flush=True)
