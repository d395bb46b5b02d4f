"""score() on the full-size text decoder: ms per call of
  (s) KosmosLanguage.score(prompt, continuations) — one prefill of the prompt, one K-row step over the C * (L - 1) candidate rows,
      the log-probs taken by kx_token_logprob;
  (f) what a caller did before score() existed, on the same tree: model(cat(prompt, continuation)) over the C sequences — the
      prompt run C times, [C, T, V] fp32 logits written — then torch log_softmax and gather on the continuation's rows.
One prompt of --prefix tokens, C in --candidates, L in --lengths; the legs alternate, best of --reps each.  One JSON line per
(C, L).  --only s|f restricts the run to one leg (for a kernel trace of that leg alone)."""
import argparse, json, os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx.model import KosmosLanguage

ap = argparse.ArgumentParser()
ap.add_argument("--candidates", default="4,16,64")
ap.add_argument("--lengths", default="1,4,16")
ap.add_argument("--prefix", type=int, default=112)
ap.add_argument("--precision", default="mixed")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default="sf")
a = ap.parse_args()
dev = torch.device("cuda", 0)
V = 32002
m = KosmosLanguage(vocab_size=V, dim=2048, _seed=0).eval().to(dev)
m.precision = a.precision


def run_s(prompt, cont):
    return m.score(prompt, cont)


def run_f(prompt, cont):
    C, L = cont.shape
    full = torch.cat([prompt.expand(C, -1), cont], 1)
    rows = m(full)[:, a.prefix - 1:a.prefix - 1 + L]
    return torch.log_softmax(rows, -1).gather(2, cont[:, :, None])[:, :, 0]


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


g = torch.Generator().manual_seed(0)
prompt = torch.randint(0, V, (1, a.prefix), generator=g).to(dev)
for C in (int(x) for x in a.candidates.split(",")):
    for L in (int(x) for x in a.lengths.split(",")):
        cont = torch.randint(0, V, (C, L), generator=g).to(dev)
        legs = [(k, f) for k, f in (("s", run_s), ("f", run_f)) if k in a.only]
        best, outs = {}, {}
        for k, f in legs:                                     # warm-up: packs weights, sizes workspaces
            outs[k] = f(prompt, cont)
        for _ in range(a.reps):
            for k, f in legs:                                 # alternating
                ms, _ = timed(f, prompt, cont)
                best[k] = min(best.get(k, ms), ms)
        rec = {"candidates": C, "length": L, "prefix": a.prefix, "precision": a.precision, "step_rows": C * (L - 1)}
        if "s" in best:
            rec["score_ms"] = round(best["s"], 3)
        if "f" in best:
            rec["forward_logsoftmax_ms"] = round(best["f"], 3)
        if len(best) == 2:
            rec["speedup"] = round(best["f"] / best["s"], 2)
            rec["max_abs_diff"] = float((outs["s"] - outs["f"]).abs().max())
        print(json.dumps(rec), flush=True)
