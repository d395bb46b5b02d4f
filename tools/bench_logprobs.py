"""generate() with per-token log-probs on the full-size text decoder (V = 64007): per (B, leg)
  off     KosmosLanguage.generate(x, N) — the default path: the launches of the tree before the feature;
  k = 0 / 5 / 16   generate(x, N, output_logprobs=True, top_logprobs=k) — one kx_step_logprobs launch per step;
  today-k what a caller did before, on the same tree: generate(x, N, output_logits=True) — every [B, V] fp32 row kept — then
          torch.log_softmax, a gather at the tokens and torch.topk(k) over the [B, N, V] block.
ms per generated token (the call's wall time over N, prefill of --prefix tokens included in every leg alike), peak device memory of
the call above what the model holds, and the library's launches per step (_hip.prof_collect() of an untimed call at N and at N / 2:
the slope).  The legs alternate, best of --reps each.  One JSON line per (B, leg); --check also compares the legs' numbers."""
import argparse, json, os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx import _hip as H
from kosmosx.model import KosmosLanguage

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,4,16")
ap.add_argument("--top", default="0,5,16")
ap.add_argument("--prefix", type=int, default=16)
ap.add_argument("--new-tokens", type=int, default=128)
ap.add_argument("--vocab", type=int, default=64007)
ap.add_argument("--precision", default="mixed")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-today", action="store_true")
ap.add_argument("--check", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
N = a.new_tokens
m = KosmosLanguage(vocab_size=a.vocab, dim=2048, _seed=0).eval().to(dev)
m.precision = a.precision


def leg_off(x, n):
    return (m.generate(x, n),)


def leg_on(k):
    return lambda x, n: m.generate(x, n, output_logprobs=True, top_logprobs=k)


def leg_today(k):
    def run(x, n):
        tokens, logits = m.generate(x, n, output_logits=True)
        lsm = torch.log_softmax(logits, -1)
        out = (tokens, lsm.gather(2, tokens[:, :, None])[:, :, 0])
        if k:
            top = torch.topk(lsm, k, dim=-1)
            out += (top.values, top.indices)
        return out
    return run


def timed(fn, x):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn(x, N)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out


def launches(fn, x, n):
    H.prof_enable(True)
    fn(x, n)
    torch.cuda.synchronize()
    r = len(H.prof_collect())
    H.prof_enable(False)
    return r


g = torch.Generator().manual_seed(0)
tops = [int(k) for k in a.top.split(",")]
for B in (int(b) for b in a.batches.split(",")):
    x = torch.randint(0, a.vocab, (B, a.prefix), generator=g).to(dev)
    legs = [("off", leg_off)] + [(str(k), leg_on(k)) for k in tops]
    if not a.no_today:
        legs += [(f"today-{k}", leg_today(k)) for k in tops]
    best, peak, outs = {}, {}, {}
    for name, f in legs:                                      # warm-up: packs weights, sizes workspaces
        outs[name] = f(x, N)
    for _ in range(a.reps):
        for name, f in legs:                                  # alternating
            ms, mib, _ = timed(f, x)
            best[name] = min(best.get(name, ms), ms)
            peak[name] = mib
    for name, f in legs:
        rec = {"batch": B, "leg": name, "new_tokens": N, "prefix": a.prefix, "vocab": a.vocab, "precision": a.precision,
               "ms_per_token": round(best[name] / N, 4), "over_off_pct": round(100 * (best[name] / best["off"] - 1), 2),
               "peak_mib": round(peak[name], 1),
               "launches_per_step": (launches(f, x, N) - launches(f, x, N // 2)) / (N - N // 2)}
        if a.check and name != "off":
            ref = outs.get("today-" + name)
            rec["tokens_equal_off"] = bool(torch.equal(outs[name][0], outs["off"][0]))
            if ref is not None:                               # the kernel against torch on the kept rows
                rec["max_abs_diff_vs_torch"] = max(float((p.float() - q.float()).abs().max()) for p, q in zip(outs[name][1:3], ref[1:3]))
                if len(ref) == 4:
                    rec["top_ids_equal_torch"] = bool(torch.equal(outs[name][3], ref[3]))
        print(json.dumps(rec), flush=True)
