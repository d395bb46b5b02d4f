"""generate() with the logit-shaping keywords on the full-size text decoder (V = 64007): per (B, leg)
  off        KosmosLanguage.generate(x, N, do_sample, top_k, top_p) — the plain sampling loop with the four keywords at their
             defaults: the launches of the tree before the feature, measured on the same box in the same run;
  bias       ... logit_bias={16 ids: values, one of them -inf} — one kx_shape_logits launch per step that edits 16 logits a row;
  penalties  ... frequency_penalty=0.5, presence_penalty=0.5 — the same launch reading the int32 [B, V] counts (V * 4 bytes a row);
  all        bias and penalties in the one launch;
  min-p      ... min_p=0.05 — no further launch: kx_sample_logits_min_p in place of kx_sample_logits.
ms per generated token (the call's wall time over N, prefill of --prefix tokens included in every leg alike, ended by a device
synchronise), the library's launches per step (_hip.prof_collect() of an untimed call at N and at N / 2: the slope) and kernel_us, the
mean device time of the leg's row-editing launch (kx_shape_logits: the profiler's records of B rows x V columns with 4-byte elements) or, in
the min-p and off legs, of the sampler launch.  The legs alternate, best of --reps each.  One JSON line per (B, leg); --check also
compares every leg's tokens with a second call (the draws repeat by seed) and the bias leg's with the banned id."""
import argparse, json, os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx import _hip as H
from kosmosx.model import KosmosLanguage

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,8")
ap.add_argument("--prefix", type=int, default=16)
ap.add_argument("--new-tokens", type=int, default=128)
ap.add_argument("--vocab", type=int, default=64007)
ap.add_argument("--precision", default="mixed")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--check", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
N = a.new_tokens
m = KosmosLanguage(vocab_size=a.vocab, dim=2048, _seed=0).eval().to(dev)
m.precision = a.precision

g = torch.Generator().manual_seed(0)
ids = sorted(set(torch.randint(2, a.vocab, (64,), generator=g).tolist()))[:16]
BIAS = {i: float(v) for i, v in zip(ids, torch.linspace(-4, 4, len(ids)).tolist())}
BANNED = ids[0]
BIAS[BANNED] = float("-inf")
SAMPLE = dict(do_sample=True, temperature=0.9, top_k=50, top_p=0.95, seed=1)
PEN = dict(frequency_penalty=0.5, presence_penalty=0.5)

LEGS = [("off", {}), ("bias", dict(logit_bias=BIAS)), ("penalties", PEN), ("all", dict(PEN, logit_bias=BIAS)), ("min-p", dict(min_p=0.05))]


def run(kw, x, n):
    return m.generate(x, n, **SAMPLE, **kw)


def timed(kw, x):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(kw, x, N)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def launches(kw, x, n, shaped):
    """(library launches of the call, mean device microseconds of its misc launches on [B, V] rows: the 4-byte records are the
    row-editing launch, the 0-byte ones the sampler)."""
    H.prof_enable(True)
    run(kw, x, n)
    torch.cuda.synchronize()
    recs = H.prof_collect()
    H.prof_enable(False)
    pick = [ms for kind, rows, cols, c, ms in recs if kind == "misc" and (rows, cols, c) == (x.shape[0], a.vocab, 4 if shaped else 0)]
    return len(recs), (round(1e3 * sum(pick) / len(pick), 2) if pick else None)


for B in (int(b) for b in a.batches.split(",")):
    x = torch.randint(0, a.vocab, (B, a.prefix), generator=g).to(dev)
    best, outs = {}, {}
    for name, kw in LEGS:                                     # warm-up: packs weights, sizes workspaces, loads every code object
        outs[name] = run(kw, x, N)
    for _ in range(a.reps):
        for name, kw in LEGS:                                 # alternating
            ms, _ = timed(kw, x)
            best[name] = min(best.get(name, ms), ms)
    for name, kw in LEGS:
        shaped = name in ("bias", "penalties", "all")
        rec = {"batch": B, "leg": name, "new_tokens": N, "prefix": a.prefix, "vocab": a.vocab, "precision": a.precision,
               "ms_per_token": round(best[name] / N, 4), "over_off_us_per_token": round(1e3 * (best[name] - best["off"]) / N, 2),
               "launches_per_step": (launches(kw, x, N, shaped)[0] - launches(kw, x, N // 2, shaped)[0]) / (N - N // 2),
               "kernel_us": launches(kw, x, N, shaped)[1], "kernel": "kx_shape_logits" if shaped else "sampler"}
        if a.check:
            rec["tokens_repeat"] = bool(torch.equal(run(kw, x, N), outs[name]))
            if name in ("bias", "all"):
                rec["banned_id_absent"] = not bool((outs[name] == BANNED).any())
        print(json.dumps(rec), flush=True)
