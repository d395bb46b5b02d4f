"""generate() with classifier-free guidance on the full-size text decoder (V = 64007): per (B, leg)
  off-B    KosmosLanguage.generate(x, N, do_sample, top_k, top_p) at B rows — the plain sampling loop with guidance_scale at its
           default: the launches of the tree before the feature, measured on the same box in the same run;
  off-2B   the same call at 2B rows (the prompts repeated): what the doubled batch alone costs;
  guided   B rows with guidance_scale=1.5 and a negative prompt of another length — 2B rows through the ragged step, one
           kx_guidance_logits launch per token in front of the sampler and one [B] token copy behind it.
ms per generated token (the call's wall time over N, prefill of --prefix tokens included in every leg alike, ended by a device
synchronise), the library's launches per step (_hip.prof_collect() of an untimed call at N and at N / 2: the slope) and kernel_us, the
mean device time of kx_guidance_logits from the profiler's records (its misc records carry the tag 33) or, in the off legs, of the
sampler launch.  The legs alternate, best of --reps each.  One JSON line per (B, leg); --check also compares every leg's tokens with a
second call (the draws repeat by seed) and the guided leg's with the plain ones (guidance changes them)."""
import argparse, json, os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx import _hip as H
from kosmosx.model import KosmosLanguage

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,4")
ap.add_argument("--prefix", type=int, default=16)
ap.add_argument("--negative", type=int, default=9)
ap.add_argument("--new-tokens", type=int, default=128)
ap.add_argument("--vocab", type=int, default=64007)
ap.add_argument("--precision", default="mixed")
ap.add_argument("--scale", type=float, default=1.5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--check", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
N = a.new_tokens
m = KosmosLanguage(vocab_size=a.vocab, dim=2048, _seed=0).eval().to(dev)
m.precision = a.precision

g = torch.Generator().manual_seed(0)
SAMPLE = dict(do_sample=True, temperature=0.9, top_k=50, top_p=0.95, seed=1)
GUIDANCE_TAG = 33                                             # the third word of kx_guidance_logits' profiler records


def run(leg, n):
    x, kw = leg
    return m.generate(x, n, **SAMPLE, **kw)


def timed(leg):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(leg, N)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def launches(leg, n, rows, tag):
    """(library launches of the call, mean device microseconds of its misc launches on [rows, V] rows with the given tag: 33 is the
    guidance launch, 0 the sampler)."""
    H.prof_enable(True)
    run(leg, n)
    torch.cuda.synchronize()
    recs = H.prof_collect()
    H.prof_enable(False)
    pick = [ms for kind, r, cols, c, ms in recs if kind == "misc" and (r, cols, c) == (rows, a.vocab, tag)]
    return len(recs), (round(1e3 * sum(pick) / len(pick), 2) if pick else None)


for B in (int(b) for b in a.batches.split(",")):
    x = torch.randint(2, a.vocab, (B, a.prefix), generator=g).to(dev)
    neg = torch.randint(2, a.vocab, (B, a.negative), generator=g).to(dev)
    legs = {"off-B": (x, {}), "off-2B": (x.repeat(2, 1), {}),
            "guided": (x, dict(guidance_scale=a.scale, negative_prompt_ids=neg))}
    best, outs = {}, {}
    for name, leg in legs.items():                            # warm-up: packs weights, sizes workspaces, loads every code object
        outs[name] = run(leg, N)
    for _ in range(a.reps):
        for name, leg in legs.items():                        # alternating
            ms, _ = timed(leg)
            best[name] = min(best.get(name, ms), ms)
    for name, leg in legs.items():
        guided = name == "guided"
        rows = B if name != "off-2B" else 2 * B               # the rows the sampler and the guidance launch see
        full, kernel_us = launches(leg, N, rows, GUIDANCE_TAG if guided else 0)
        rec = {"batch": B, "leg": name, "step_rows": 2 * B if name != "off-B" else B, "new_tokens": N, "prefix": a.prefix,
               "negative": a.negative if guided else None, "vocab": a.vocab, "precision": a.precision, "ms_per_token": round(best[name] / N, 4),
               "over_off_B_us_per_token": round(1e3 * (best[name] - best["off-B"]) / N, 2),
               "over_off_2B_us_per_token": round(1e3 * (best[name] - best["off-2B"]) / N, 2),
               "launches_per_step": (full - launches(leg, N // 2, rows, 0)[0]) / (N - N // 2),
               "kernel_us": kernel_us, "kernel": "kx_guidance_logits" if guided else "sampler"}
        if a.check:
            rec["tokens_repeat"] = bool(torch.equal(run(leg, N), outs[name]))
            if guided:
                rec["differs_from_off"] = not bool(torch.equal(outs[name], outs["off-B"]))
        print(json.dumps(rec), flush=True)
