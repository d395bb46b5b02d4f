"""Device time of the sampler launch with the truncation filters, at the product's vocabulary (V = 64007): per (B, leg)
  min-p      ops.sample_logits(rows, temperature, top_k, top_p, min_p=0.05) — kx_sample_logits_min_p, the launch the filters extend,
             on the same rows in the same run: the baseline;
  typical    ... typical_p=0.9         — kx_sample_logits_truncate: 1 + 3 more passes over the row;
  epsilon    ... epsilon_cutoff=3e-4   — 1 more pass;
  eta        ... eta_cutoff=2e-3       — 1 more pass;
  all        the three together        — 1 + 3, 1, 1 more passes.
kernel_us is the device time of ONE launch (_hip.prof_collect(): the library's events around the launch), the best of --reps; the legs
alternate inside every repetition.  Rows are Gaussian logits at --scale, the same for every leg.  One JSON line per (B, leg); --check
also asserts that two calls of a leg draw the same tokens and that every token lies inside the leg's keep_mask."""
import argparse, json, os, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx import _hip as H
from kosmosx import ops

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,8")
ap.add_argument("--vocab", type=int, default=64007)
ap.add_argument("--scale", type=float, default=3.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--check", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
SAMPLE = dict(temperature=0.9, top_k=50, top_p=0.95, min_p=0.05, seed=1, position=7)
LEGS = [("min-p", {}), ("typical", dict(typical_p=0.9)), ("epsilon", dict(epsilon_cutoff=3e-4)), ("eta", dict(eta_cutoff=2e-3)),
        ("all", dict(typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3))]


def launch_us(rows, out, kw):
    H.prof_enable(True)
    ops.sample_logits(rows, out=out, **SAMPLE, **kw)
    torch.cuda.synchronize()
    recs = H.prof_collect()
    H.prof_enable(False)
    pick = [ms for kind, r, c, _, ms in recs if kind == "misc" and (r, c) == tuple(rows.shape)]
    assert len(pick) == 1, recs                                # one launch, with or without the filters
    return 1e3 * pick[0]


for B in (int(b) for b in a.batches.split(",")):
    rows = (torch.randn((B, a.vocab), generator=torch.Generator().manual_seed(B)) * a.scale).to(dev)
    out = torch.empty(B, dtype=torch.int64, device=dev)
    for _, kw in LEGS:                                         # warm-up: loads every code object
        ops.sample_logits(rows, out=out, **SAMPLE, **kw)
    best = {}
    for _ in range(a.reps):
        for name, kw in LEGS:                                  # alternating
            us = launch_us(rows, out, kw)
            best[name] = min(best.get(name, us), us)
    for name, kw in LEGS:
        tok, kept, mask = ops.sample_logits(rows, return_debug=True, **SAMPLE, **kw)
        rec = {"batch": B, "leg": name, "vocab": a.vocab, "scale": a.scale, "reps": a.reps, "kernel_us": round(best[name], 2),
               "over_min_p_us": round(best[name] - best["min-p"], 2), "kept_mean": round(float(kept.float().mean()), 1)}
        if a.check:
            again = ops.sample_logits(rows, **SAMPLE, **kw)
            rec["tokens_repeat"] = bool(torch.equal(tok, again))
            rec["token_in_mask"] = bool(mask.gather(1, tok[:, None]).bool().all())
            assert rec["tokens_repeat"] and rec["token_in_mask"], rec
        print(json.dumps(rec), flush=True)
