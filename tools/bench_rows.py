"""Device time of the sampler launch with per-row options (kx_sample_logits_rows), at the product's vocabulary (V = 64007):
  equal      per B: the records of all rows equal — temperature, top-k, top-p, min-p, typical-p, epsilon and eta as below — against
             scalar, the kx_sample_logits_truncate launch of the SAME build with the same values on the same rows in the same run: the
             baseline (a comparison with an earlier build's library takes KOSMOSX_HIP_LIB and a second run of the scalar leg).  The two
             launches run the same passes; the rows launch adds one 56-byte uniform load per workgroup;
  mixed      per B: rows with unlike records (the six of MIXED, repeated) in ONE launch, against the sum of their one-row launches through
             the scalar entry point each record selects — what serving them separately costs the sampler.
kernel_us is the device time of ONE launch (_hip.prof_collect(): the library's events around the launch), the best of --reps; the legs
alternate inside every repetition.  Rows are Gaussian logits at --scale, the same for every leg.  One JSON line per (B, leg); --check
also asserts that the equal-records launch draws the scalar launch's tokens and the mixed launch its one-row launches' tokens."""
import argparse, json, os, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx import _hip as H
from kosmosx import ops

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,4,8")
ap.add_argument("--vocab", type=int, default=64007)
ap.add_argument("--scale", type=float, default=3.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--check", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
EQUAL = dict(do_sample=True, temperature=0.9, top_k=50, top_p=0.95, min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3, seed=1)
MIXED = [dict(do_sample=False), dict(do_sample=True, temperature=0.7), dict(do_sample=True, temperature=1.0, top_k=50, top_p=0.9, seed=3),
         dict(do_sample=True, temperature=1.1, min_p=0.05, typical_p=0.9, seed=4), dict(do_sample=True, temperature=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3),
         EQUAL]
POSITION = 7


def launch_us(logits, out, **kw):
    H.prof_enable(True)
    ops.sample_logits(logits, out=out, position=POSITION, **kw)
    torch.cuda.synchronize()
    recs = H.prof_collect()
    H.prof_enable(False)
    pick = [ms for kind, r, c, _, ms in recs if kind == "misc" and (r, c) == tuple(logits.shape)]
    assert len(pick) == 1, recs                                # one launch
    return 1e3 * pick[0]


for B in (int(b) for b in a.batches.split(",")):
    rows = (torch.randn((B, a.vocab), generator=torch.Generator().manual_seed(B)) * a.scale).to(dev)
    out, seq = torch.empty(B, dtype=torch.int64, device=dev), torch.arange(B, dtype=torch.int64, device=dev)
    one, ones = torch.empty(1, dtype=torch.int64, device=dev), [rows[b:b + 1].contiguous() for b in range(B)]
    mixed = [MIXED[b % len(MIXED)] for b in range(B)]
    equal_table, mixed_table = ops.SampleRowTable([EQUAL] * B, a.vocab, dev), ops.SampleRowTable(mixed, a.vocab, dev)
    legs = {"scalar": lambda: launch_us(rows, out, sequence_ids=seq, **EQUAL),
            "equal": lambda: launch_us(rows, out, sequence_ids=seq, rows=equal_table),
            "one-row sum": lambda: sum(launch_us(ones[b], one, sequence_ids=seq[b:b + 1], **mixed[b]) for b in range(B)),
            "mixed": lambda: launch_us(rows, out, sequence_ids=seq, rows=mixed_table)}
    for fn in legs.values():                                   # warm-up: loads every code object
        fn()
    best = {}
    for _ in range(a.reps):
        for name, fn in legs.items():                          # alternating
            us = fn()
            best[name] = min(best.get(name, us), us)
    if a.check:
        want = ops.sample_logits(rows, position=POSITION, sequence_ids=seq, **EQUAL)
        assert torch.equal(want, ops.sample_logits(rows, position=POSITION, sequence_ids=seq, rows=equal_table))
        got = ops.sample_logits(rows, position=POSITION, sequence_ids=seq, rows=mixed_table)
        for b in range(B):
            assert torch.equal(got[b:b + 1], ops.sample_logits(ones[b], position=POSITION, sequence_ids=seq[b:b + 1], **mixed[b])), b
    for name, base in (("scalar", "scalar"), ("equal", "scalar"), ("one-row sum", "one-row sum"), ("mixed", "one-row sum")):
        print(json.dumps({"batch": B, "leg": name, "vocab": a.vocab, "scale": a.scale, "reps": a.reps, "kernel_us": round(best[name], 2),
                          "against": base, "ratio": round(best[name] / best[base], 4), "checked": bool(a.check)}), flush=True)
