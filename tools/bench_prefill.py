"""Chunked prefill and extend() on the full-size text decoder (KosmosLanguage, the reference's 64007-token vocabulary).

  (a) generate(max_new_tokens=1) at B in --batches and T in --lengths with prefill_chunk in --chunks ("none" = one piece): ms per
      call, the legs alternating, best of --reps; and the peak device memory of one call above what was allocated before it
      (torch.cuda.max_memory_allocated after reset_peak_memory_stats, the decoder's grow-only workspace dropped first so that
      every leg pays for its own).  T = 2045, not 2046: generate()'s budget check is conservative by one position.
  (b) appending Tn in --append known tokens to a cache of P in --cached rows (B = --append-batch), three ways on the same state:
      extend() (one pass, with logits); Tn single-token steps; a fresh prefill of the P + Tn tokens.  The state is rewound
      between legs by resetting state["len"] (rows at and after it are rewritten by whoever runs next).

One JSON line per configuration.  --legs a|b|ab."""
import argparse, json, os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx.model import KosmosLanguage

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,8")
ap.add_argument("--lengths", default="512,2045")
ap.add_argument("--chunks", default="none,128,256,512")
ap.add_argument("--cached", default="128,1024")
ap.add_argument("--append", default="16,64,256")
ap.add_argument("--append-batch", type=int, default=1)
ap.add_argument("--precision", default="mixed")
ap.add_argument("--vocab", type=int, default=64007)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--legs", default="ab")
a = ap.parse_args()
dev = torch.device("cuda", 0)
V = a.vocab
m = KosmosLanguage(vocab_size=V, dim=2048, _seed=0).eval().to(dev)
m.precision = a.precision
g = torch.Generator().manual_seed(0)


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


if "a" in a.legs:
    chunks = [None if c == "none" else int(c) for c in a.chunks.split(",")]
    for B in (int(x) for x in a.batches.split(",")):
        for T in (int(x) for x in a.lengths.split(",")):
            tok = torch.randint(0, V, (B, T), generator=g).to(dev)
            legs = {("none" if c is None else str(c)): (lambda c=c: m.generate(tok, 1, prefill_chunk=c)) for c in chunks}
            outs = {k: f() for k, f in legs.items()}                     # warm-up: packs weights, loads code objects
            mem = {k: peak_mb(f) for k, f in legs.items()}
            for f in legs.values():
                f()                                                     # the workspace back at its largest before the timed window
            best = {}
            for _ in range(a.reps):
                for k, f in legs.items():                               # alternating
                    ms, _ = timed(f)
                    best[k] = min(best.get(k, ms), ms)
            print(json.dumps({"leg": "a", "batch": B, "prompt": T, "precision": a.precision, "vocab": V,
                              "ms": {k: round(v, 2) for k, v in best.items()}, "peak_mb": {k: round(v, 1) for k, v in mem.items()},
                              "same_token_as_one_piece": {k: bool(torch.equal(o, outs["none"])) for k, o in outs.items()} if "none" in outs else None}),
                  flush=True)

if "b" in a.legs:
    B = a.append_batch
    for P in (int(x) for x in a.cached.split(",")):
        for Tn in (int(x) for x in a.append.split(",")):
            tok = torch.randint(0, V, (B, P + Tn), generator=g).to(dev)
            state = {"max_len": P + Tn}
            with torch.no_grad():
                m(tok[:, :P], incremental_state=state)

            def run_extend():
                state["len"] = P
                with torch.no_grad():
                    return m.extend(tok[:, P:], state)[:, -1]

            def run_steps():
                state["len"] = P
                with torch.no_grad():
                    for t in range(P, P + Tn):
                        out = m(tok[:, :t + 1], incremental_state=state)
                return out[:, -1]

            def run_prefill():
                with torch.no_grad():
                    return m(tok, incremental_state={"max_len": P + Tn})[:, -1]

            legs = {"extend": run_extend, "steps": run_steps, "prefill": run_prefill}
            outs = {k: f() for k, f in legs.items()}
            best = {}
            for _ in range(a.reps):
                for k, f in legs.items():
                    ms, _ = timed(f)
                    best[k] = min(best.get(k, ms), ms)
            rms = float(outs["prefill"].pow(2).mean().sqrt())
            print(json.dumps({"leg": "b", "batch": B, "cached": P, "appended": Tn, "precision": a.precision, "vocab": V,
                              "ms": {k: round(v, 2) for k, v in best.items()},
                              "last_row_vs_prefill": {k: float((outs[k] - outs["prefill"]).abs().max()) / rms for k in ("extend", "steps")}}),
                  flush=True)
