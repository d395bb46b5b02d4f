"""A session turn against re-prefilling the conversation, on the full-size text decoder (KosmosLanguage, the reference's
64007-token vocabulary).

For B in --batches and a first turn that leaves about C in --cached rows in the cache (a prompt of C - --new tokens, --new
generated), the second turn brings --turn new tokens and generates --new:
  (1) Session.generate on the kept cache (the session is rewound between repetitions: its host bookkeeping is restored, the cache
      rows at and after a row's valid length are rewritten by whoever runs next);
  (2) a fresh generate() over the concatenated prompt (first prompt, first output, the new tokens).
The two legs alternate in one process, best of --reps; peak device memory of one call above what was allocated before it, as
tools/bench_prefill.py measures it.
  (3) at B = 1, where both apply: the block's append alone, through extend() (kx_decoder_extend, host P) and through
      Decoder._extend_ragged (kx_decoder_extend_ragged, device positions), on the same state, with logits.

One JSON line per configuration.  --legs 12|3|123."""
import argparse, copy, json, os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx.model import KosmosLanguage

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,4")
ap.add_argument("--cached", default="512,1024")
ap.add_argument("--turn", type=int, default=32)
ap.add_argument("--new", type=int, default=32)
ap.add_argument("--precision", default="mixed")
ap.add_argument("--vocab", type=int, default=64007)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--legs", default="123")
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


def best_of(legs):
    outs = {k: f() for k, f in legs.items()}                                # warm-up: packs weights, loads code objects
    best = {}
    for _ in range(a.reps):
        for k, f in legs.items():                                           # alternating
            ms, _ = timed(f)
            best[k] = min(best.get(k, ms), ms)
    return outs, {k: round(v, 2) for k, v in best.items()}


if "1" in a.legs or "2" in a.legs:
    for B in (int(x) for x in a.batches.split(",")):
        for C in (int(x) for x in a.cached.split(",")):
            T0 = C - a.new
            tok = torch.randint(0, V, (B, T0), generator=g).to(dev)
            x2 = torch.randint(0, V, (B, a.turn), generator=g).to(dev)
            out1, sess = m.generate(tok, a.new, return_session=True, session_capacity=C + a.turn + a.new + 1)
            snap = {k: copy.copy(getattr(sess, k)) for k in ("lengths", "_cached", "_text", "_pending")}
            cat = torch.cat([tok, out1, x2], 1)

            def run_session():
                for k, v in snap.items():                                   # rewind
                    setattr(sess, k, copy.copy(v))
                return sess.generate(x2, a.new)

            def run_fresh():
                return m.generate(cat, a.new)

            legs = {"session": run_session, "fresh": run_fresh}
            outs, ms = best_of(legs)
            mem = {k: round(peak_mb(f), 1) for k, f in legs.items()}
            print(json.dumps({"leg": "12", "batch": B, "cached": snap["_cached"][0], "turn": a.turn,
                              "new": a.new, "precision": a.precision, "vocab": V, "ms": ms, "peak_mb": mem,
                              "same_tokens": bool(torch.equal(outs["session"], outs["fresh"]))}), flush=True)
            del sess, snap

if "3" in a.legs:
    for C in (int(x) for x in a.cached.split(",")):
        P, Tn = C, a.turn + 1                                               # the pending token and the new ones
        tok = torch.randint(0, V, (1, P + Tn), generator=g).to(dev)
        state = {"max_len": P + Tn}
        with torch.no_grad():
            m(tok[:, :P], incremental_state=state)
        pos = torch.full((1,), P, dtype=torch.int32, device=dev)
        block = tok[:, P:].contiguous()

        def run_uniform():
            state.pop("positions", None)
            state["len"] = P
            with torch.no_grad():
                return m.extend(block, state)[:, -1]

        def run_ragged():
            state.update(positions=pos, pos_max=P)
            with torch.no_grad():
                return m.decoder._extend_ragged(block, state, pos, m.precision)[:, -1]

        outs, ms = best_of({"uniform": run_uniform, "ragged": run_ragged})
        state.pop("positions", None)
        print(json.dumps({"leg": "3", "batch": 1, "cached": P, "appended": Tn, "precision": a.precision, "vocab": V, "ms": ms,
                          "same_bits": bool(torch.equal(outs["uniform"], outs["ragged"]))}), flush=True)
