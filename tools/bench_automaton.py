"""generate() under a token automaton on the full-size text decoder (V = 64007): per (B, leg)
  off      KosmosLanguage.generate(x, N) — the default path: the launches of the tree before the feature;
  badword  generate(x, N, bad_words_ids=[[0]]) — one kx_constrain_logits launch per step: the yardstick for one more launch;
  free     generate(x, N, token_automaton=<one state that allows everything>) — one kx_automaton_step launch per step that stores
           nothing: the launch's floor (plus the stop poll every 8 steps, which an automaton turns on);
  sparse   generate(x, N, token_automaton=TokenAutomaton.from_allowed(16 ids)) — every step stores the whole row (V * 4 bytes per row);
  free-nopoll / sparse-nopoll   the same two with eos_poll=0: what the stop poll's device-to-host read every 8 steps costs;
  today    what a caller did before, on the same tree: the raw incremental protocol, a torch mask on the [B, V] row and argmax, the
           token read back to the host and fed from there.
ms per generated token (the call's wall time over N, prefill of --prefix tokens included in every leg alike), the library's
launches per step (_hip.prof_collect() of an untimed call at N and at N / 2: the slope) and kernel_us, the mean device time of the
leg's row-editing launch (kx_constrain_logits / kx_automaton_step: the profiler's records of B rows x V columns).  The legs alternate, best of --reps each.
One JSON line per (B, leg); --check also compares sparse with today (the same greedy tokens) and free with off."""
import argparse, json, os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx import _hip as H
from kosmosx.automaton import TokenAutomaton
from kosmosx.model import KosmosLanguage

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,8")
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

g = torch.Generator().manual_seed(0)
allowed = sorted(set(torch.randint(2, a.vocab, (64,), generator=g).tolist()))[:16]
FREE = TokenAutomaton([{}], default=[0])
SPARSE = TokenAutomaton.from_allowed(allowed)
ban = torch.ones(a.vocab, dtype=torch.bool)
ban[allowed] = False
ban = ban.to(dev)


def leg_today(x, n):
    state, seq, toks = {}, x, []
    with torch.no_grad():
        out = m(seq, incremental_state=state)
        for i in range(n):
            nxt = out[:, -1].masked_fill(ban, float("-inf")).argmax(-1).tolist()        # the pick leaves the device
            toks.append(nxt)
            seq = torch.cat([seq, torch.tensor(nxt, dtype=torch.int64, device=dev)[:, None]], 1)
            if i + 1 < n:
                out = m(seq, incremental_state=state)
    return torch.tensor(toks, dtype=torch.int64, device=dev).t().contiguous()


LEGS = [("off", lambda x, n: m.generate(x, n)), ("badword", lambda x, n: m.generate(x, n, bad_words_ids=[[0]])),
        ("free", lambda x, n: m.generate(x, n, token_automaton=FREE)), ("sparse", lambda x, n: m.generate(x, n, token_automaton=SPARSE)),
        ("free-nopoll", lambda x, n: m.generate(x, n, token_automaton=FREE, eos_poll=0)),
        ("sparse-nopoll", lambda x, n: m.generate(x, n, token_automaton=SPARSE, eos_poll=0))]
if not a.no_today:
    LEGS.append(("today", leg_today))


def timed(fn, x):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(x, N)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def launches(fn, x, n):
    """(library launches of the call, mean device microseconds of its misc launches on [B, V] rows with 4-byte elements or None)."""
    H.prof_enable(True)
    fn(x, n)
    torch.cuda.synchronize()
    recs = H.prof_collect()
    H.prof_enable(False)
    edit = [ms for kind, rows, cols, c, ms in recs if kind == "misc" and (rows, cols, c) == (x.shape[0], a.vocab, 4)]
    return len(recs), (round(1e3 * sum(edit) / len(edit), 2) if edit else None)


for B in (int(b) for b in a.batches.split(",")):
    x = torch.randint(0, a.vocab, (B, a.prefix), generator=g).to(dev)
    best, outs = {}, {}
    for name, f in LEGS:                                      # warm-up: packs weights, sizes workspaces
        outs[name] = f(x, N)
    for _ in range(a.reps):
        for name, f in LEGS:                                  # alternating
            ms, _ = timed(f, x)
            best[name] = min(best.get(name, ms), ms)
    for name, f in LEGS:
        rec = {"batch": B, "leg": name, "new_tokens": N, "prefix": a.prefix, "vocab": a.vocab, "precision": a.precision,
               "ms_per_token": round(best[name] / N, 4), "over_off_us_per_token": round(1e3 * (best[name] - best["off"]) / N, 2),
               "launches_per_step": (launches(f, x, N)[0] - launches(f, x, N // 2)[0]) / (N - N // 2), "kernel_us": launches(f, x, N)[1]}
        if a.check:
            if name == "free":
                rec["tokens_equal_off"] = bool(torch.equal(outs["free"], outs["off"]))
            if name == "sparse":
                rec["tokens_allowed"] = bool(torch.isin(outs["sparse"], torch.tensor(allowed, device=dev)).all())
                if "today" in outs:
                    rec["tokens_equal_today"] = bool(torch.equal(outs["sparse"], outs["today"]))
        print(json.dumps(rec), flush=True)
