"""Contrastive search (generate(penalty_alpha=, top_k=k)): what its launches cost, at the product's sizes (V = 64007, D = 2048).

  launches   per (B, k, P): the device time of each launch the loop adds beside the decode step — kx_contrast_candidates (the
             sequence's logits row, addressed through the row index), kx_contrast_hidden (M = B * k rows), kx_contrast_select's two
             launches (the partial maxima over P history rows, then the choice) and kx_kv_cache_commit (24 layers, 32 heads, fp32
             caches) — on synthetic buffers of the right shapes.  kernel_us is the device time of ONE launch (_hip.prof_collect(): the
             library's events around the launch), the best of --reps.
  generate   per (B, k): ms per generated token of generate(penalty_alpha=0.6, top_k=k) against greedy generate() of the same build,
             the same model (the full-size text decoder, KosmosLanguage) and the same prompt of --prompt tokens in the same run, the
             legs alternating; ms per token = (call at --new tokens - call at 1 token) / (--new - 1), best against best of --reps.
             A greedy call at 1 token is the prefill and one sampler launch; a contrastive call at 1 token also runs one step at
             B * k rows, so the difference holds --new - 1 further steps in both.
One JSON line per measurement.  --check also asserts what the launches computed: the candidates against ops.step_logprobs, the choice
against a float64 restatement on the host, the committed rows against torch indexing.  --skip-generate: the launches only."""
import argparse, ctypes, json, os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kosmos-x_amd")]
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")
import torch
from kosmosx import _hip as H
from kosmosx import ops

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,4")
ap.add_argument("--candidates", default="4,8")
ap.add_argument("--history", default="128,2048")
ap.add_argument("--vocab", type=int, default=64007)
ap.add_argument("--dim", type=int, default=2048)
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--prompt", type=int, default=128)
ap.add_argument("--new", type=int, default=17)
ap.add_argument("--precision", default="mixed")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--check", action="store_true")
ap.add_argument("--skip-generate", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_contrast: no GPU — a time measured anywhere else says nothing about the MI355X")
dev = torch.device("cuda", 0)
V, D, L, NH = a.vocab, a.dim, a.layers, a.dim // 64
ALPHA = 0.6


def best_us(fn, pick):
    """Best device time over --reps of the launches ``fn`` issues, per profiler record that ``pick`` names (a dict name -> us)."""
    best = {}
    for _ in range(a.reps + 1):                                # (the first repetition loads the code objects)
        H.prof_enable(True)
        fn()
        torch.cuda.synchronize()
        recs = H.prof_collect()
        H.prof_enable(False)
        names = pick(recs)
        for name, ms in names.items():
            best[name] = min(best.get(name, 1e9), 1e3 * ms)
    return best


for B in (int(x) for x in a.batches.split(",")):
    for k in (int(x) for x in a.candidates.split(",")):
        for P in (int(x) for x in a.history.split(",")):
            M, cap = B * k, P + 2
            g = torch.Generator().manual_seed(B * 100 + k)
            logits = (torch.randn((M, V), generator=g) * 3.0).to(dev)
            hist = torch.nn.functional.normalize(torch.randn((B, cap, D), generator=g), dim=-1).to(dev)
            x = torch.randn((M, 1, D), generator=g).to(dev)
            gam, bet = torch.ones(D, device=dev), torch.zeros(D, device=dev)
            w = H.DecoderWeights()
            w.struct_bytes, w.layer_bytes = ctypes.sizeof(H.DecoderWeights), ctypes.sizeof(H.DecoderLayer)
            w.dim, w.eps, w.ln_g, w.ln_b = D, 1e-5, gam.data_ptr(), bet.data_ptr()
            chosen_prev = torch.randint(0, k, (B,), generator=g).to(torch.int32).to(dev)
            st, pr = torch.zeros(M, dtype=torch.int64, device=dev), torch.zeros(M, device=dev)
            u = torch.empty((M, D), device=dev)
            pos = torch.full((M,), P, dtype=torch.int32, device=dev)
            hlen, fin = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
            nxt, ch = torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            err, scratch = torch.zeros(1, dtype=torch.int32, device=dev), ops.contrast_scratch(B, k, cap, dev)
            kc, vc = (torch.zeros((L, B, NH, cap, 64), device=dev) for _ in range(2))
            kt, vt = (torch.randn((L, M, NH, 1, 64), generator=g).to(dev) for _ in range(2))

            def launches():
                pos.fill_(P)
                ops.contrast_candidates(logits, k=k, step_tokens=st, prob=pr, chosen=chosen_prev, k_prev=k, finished=fin)
                ops.contrast_hidden(w, x, u.view(M, 1, D))
                ops.contrast_select(u, pr, hist, hist_rows=pos, p_stride=k, hist_len=hlen, alpha=ALPHA, step_tokens=st, finished=fin,
                                    next_token=nxt, chosen=ch, scratch=scratch, error_word=err)
                ops.kv_cache_commit(kt, vt, kc, vc, ch, pos, err, finished=fin)

            def pick(recs):
                out = {}
                for kind, ra, rb, rc, ms in recs:
                    if kind == "misc" and (ra, rb, rc) == (B, V, k):
                        out["candidates"] = ms
                    elif kind == "layernorm" and (ra, rb) == (M, D):
                        out["hidden"] = ms
                    elif kind == "misc" and (ra, rb, rc) == (M, cap, D):
                        out["select_partial"] = ms
                    elif kind == "misc" and (ra, rb, rc) == (B, k, D):
                        out["select_choice"] = ms
                    elif kind == "misc" and (ra, rb, rc) == (L * B * NH, 1, 4):
                        out["commit"] = ms
                assert len(out) == 5, recs
                return out
            best = best_us(launches, pick)
            if a.check:
                launches()
                torch.cuda.synchronize()
                assert int(err.item()) == 0
                rows = torch.arange(B, device=dev) * k + chosen_prev.long()
                lp, tl, ti = torch.zeros(B, 1, device=dev), torch.zeros(B, 1, k, device=dev), torch.zeros(B, 1, k, dtype=torch.int64, device=dev)
                ops.step_logprobs(logits[rows].contiguous(), torch.zeros(B, dtype=torch.int64, device=dev), out=lp, col=0, top_n=k, top_out=tl, top_ids=ti)
                assert torch.equal(st.view(B, k), ti[:, 0])
                pen = torch.einsum("bkd,bpd->bkp", u.view(B, k, D).double(), hist[:, :P].double()).amax(-1)
                score = (1.0 - ALPHA) * pr.view(B, k).double() - ALPHA * pen
                assert torch.equal(score.argmax(-1).to(torch.int32), ch), (score, ch)
                ar = torch.arange(B, device=dev)
                assert torch.equal(kc[:, ar, :, P], kt[:, ar * k + ch.long(), :, 0]) and torch.equal(vc[:, ar, :, P], vt[:, ar * k + ch.long(), :, 0])
                assert torch.equal(hist[ar, P], u[ar * k + ch.long()]) and pos.tolist() == [P + 1] * M
            for name, us in best.items():
                print(json.dumps({"leg": "launch", "launch": name, "batch": B, "k": k, "history_rows": P, "vocab": V, "dim": D, "reps": a.reps,
                                  "kernel_us": round(us, 2), "checked": bool(a.check)}), flush=True)
            print(json.dumps({"leg": "launch", "launch": "sum of the five", "batch": B, "k": k, "history_rows": P,
                              "kernel_us": round(sum(best.values()), 2)}), flush=True)
            del kc, vc, kt, vt, hist, logits

if not a.skip_generate:
    from kosmosx.model import KosmosLanguage
    m = KosmosLanguage(vocab_size=V, dim=D, _seed=0).eval().to(dev)
    m.precision = a.precision

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for B in (int(x) for x in a.batches.split(",")):
        tok = torch.randint(0, V, (B, a.prompt), generator=torch.Generator().manual_seed(B)).to(dev)
        for k in (int(x) for x in a.candidates.split(",")):
            legs = {"greedy": lambda n: m.generate(tok, n), "contrastive": lambda n: m.generate(tok, n, penalty_alpha=ALPHA, top_k=k)}
            for fn in legs.values():                           # warm-up: packs the weights, loads the code objects
                fn(2)
            ms = {(name, n): [] for name in legs for n in (1, a.new)}
            for _ in range(a.reps):
                for name, fn in legs.items():                  # alternating
                    for n in (1, a.new):
                        ms[(name, n)].append(timed(lambda: fn(n)))
            per = {name: (min(ms[(name, a.new)]) - min(ms[(name, 1)])) / (a.new - 1) for name in legs}
            print(json.dumps({"leg": "generate", "batch": B, "k": k, "rows_per_step": B * k, "prompt": a.prompt, "new": a.new,
                              "precision": a.precision, "reps": a.reps, "greedy_ms_per_token": round(per["greedy"], 4),
                              "contrastive_ms_per_token": round(per["contrastive"], 4),
                              "ratio": round(per["contrastive"] / per["greedy"], 3)}), flush=True)
