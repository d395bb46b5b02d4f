"""Summary of one kernel trace of tools/bench_generate.py (variant (a), B = 1):

    rocprofv3 --kernel-trace --memory-copy-trace --stats -d OUT -o gen -- python tools/bench_generate.py --batches 1 --only a --reps 1
    python tools/trace_generate_summary.py OUT/gen_results.db

(the ragged loop: ... --batches 4 --ragged --only r --reps 1; its step starts with step_prepare_kernel instead of embed_step_kernel)

Looks at the second (timed) generate() of the run, from its first to its 64th sampler launch: kernel dispatches per step,
memory copies inside that window (there must be none: no stop poll without an eos_token_id), and the sampler's own time."""
import sqlite3
from collections import Counter
import sys

c = sqlite3.connect(sys.argv[1])
rows = c.execute("select name,start,end,duration from kernels order by start").fetchall()
samp = [r for r in rows if "sample_kernel" in r[0]]
print("sample_kernel dispatches in the run:", len(samp))
w0, w1 = samp[64][1], samp[127][2]
inwin = [r for r in rows if w0 <= r[1] <= w1]
print("kernel dispatches from the 1st to the 64th sampler launch of one generate():", len(inwin), "->", (len(inwin) - 1) / 63,
      "per step (decode step + kx_embed_step / kx_step_prepare + kx_sample_logits)")
odd = {n[:100]: k for n, k in Counter(r[0] for r in inwin).items() if k % 63 and "sample_kernel" not in n}
print("kernels in that window that are not once-per-step (name: dispatches):", odd or "none")
for r in inwin:                                       # where each of them sits: after which sampler launch of the call, next to what
    if r[0][:100] in odd:
        after = sum(1 for q in samp[64:128] if q[1] <= r[1])
        i = rows.index(r)
        print("  %s starts after sampler launch %d of 64, between [%s] and [%s]" % (
            r[0][:60], after, rows[i - 1][0][:70], rows[i + 1][0][:70] if i + 1 < len(rows) else "end of trace"))
cop = c.execute("select count(*) from rocpd_memory_copy where start>=? and start<=?", (w0, w1)).fetchone()[0]
print("memory copies of any direction in that window:", cop)
d = sorted(r[3] for r in samp[64:128])
print("sample_kernel duration, ns (V=32002, top_k=50, top_p=0.9, T=0.8): min %d median %d max %d" % (d[0], d[len(d) // 2], d[-1]))
for kname in ("embed_step", "step_prepare"):
    es = sorted(r[3] for r in rows if kname in r[0])
    if es:
        print("%s_kernel: %d dispatches, median %d ns" % (kname, len(es), es[len(es) // 2]))
print("\ntop kernels of the whole run (name, calls, total, average, %):")
for r in c.execute("select name,total_calls,total_duration,average,percentage from top_kernels order by total_duration desc limit 12"):
    print("  %-90s %6d %12d %10.0f %6.2f" % (r[0][:90], r[1], r[2], r[3], r[4]))
