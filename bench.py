#!/usr/bin/env python
"""bench.py — multimodal forward samples/s (224x224 image + 50 tokens) @ ViT-L/14 + Perceiver + 24L/2048d.

    python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the headline line (`value`, `ms_per_step`); every other
figure of the line (`roofline`, `parity`, `cpu_baseline`, the other precision modes, `c3`, `batch1`, `decode`,
`training_step`, `kernel_breakdown`) is measured only with `--full` and is null otherwise.  `--dump-outputs DIR` writes
what the last timed step returned (a fixed sample of the logits, float32 .npy) so two builds can be compared.

One process per GPU (RCCL over xGMI for N > 1).  A "step" is one pass of the hot path
(`Kosmos.forward`, /root/reference/kosmosx/model.py:208-253) over one per-GPU shard of synthetic
input already resident in HBM: `--batch` samples (default 32 = BASELINE.json configs[3] per-GPU share,
256 / 8), each one 1x3x224x224 image + 50 text tokens -> logits [114, 32002]; for N > 1 the step ends
with the all-gather of logits (bf16 on the wire, overlapped with the next step's compute).
Weak scaling: per-GPU work is fixed as N grows.  Rank 0 prints ONE JSON line.

Two steps are kept in flight on two streams (`--pipeline`), and the library is told so (`--objective`, kx_set_tuning key 18 =
"throughput": per GEMM the launch with the fewest CU-microseconds; with `--pipeline 1` "latency": the launch that finishes soonest
alone — same bits either way); `config.schedule_objective` records it, `roofline` is measured on the timed
loop's launches and also reports the family's rate under the latency objective.

Headline arithmetic (`--precision`, default mixed): the fastest mode that holds the north star's 1e-3 logit tolerance
against the fp32 CPU path — `parity` in the JSON is measured in the same run.  Plain bf16 operands (3.5e-2) are
reported in `precision_modes` with their parity next to their (higher) throughput; `c3` is BASELINE.json configs[2]
(text-only B=32, T=2046: the config of the >= 40 % MFMA target), `batch1` configs[1] (HBM roofline).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
for p in (str(ROOT), str(ROOT / "kosmos-x_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("KOSMOSX_NO_LOGGING_CONFIG", "1")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (MI355X_MICROARCH.md, chip-level parameters)
PEAK_F32_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="samples per GPU per step")
    ap.add_argument("--text-len", type=int, default=50)
    ap.add_argument("--precision", default="mixed", choices=["bf16", "fp32", "bf16x3", "f16c", "mixed", "f16"],
                    help="headline arithmetic.  Default mixed: the fastest mode that holds the north star's 1e-3 logit "
                         "tolerance — the error-budgeted mix of plain fp16 (CLIP tower) and f16c (Perceiver, decoder: "
                         "fp16 MFMA + two fp8 correction MFMAs); bf16 is reported next to it with its parity")
    ap.add_argument("--no-extra", action="store_true", help="skip the c3 / batch-1 / training legs (headline only)")
    ap.add_argument("--no-gather", action="store_true", help="skip the logits all-gather (N > 1)")
    ap.add_argument("--gather-algo", default=os.environ.get("KOSMOSX_GATHER_ALGO", "all_gather"), choices=["auto", "all_gather", "direct"],
                    help="all_gather (default): RCCL's own collective — the only schedule that has run on more than one "
                         "GPU-backed rank so far.  auto: by message size — world-1 grouped send/recv pairs, one xGMI link per "
                         "peer, for the 233 MB logits shard at N > 2 (~1.5 ms by SURVEY 8e's arithmetic against ~10 ms for a "
                         "ring), all_gather for small messages, N = 2 and whenever a shard is empty; direct forces the grouped "
                         "schedule.  direct / auto stay opt-in (KOSMOSX_GATHER_ALGO) until an 8-GPU node has run them: "
                         "gloo world 2 / 3 and RCCL world 1 are what cover them (ADVICE r4)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="budget for the cpu_baseline sample")
    ap.add_argument("--prof-steps", type=int, default=3, help="instrumented steps for the roofline leg")
    ap.add_argument("--objective", default="auto", choices=["auto", "latency", "throughput"],
                    help="scheduling objective of the library's kernel choice (kx_set_tuning key 18); auto = throughput when "
                         "--pipeline >= 2, else latency (tools/r6_round.sh prof32 profiles the headline's kernels on one stream)")
    ap.add_argument("--pipeline", type=int, default=2,
                    help="issue consecutive steps round-robin on P HIP streams (independent requests overlap: one "
                         "step's partial kernel waves are filled by its neighbour's)")
    ap.add_argument("--graph", action="store_true", help="replay the forward as one hipGraph (launch-bound batches)")
    ap.add_argument("--streams", type=int, default=1, help="micro-batch the shard over S HIP streams (overlaps kernel tails)")
    ap.add_argument("--gemm-tile", type=int, default=0, help="kernel-variant override (kx_set_tuning key 1), A/B only")
    ap.add_argument("--tune", default="", help="A/B only: comma list of kx_set_tuning key=value pairs, e.g. 4=1")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: the instrumented roofline pass, the other precision "
                         "modes, parity and the CPU baseline, and the c3 / batch-1 / decode / training legs (off: the line "
                         "carries the headline only; --no-extra, --no-cpu-baseline and --prof-steps trim a --full run)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one returned to DIR/<name>.npy (float32): the logits of "
                         "the first and the last sample of the shard and a fixed, seeded sample of the whole logits tensor")
    return ap.parse_args()


DUMP_SAMPLE = 1 << 20          # elements of the seeded whole-tensor sample (4 MB in float32)
DUMP_SEED = 20240
DUMP_SAMPLE_BYTES = 28 << 20  # cap per dumped sample: 2 x 28 MB + 4 MB stays under 64 MB


def dump_outputs(out, dirname):
    """What the timed path returned in its last step, as float32 .npy files (< 64 MB in all): the logits of the first and
    the last sample (every position, up to DUMP_SAMPLE_BYTES each), and DUMP_SAMPLE elements of the whole tensor at flat
    indices drawn from a fixed seed (sorted)."""
    import numpy as np
    d = Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    flat = out.reshape(-1)
    idx = torch.randint(0, flat.numel(), (min(DUMP_SAMPLE, flat.numel()),),
                        generator=torch.Generator().manual_seed(DUMP_SEED)).sort().values.to(out.device)
    rows = max(1, DUMP_SAMPLE_BYTES // (out.shape[-1] * 4))         # positions kept per sample (all 114 by default)
    arrays = {"logits_first_sample": out[0, :rows], "logits_last_sample": out[-1, :rows], "logits_seeded_sample": flat[idx]}
    for name, a in arrays.items():
        np.save(d / f"{name}.npy", a.float().cpu().numpy())


_PMC_TILES = {"160x128": "gemm_kernel<{T},160,128", "128x128": "gemm_kernel<{T},128,128", "64x64": "gemm_kernel<{T},64,64",
              "256x128_phased": "gemm_kernel_p3<{T}", "256x256_phased": "gemm_kernel_p5<{T}"}
_PMC_TYPES = {"bf16": "bf16", "f16c": "f16c_t", "f16": "f16c_t"}      # KX_PREC_F16 rows run the f16c_t kernels without correction tiles
_PMC_FILES = {"mixed": ("profiles/r06_pmc.json", "profiles/r06_pmc_summary.md")}
_PMC_DECODE = "profiles/r06_decode_pmc.json"      # tools/pmc_round.sh on tools/bench_decode.py (bf16 and mixed), same digest guard


def pmc_kernel_prefix(kind):
    """kernel-kind name of kx_prof (gemm_<type>_<tile>) -> prefix of the kernel's demangled name in the PMC tables"""
    parts = kind.split("_", 2)
    if len(parts) == 3 and parts[0] == "gemm" and parts[1] in _PMC_TYPES and parts[2] in _PMC_TILES:
        return _PMC_TILES[parts[2]].format(T=_PMC_TYPES[parts[1]])
    return "attn_" if kind.startswith("attn") else None


def gemm_sources_digest() -> str:
    """sha256 over the sources of the GEMM kernel family (what roofline.traffic was measured on)."""
    import hashlib
    h = hashlib.sha256()
    csrc = Path(__file__).resolve().parent / "kosmos-x_amd" / "csrc"
    for f in sorted(list(csrc.glob("kx_gemm*")) + [csrc / "kx_common.h"]):
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()[:16]



def pmc_traffic(kernel, args):
    """roofline.traffic: HBM-side bytes per launch of the dominant kernel.  PMC counters need rocprofv3 around the
    process, so they are not collected here: the value comes from the committed PMC pass of this same command
    (tools/pmc_round.sh -> tools/pmc_summary.py -> profiles/r0N_*_pmc.json; FETCH_SIZE x2 + WRITE_SIZE, the guide's gfx950
    correction) and is only reported for the default workload and the precision it was measured on; otherwise null."""
    ent = _PMC_FILES.get(args.precision)
    key = pmc_kernel_prefix(kernel)
    if not (ent and key and args.batch == 32 and args.text_len == 50):
        return {"traffic": None}
    f = Path(__file__).resolve().parent / ent[0]
    if not f.exists():
        return {"traffic": None, "traffic_source": f"{ent[0]} not collected yet for this code (tools/pmc_round.sh)"}
    data = json.loads(f.read_text())
    meta = data.pop("_meta", {})
    if meta.get("gemm_sources_digest") != gemm_sources_digest():          # counters of other code are not this code's traffic
        return {"traffic": None, "traffic_source": f"{ent[0]} was collected on GEMM sources {meta.get('gemm_sources_digest')}, "
                                                   f"this library is built from {gemm_sources_digest()}: refused (re-run tools/pmc_round.sh)"}
    rows = [v for k, v in data.items() if k.startswith(key)]
    n = sum(v["launches"] for v in rows)
    if not n:
        return {"traffic": None}
    t = sum(v["launches"] * (v["fetch_bytes_x2"] + v["write_bytes"]) for v in rows) / n
    return {"traffic": round(t), "traffic_unit": "bytes/launch", "traffic_source": ent[1] + " (committed PMC pass of this command, not this run)"}


def decode_traffic(mode):
    """HBM-side bytes per decode STEP from the committed PMC pass of tools/bench_decode.py --precision <mode> (FETCH_SIZE x2 +
    WRITE_SIZE summed over the step's launches), refused when the kernels have changed since."""
    f = Path(__file__).resolve().parent / _PMC_DECODE
    if not f.exists():
        return {"traffic": None, "traffic_source": f"{_PMC_DECODE} not collected yet for this code"}
    data = json.loads(f.read_text())
    if data.get("_meta", {}).get("gemm_sources_digest") != gemm_sources_digest():
        return {"traffic": None, "traffic_source": f"{_PMC_DECODE} was collected on other kernel sources "
                                                   f"({data.get('_meta', {}).get('gemm_sources_digest')} vs {gemm_sources_digest()}): refused"}
    ent = data.get(mode)
    if not ent:
        return {"traffic": None}
    return {"traffic": ent["bytes_per_step"], "traffic_unit": "bytes/step",
            "traffic_source": f"{_PMC_DECODE} (committed FETCH_SIZE x2 + WRITE_SIZE pass of tools/bench_decode.py --precision {mode}; not this run)"}


def kernel_report(records, steps):
    """Aggregate kx_prof records (one per kernel launch) into per-kernel totals per step."""
    agg = {}
    shapes = {}
    for kind, a, b, c, ms in records:
        if kind.startswith("gemm"):
            se = shapes.setdefault((kind, a, b, c), [0, 0.0])
            se[0] += 1
            se[1] += ms
        e = agg.setdefault(kind, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
        e["launches"] += 1
        e["ms"] += ms
        if kind.startswith("gemm"):
            e["flops"] += 2.0 * a * b * c                     # algorithmic: 2*M*N*K per launch
        elif kind.startswith("attn"):
            e["flops"] += 4.0 * a * b * c * 64                # dense QK^T + PV, head_dim 64 (B*H, Tq, Tk)
        elif kind == "layernorm":
            # c = HBM bytes per value of the launch as kx_layernorm reports them (fp32 row in + pre_add row + the output
            # format's bytes: 6 bf16 / fp16 rows, 8 KX_F16C or fp32 rows, 10 KX_BF16X3); 0 / 1 = entry points that do not
            # report it (kx_gelu_layernorm, the backward): fp32 in, 16-bit out
            e["bytes"] += a * b * (float(c) if c > 1 else 6.0)
    for e in agg.values():
        e["launches"] /= steps
        e["ms"] /= steps
        e["flops"] /= steps
        e["bytes"] /= steps
    top = sorted(shapes.items(), key=lambda kv: -kv[1][1])[:14]
    agg["_gemm_shapes"] = [{"kernel": k[0], "M": k[1], "N": k[2], "K": k[3], "launches_per_step": v[0] / steps,
                            "ms_per_step": round(v[1] / steps, 4),
                            "tflops": round(2.0 * k[1] * k[2] * k[3] * v[0] / (v[1] * 1e-3) / 1e12, 1)} for k, v in top]
    return agg


DTYPE_NAMES = {"mixed": "mixed fp16/f16c (CLIP tower: fp16 MFMA; Perceiver + decoder: fp16 MFMA + fp8-e4m3 correction MFMAs; "
                        "fp32 accumulate / residual / statistics)", "f16": "fp16",
               "bf16": "bf16", "fp32": "fp32", "bf16x3": "bf16x3 (bf16 MFMA on hi/lo split operands)",
               "f16c": "f16c (fp16 MFMA + fp8-e4m3 correction MFMAs, fp32 accumulate / residual / statistics)"}
TOL = {"bf16": 1e-3, "f16c": 1e-3, "mixed": 1e-3, "f16": 1e-3, "bf16x3": 1e-3, "fp32": 1e-5}     # north star: 1e-3 bf16 class / 1e-5 fp32


def parity_block(mode, parity_all):
    """max|logit difference| / rms(logits) of the headlined arithmetic against the fp32 CPU path, measured in this run.
    `logit_rms` is stated so that the relative figure converts to the north star's absolute one on any weights."""
    if not parity_all or mode not in parity_all:
        return None
    e = parity_all[mode]
    rms = parity_all.get("_logit_rms")
    return {"dtype": mode, "max_abs_over_rms": float(f"{e:.3e}"), "tolerance": TOL[mode], "meets": bool(e <= TOL[mode]),
            **({"logit_rms": float(f"{rms:.4f}"), "max_abs": float(f"{e * rms:.3e}")} if rms else {}),
            "against": "fp32 CPU oracle forward of sample 0 (cpu_baseline leg) vs row 0 of the full-shard HIP forward — the "
                       "benchmarked kernel path — identical weights and inputs"}


def modes_block(head, head_value, head_s_per_step, other, parity_all, flops_per_sample, B):
    """Every arithmetic mode on the same shard: throughput next to its parity, so a number can never be read without its
    tolerance.  `fastest_meeting_tolerance` names the mode a parity-bound deployment would run."""
    rows = {head: {"samples_per_s": head_value, "ms_per_step": round(head_s_per_step * 1e3, 3), "headline": True}}
    for m, v in (other or {}).items():
        rows[m] = dict(v)
    for m, v in rows.items():
        v["model_tflops"] = round(flops_per_sample * v["samples_per_s"] / 1e12, 1)
        v["mfma_peak_frac_end_to_end"] = round(flops_per_sample * v["samples_per_s"] / 1e12 / PEAK_BF16_TFLOPS, 4)
        if parity_all and m in parity_all and not m.startswith("_"):
            v["parity_max_abs_over_rms"] = float(f"{parity_all[m]:.3e}")
            v["tolerance"] = TOL[m]
            v["meets_tolerance"] = bool(parity_all[m] <= TOL[m])
    ok = [m for m, v in rows.items() if v.get("meets_tolerance")]
    rows["fastest_meeting_tolerance"] = max(ok, key=lambda m: rows[m]["samples_per_s"]) if ok else None
    # which fp8 correction products the KX_PREC_F16C launches of `mixed` / `f16c` contract (kx_gemm_args.f16c_corr,
    # tuning key 16) and the measured reason: every decoder family one-sided ALONE leaves >= 9.6e-4 on the logits (C1 rows of this
    # workload and a C3 row; acceptance line 5e-4), the Perceiver weight-side only 5.1e-4 for 0.6 % of the step
    rows["f16c_correction_assignment"] = {
        "tuning_key_16": 0, "assignment": "both corrections in every GEMM family (qkv, out_proj, fc1, fc2, output projection, Perceiver)",
        "one_sided_table": "profiles/r06_a_corr_table_one_sided_corrections.json (tools/corr_table.py --c3; DESIGN.md section 5)",
        "cheapest_single_family_one_sided": {"fc2 weight-side only": {"c1_max_abs_over_rms": 1.038e-3, "c3": 9.608e-4, "step_gain": "4.3 %"}},
        "split_fp16_attention": "three products per matrix product; P plain / V split (tuning key 2 = 6) measured 5.8e-4 (C1) / 5.1e-4 (C3) "
                                "for -17 % of the T = 2046 kernel: over the 5e-4 acceptance line, opt-in"}
    return rows


def host_info() -> dict:
    """What the cpu_baseline number was measured ON: logical CPUs, the affinity mask
    of this process, the cgroup CPU quota (a container can see 128 CPUs and be allowed 16 cores' worth of time — then every
    thread count above the quota oversubscribes), the CPU model, torch's thread settings."""
    info = {"os_cpu_count": os.cpu_count(), "torch_num_threads_default": torch.get_num_threads()}
    try:
        info["sched_affinity"] = len(os.sched_getaffinity(0))
    except Exception:
        pass
    quota = None
    try:                                                     # cgroup v2, then v1
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else float(q) / float(per)
    except Exception:
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            quota = None if q <= 0 else q / per
        except Exception:
            pass
    info["cgroup_cpu_quota_cores"] = quota
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                info["cpu_model"] = line.split(":", 1)[1].strip()
                break
        info["sockets"] = len({l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("physical id")}) or None
    except Exception:
        pass
    info["omp_num_threads_env"] = os.environ.get("OMP_NUM_THREADS")
    info["torch_version"] = torch.__version__
    try:
        info["mkl"] = bool(torch.backends.mkl.is_available())
    except Exception:
        pass
    return info



def c3_leg(cfg, dev, _hip, steps=10, warmup=2, check=True):
    """BASELINE configs[2].  Every mode carries its parity against the CPU oracle on ONE row of the batch (rows are
    independent; the full-size test checks more) and `meets_tolerance`; the block's own figures are those of the FASTEST
    MODE INSIDE 1e-3 (bf16's 0.40 is context, never the target's number)."""
    from kosmosx.model import KosmosLanguage
    d = cfg.decoder
    lm = KosmosLanguage(vocab_size=cfg.vocab, dim=d.decoder_embed_dim, _seed=0).eval()   # example_lang.py:9-12
    lm_cpu = None
    if check:
        sys.path.insert(0, str(ROOT / "tests"))
        from helpers import oracle_weights as _ow
        lm_cpu = _ow(lm)
    lm = lm.to(dev)
    kept = {}
    B, T, D, F, V, L = 32, 2046, d.decoder_embed_dim, d.decoder_ffn_embed_dim, cfg.vocab, d.decoder_layers
    tok = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(0)).to(dev)
    flops = B * T * (L * (8 * D * D + 4 * D * F) + 2 * D * V) + B * L * 2 * D * T * (T + 1)     # causal-algorithmic, SURVEY 8d
    out = {"workload": f"KosmosLanguage forward, batch {B}, seq {T}, 24L/2048d, logits fp32 [{B},{T},{V}] "
                       "(BASELINE.json configs[2]; example_lang.py's 2048 overflows the position table)",
           "algorithmic_tflop_per_forward": round(flops / 1e12, 2), "steps": steps, "warmup": warmup}
    for mode in ("bf16", "f16c"):
        lm.precision = mode
        with torch.no_grad():
            for _ in range(warmup):
                lm(tok)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(steps):
                lm(tok)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t1) / steps
            _hip.prof_enable(True)
            lg = lm(tok)
            torch.cuda.synchronize()
            recs = _hip.prof_collect()
            _hip.prof_enable(False)
            kept[mode] = lg[B - 1].float().cpu()               # the LAST row of the batch: [T, V]
            del lg
        agg, shapes = {}, {}
        for kind, x, y, z, ms in recs:
            e = agg.setdefault(kind, [0, 0.0]); e[0] += 1; e[1] += ms
            if kind.startswith("gemm"):
                e = shapes.setdefault((x, y, z), [0, 0.0]); e[0] += 1; e[1] += ms
        out[mode] = {"ms_per_forward": round(dt * 1e3, 2), "tokens_per_s": round(B * T / dt, 1),
                     "model_tflops": round(flops / dt / 1e12, 1), "frac_of_bf16_mfma_peak": round(flops / dt / 1e12 / PEAK_BF16_TFLOPS, 4),
                     "kernels_ms_per_forward": {k: {"launches": v[0], "ms": round(v[1], 2)} for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1])},
                     "gemm_shapes": [{"M": k[0], "N": k[1], "K": k[2], "launches": v[0], "ms": round(v[1], 2),
                                      "tflops": round(2.0 * k[0] * k[1] * k[2] * v[0] / v[1] / 1e9, 1)}
                                     for k, v in sorted(shapes.items(), key=lambda kv: -kv[1][1])]}
        lm.decoder.invalidate_packed()
    del lm
    torch.cuda.empty_cache()
    if lm_cpu is not None:
        from oracle import kosmos_oracle as O
        t0 = time.perf_counter()
        ref = O.kosmos_language_forward(lm_cpu, tok[B - 1:].cpu(), O.DecoderCfg(vocab=cfg.vocab))[0]
        rms = float(ref.pow(2).mean().sqrt())
        for mode, got in kept.items():
            e = float((got - ref).abs().max() / rms)
            out[mode].update({"parity_max_abs_over_rms": float(f"{e:.3e}"), "tolerance": 1e-3, "meets_tolerance": bool(e <= 1e-3)})
        out["parity_against"] = (f"fp32 CPU oracle forward of row {B - 1} of the batch, all {T} positions (logit rms {rms:.4f}; "
                                 f"{time.perf_counter() - t0:.0f} s of host time, outside every timed region)")
        # the headline choice below rests on ONE batch row (a CPU forward of T = 2046 is 25 s per row); the same modes are
        # held to the same bound on three rows spread over the batch in tests/test_fullsize_parity_gpu.py
        out["parity_rows"] = [B - 1]
        out["parity_rows_note"] = ("one row of the batch, every position; rows 0 / 19 / 31 of the same workload are bounded in "
                                   "tests/test_fullsize_parity_gpu.py::test_c3_batch32_seq2046_rows_against_the_oracle")
        ok = [m for m in kept if out[m]["meets_tolerance"]]
        out["fastest_meeting_tolerance"] = min(ok, key=lambda m: out[m]["ms_per_forward"]) if ok else None
        if ok:
            b = out[out["fastest_meeting_tolerance"]]
            out.update({k: b[k] for k in ("ms_per_forward", "tokens_per_s", "model_tflops", "frac_of_bf16_mfma_peak")})
    else:
        out["note"] = "parity not measured in this run (--no-cpu-baseline): no mode is headlined"
    return out


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("bench.py --gpus N > 1 must be launched with torch.distributed.run (one rank per GPU)")
        args.gpus = world
    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X: the Kosmos-X HIP path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    force_dist = os.environ.get("KOSMOSX_FORCE_DIST") == "1"     # exercise the RCCL path with a single rank (testing)
    if world > 1 or force_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group(backend="nccl", device_id=dev)   # "nccl" is RCCL on ROCm

    from kosmosx import _hip
    from kosmosx.config import DecoderConfig, KosmosConfig
    from kosmosx.model import Kosmos
    from kosmosx.parallel import LogitsGatherer

    cfg = KosmosConfig(decoder=DecoderConfig())
    t_build = time.time()
    model = Kosmos._from_config(cfg, seed=0).eval()            # identical weights on every rank (replicated)
    cpu_weights = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        from helpers import oracle_weights
        cpu_weights = oracle_weights(model)                     # shares the CPU storage, no copy
    model = model.to(dev)
    model.precision = args.precision
    if args.gemm_tile:
        _hip.load().kx_set_tuning(1, args.gemm_tile)
    for kv in filter(None, args.tune.split(",")):
        k, v = kv.split("=")
        _hip.load().kx_set_tuning(int(k), int(v))
    model.use_hip_graphs = bool(args.graph)
    t_build = time.time() - t_build

    g = torch.Generator().manual_seed(1000 + rank)              # per-rank synthetic shard
    B, Tt = args.batch, args.text_len
    tok = torch.randint(0, cfg.vocab, (B, Tt), generator=g).to(dev)
    img = torch.randn(B, 3, cfg.vit.image, cfg.vit.image, generator=g).to(dev)
    gatherer = (LogitsGatherer(wire_dtype=None, force=force_dist, algo=args.gather_algo, slots=max(1, args.pipeline) + 1)
                if ((world > 1 or force_dist) and not args.no_gather) else None)
    if gatherer is not None:
        model.logits_dtype = torch.bfloat16       # the logits GEMM's epilogue writes the wire format itself: no cast kernel

    S = max(1, args.streams)
    side = [torch.cuda.Stream(device=dev) for _ in range(S)] if S > 1 else []
    toks, imgs = tok.chunk(S), img.chunk(S)
    logits_buf = torch.empty((B, Tt + cfg.perceiver.latents, cfg.vocab), dtype=torch.float32, device=dev) if S > 1 else None

    def forward_shard():
        if S == 1:
            return model(tok, img)
        cur = torch.cuda.current_stream(dev)
        lo = 0
        for st, t_, i_ in zip(side, toks, imgs):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                logits_buf[lo:lo + t_.shape[0]].copy_(model(t_, i_))
            lo += t_.shape[0]
        for st in side:
            cur.wait_stream(st)
        return logits_buf

    P = max(1, args.pipeline)
    pipe = [torch.cuda.Stream(device=dev) for _ in range(P)] if P > 1 else []
    step_no = [0]

    def step():
        with torch.no_grad():
            if P > 1:                                   # independent requests: step i runs on stream i % P
                st = pipe[step_no[0] % P]
                step_no[0] += 1
                st.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(st):
                    logits = forward_shard()
                    return gatherer.gather(logits, total=B * world) if gatherer is not None else logits
            logits = forward_shard()
            if gatherer is not None:
                return gatherer.gather(logits, total=B * world)
            return logits

    def fence():
        for st in pipe:
            torch.cuda.current_stream(dev).wait_stream(st)
        if gatherer is not None:
            gatherer.wait()
        torch.cuda.synchronize()
        if world > 1 or force_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # Scheduling objective (kx_set_tuning key 18): with two or more steps in flight the library is asked for the
    # launches with the fewest CU-microseconds (a launch's idle CUs are filled by the other step), with one step for the launches
    # that finish soonest alone.  The headline loop, the instrumented roofline pass, the other precision modes and the parity
    # forward all run under THIS objective; the single-request legs (training, C3, decode, batch 1) under "latency".
    from kosmosx import ops as _ops
    objective = args.objective if args.objective != "auto" else ("throughput" if P > 1 else "latency")
    _ops.set_objective(objective)
    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    assert out.shape[-1] == cfg.vocab and out.shape[-2] == Tt + cfg.perceiver.latents
    if args.dump_outputs and rank == 0:
        dump_outputs(out, args.dump_outputs)

    # ---- roofline leg: the same step, instrumented launch by launch with HIP events on the launch stream ----
    roofline, breakdown, gemm_shapes = None, None, None
    if rank == 0 and args.full and args.prof_steps > 0:
        model.use_hip_graphs = False                        # per-launch events cannot be recorded under capture/replay
        _hip.prof_enable(True)
        for _ in range(args.prof_steps):
            with torch.no_grad():
                model(tok, img)
        torch.cuda.synchronize()
        recs = _hip.prof_collect()
        _hip.prof_enable(False)
        agg = kernel_report(recs, args.prof_steps)
        gemm_shapes = agg.pop("_gemm_shapes")
        dom = max(agg, key=lambda k: agg[k]["ms"])
        e = agg[dom]
        if e["flops"] > 0:
            peak = PEAK_F32_TFLOPS if "_f32" in dom else PEAK_BF16_TFLOPS    # fp16 and bf16 MFMA share the dense peak
            ach = e["flops"] / (e["ms"] * 1e-3) / 1e12
            roofline = {"kernel": dom, "bound": "mfma",
                        "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s",
                        "frac": round(ach / peak, 4), **pmc_traffic(dom, args),
                        "measured_in": "instrumented single-stream pass (HIP events around every launch) of the SAME launches as the "
                                       f"timed loop (scheduling objective: {objective}); `value` is measured with {P} steps in "
                                       f"flight on {P} streams",
                        **({"note": "f16c kernels (Perceiver, decoder; every kernel in --precision f16c) issue one fp16 MFMA "
                            "pass plus two fp8 correction passes at twice the rate = 2x the bf16 MFMA time per ALGORITHMIC "
                            "flop, which is what `achieved` counts; the CLIP tower's kernels in mixed mode are plain fp16 (1x)",
                            "matrix_pipe_frac": round(2.0 * ach / peak, 4)}   # MFMA issue time of this kernel / its peak issue rate
                           if "_f16c_" in dom else {}),
                        "launches_per_step": e["launches"], "avg_launch_ms": round(e["ms"] / e["launches"], 5),
                        "algorithmic_flops_per_step": e["flops"]}
        else:
            ach = e["bytes"] / (e["ms"] * 1e-3) / 1e9
            roofline = {"kernel": dom, "bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                        "frac": round(ach / PEAK_HBM_GBS, 4), "traffic": None,
                        "launches_per_step": e["launches"], "avg_launch_ms": round(e["ms"] / e["launches"], 5)}
        if objective == "throughput" and e["flops"] > 0:
            # the same family with every launch chosen to finish soonest ALONE (latency objective): the kernel's own best rate.
            # Under the throughput objective the launches above are chosen for the fewest CU-microseconds (256-row tiles where
            # 192-row ones only saved padding); alone on the chip they are a few per cent slower — which is the point of an objective
            _ops.set_objective("latency")
            _hip.prof_enable(True)
            for _ in range(args.prof_steps):
                with torch.no_grad():
                    model(tok, img)
            torch.cuda.synchronize()
            agg_l = kernel_report(_hip.prof_collect(), args.prof_steps)
            _hip.prof_enable(False)
            _ops.set_objective(objective)
            if dom in agg_l and agg_l[dom]["ms"] > 0:
                ach_l = agg_l[dom]["flops"] / (agg_l[dom]["ms"] * 1e-3) / 1e12
                roofline["alone_under_latency_objective"] = {
                    "achieved": round(ach_l, 2), "frac": round(ach_l / peak, 4), "ms_per_step": round(agg_l[dom]["ms"], 4),
                    "note": "same family, same instrumented single-stream pass, launches chosen to finish soonest alone (what a "
                            "single-request caller runs; `value` is NOT measured with these launches)"}
        fam = [v for k, v in agg.items() if k.startswith("gemm_") and "_f32_" not in k]
        if fam:
            agg["gemm_16bit_all_variants"] = {"launches": sum(v["launches"] for v in fam), "ms": sum(v["ms"] for v in fam),
                                              "flops": sum(v["flops"] for v in fam), "bytes": 0.0}
        breakdown = {k: {"ms_per_step": round(v["ms"], 4), "launches_per_step": v["launches"],
                         **({"tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2)} if v["flops"] else {}),
                         **({"gbs": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1)} if v["bytes"] else {})}
                     for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])}

    # ---- the same step in the other precision modes (single-GPU run only; reported next to the headline, never as it) ----
    other_modes = None
    if rank == 0 and world == 1 and not force_dist and args.full and not args.no_cpu_baseline:
        other_modes = {}
        for mode in [m for m in ("bf16", "mixed", "f16c", "bf16x3", "fp32") if m != args.precision]:
            model.precision = mode
            k = args.steps if mode in ("bf16", "f16c", "mixed") else max(3, min(args.steps, 8))
            for _ in range(2):
                step()
            fence()
            t1 = time.perf_counter()
            for _ in range(k):
                step()
            fence()
            dt_m = (time.perf_counter() - t1) / k
            other_modes[mode] = {"samples_per_s": round(B / dt_m, 1), "ms_per_step": round(dt_m * 1e3, 3), "steps": k}
            model.invalidate_packed()
        model.precision = args.precision

    _ops.set_objective("latency")                            # the legs below issue one request at a time
    # ---- SURVEY 8f row 1 next to the headline: one training step of the text decoder (never part of `value`) ----
    training = None
    if rank == 0 and world == 1 and not force_dist and args.full and not args.no_cpu_baseline and not args.no_extra:
        try:
            from kosmosx.model import KosmosLanguage
            from kosmosx.training import LanguageModelTrainer
            tb = [torch.randint(2, cfg.vocab, (8, 512), generator=g).to(dev) for _ in range(4)]

            def train_leg(train_mode):                     # a fresh model per mode: the trainer updates its model's parameters
                lm = KosmosLanguage(vocab_size=cfg.vocab, dim=cfg.decoder.decoder_embed_dim, _seed=0).eval().to(dev)
                tr = LanguageModelTrainer(lm, precision="bf16", train_mode=train_mode, dropout_seed=1234)
                tr.step(tb[0])
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for i in range(1, 4):
                    tloss = tr.step(tb[i])
                torch.cuda.synchronize()
                dt_t = (time.perf_counter() - t1) / 3
                res = {"tokens_per_s": round(8 * 512 / dt_t, 1), "ms_per_step": round(dt_t * 1e3, 2), "loss": round(float(tloss), 4)}
                if train_mode:
                    res = {"dropout": tr.p_drop, "attention_dropout": tr.p_attn, **res}
                else:
                    # roofline of the step's dominant kernel family: one more step, instrumented launch by
                    # launch with HIP events on the launch stream, exactly as the headline's roofline leg
                    _hip.prof_enable(True)
                    tr.step(tb[0])
                    torch.cuda.synchronize()
                    trecs = _hip.prof_collect()
                    _hip.prof_enable(False)
                    tagg = kernel_report(trecs, 1)
                    tagg.pop("_gemm_shapes", None)
                    fam = {k: v for k, v in tagg.items() if k.startswith("gemm") and v["flops"] > 0 and k != "gemm_16bit_all_variants"}
                    if fam:
                        tdom = max(fam, key=lambda k: fam[k]["ms"])
                        te = fam[tdom]
                        tach = te["flops"] / (te["ms"] * 1e-3) / 1e12
                        tpeak = PEAK_F32_TFLOPS if "_f32" in tdom else PEAK_BF16_TFLOPS   # the headline roofline's rule
                        res["roofline"] = {"kernel": tdom, "bound": "mfma", "achieved": round(tach, 1), "peak": tpeak,
                                           "unit": "TFLOP/s", "frac": round(tach / tpeak, 4), "traffic": None,
                                           "launches_per_step": te["launches"], "ms_per_step": round(te["ms"], 2),
                                           "step_ms_in_gemms": round(sum(v["ms"] for v in fam.values()), 2),
                                           "measured_in": "one instrumented step (HIP events around every launch)"}
                del tr, lm
                torch.cuda.empty_cache()
                return res
            training = {"workload": "KosmosLanguage 24L/2048d next-token step: forward + backward + clip_grad_norm_(1.0) + "
                                    "AdamW, 8 x 512 tokens, bf16 products on fp32 master weights (tools/bench_train.py)",
                        **train_leg(False)}
            # ... and the reference's own mode of that step: model.train() (/root/reference/train.py:642) = dropout and
            # attention dropout 0.1 (kosmosx/model.py:175-177), Philox masks drawn inside the kernels
            training["train_mode"] = train_leg(True)
            del tb
        except Exception as e:                      # the headline line must not depend on the extra leg
            training = {"error": f"{type(e).__name__}: {e}"}

    # ---- BASELINE.json configs[2] ("C3"): text-only KosmosLanguage forward, B = 32, T = 2046 (2048 overflows the reference's
    # position table) — the config the north star's ">= 40 % of bf16 MFMA peak" is quoted on.  bf16 and f16c. ----
    c3 = None
    if rank == 0 and world == 1 and not force_dist and args.full and not args.no_extra:
        try:
            c3 = c3_leg(cfg, dev, _hip, check=not args.no_cpu_baseline)
        except Exception as e:
            c3 = {"error": f"{type(e).__name__}: {e}"}
        torch.cuda.empty_cache()

    # ---- incremental decoding, one token per step against the KV cache (B = 1): a step streams the
    # decoder's live weights once.  Every mode is timed and its logits kept; the cpu_baseline leg below compares them with the
    # oracle, and the block's headline is the FASTEST MODE THAT MEETS THE TOLERANCE (round 2 headlined
    # bf16, the mode the same line marks meets_tolerance: false).  "mixed" / "f16c" steps run fp32 products on block-scaled
    # 16-bit weights streamed as 2.125 bytes each (Decoder._forward_incremental; an f16c row would stream 4).
    decode, decode_check = None, None
    if rank == 0 and world == 1 and not force_dist and args.full and not args.no_extra:
        try:
            from kosmosx.model import KosmosLanguage
            d = cfg.decoder
            lm = KosmosLanguage(vocab_size=cfg.vocab, dim=d.decoder_embed_dim, _seed=0).eval()
            lm_cpu = None
            if cpu_weights is not None:
                from helpers import oracle_weights as _ow
                lm_cpu = _ow(lm)                              # CPU fp32 copies for the checker (cpu_baseline leg)
            lm = lm.to(dev)
            prefix, nstep = 114, 48
            dtok = torch.randint(0, cfg.vocab, (1, prefix + nstep + 8), generator=torch.Generator().manual_seed(0)).to(dev)
            L, D, F, V = d.decoder_layers, d.decoder_embed_dim, d.decoder_ffn_embed_dim, cfg.vocab
            nw = L * (4 * D * D + 2 * D * F) + D * V
            modes, kept = {}, {}
            for mode in ("bf16", "mixed", "fp32"):
                lm.precision = mode
                with torch.no_grad():
                    for rep in range(2):                      # rep 0 = warm-up
                        state = {"max_len": 512}
                        lm(dtok[:, :prefix], incremental_state=state)
                        for t in range(prefix, prefix + 4):
                            lm(dtok[:, :t + 1], incremental_state=state)
                        torch.cuda.synchronize()
                        outs = []
                        t1 = time.perf_counter()
                        for t in range(prefix + 4, prefix + 4 + nstep):
                            outs.append(lm(dtok[:, :t + 1], incremental_state=state))
                        torch.cuda.synchronize()
                        dts = (time.perf_counter() - t1) / nstep
                kept[mode] = torch.cat(outs, 1)[0].float().cpu()                   # [nstep, V]
                wbytes = {"bf16": 2.0, "mixed": 2.125, "fp32": 4.0}[mode]          # bytes streamed per weight
                cbytes = 2.0 if mode == "bf16" else 4.0                             # bytes per cached key / value
                wb = wbytes * nw + 2.0 * L * (prefix + 4 + nstep / 2) * D * cbytes
                modes[mode] = {"ms_per_token": round(dts * 1e3, 3), "tokens_per_s": round(1.0 / dts, 1),
                               "step_arithmetic": {"bf16": "bf16 operands, bf16 KV cache",
                                                   "mixed": "fp32 products on the exact-f32 MFMA; block-scaled 16-bit weights (int16 + one fp32 scale "
                                                            "per row and 32 columns: 2.125 bytes streamed per weight, rebuilt in registers), fp32 KV cache",
                                                   "fp32": "fp32 operands on the exact-f32 MFMA (weight-streaming kernel, 4 bytes per "
                                                           "weight), fp32 KV cache"}[mode],
                               "roofline": {"bound": "hbm", "achieved": round(wb / dts / 1e9, 1), "peak": PEAK_HBM_GBS,
                                            "unit": "GB/s", "frac": round(wb / dts / 1e9 / PEAK_HBM_GBS, 4),
                                            "algorithmic_bytes": wb, "note": "decoder weights + KV cache streamed once per token"}}
                del state
                lm.decoder.invalidate_packed()
                torch.cuda.empty_cache()
            for mode in ("bf16", "mixed"):
                modes[mode]["roofline"].update(decode_traffic(mode))
            decode = {"workload": f"KosmosLanguage decode step, batch 1, context {prefix + 4}..{prefix + 4 + nstep} tokens",
                      "modes": modes}
            decode_check = (lm_cpu, dtok[:, :prefix + 4 + nstep].cpu(), kept, prefix + 4)
            del lm
            torch.cuda.empty_cache()
        except Exception as e:
            decode = {"error": f"{type(e).__name__}: {e}"}

    # ---- BASELINE.json configs[1]: batch 1 (one 224x224 image + 50 tokens), one request at a time: weight-streaming bound ----
    batch1 = None
    if rank == 0 and world == 1 and not force_dist and args.full and not args.no_extra:
        batch1 = {}
        live_bytes = 3.20e9                                   # bf16 operand copies of the live weights
        for mode in ("bf16", "mixed"):
            model.precision = mode
            with torch.no_grad():
                for _ in range(3):
                    model(tok[:1], img[:1])
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(20):
                    model(tok[:1], img[:1])
                torch.cuda.synchronize()
            lat = (time.perf_counter() - t1) / 20
            wbytes = live_bytes + (2.59e9 if mode == "mixed" else 0.0)  # f16c rows (Perceiver, decoder) are 4 bytes per value
            batch1[mode] = {"latency_ms": round(lat * 1e3, 3), "samples_per_s": round(1.0 / lat, 1),
                            "roofline": {"bound": "hbm", "achieved": round(wbytes / lat / 1e9, 1), "peak": PEAK_HBM_GBS,
                                         "unit": "GB/s", "frac": round(wbytes / lat / 1e9 / PEAK_HBM_GBS, 4),
                                         "algorithmic_bytes": wbytes, "note": "live weights streamed once per forward"}}
        model.precision = args.precision

    # ---- cpu_baseline: the oracle (a port — the reference's third-party stack is absent) on the host cores ----
    _ops.set_objective(objective)                            # parity is measured on the headline's kernels
    cpu_baseline, parity_all = None, None
    if cpu_weights is not None:
        from helpers import oracle_cfg
        from oracle import kosmos_oracle as O
        ocfg = oracle_cfg(cfg)
        ctok, cimg = tok[:1].cpu(), img[:1].cpu()
        O.kosmos_forward(cpu_weights, ctok, cimg, ocfg)          # warm-up (page-in, thread pool)
        # a fair CPU number: torch's default (all hardware threads) oversubscribes these small GEMMs on a many-core
        # host, so probe a few thread counts once and time the sample at the fastest
        ncpu = torch.get_num_threads()
        hinfo = host_info()
        quota = hinfo.get("cgroup_cpu_quota_cores")
        qthr = max(1, min(ncpu, int(round(quota)))) if quota else ncpu        # the thread count the cgroup actually pays for
        best_t, best_n = None, ncpu
        for nthr in sorted({ncpu, min(ncpu, 64), min(ncpu, 32), min(ncpu, 16), qthr}, reverse=True):
            torch.set_num_threads(nthr)
            O.kosmos_forward(cpu_weights, ctok, cimg, ocfg)
            t1 = time.perf_counter()
            O.kosmos_forward(cpu_weights, ctok, cimg, ocfg)
            dt1 = time.perf_counter() - t1
            if best_t is None or dt1 < best_t:
                best_t, best_n = dt1, nthr
        torch.set_num_threads(best_n)
        n, t_cpu = 0, 0.0
        while (t_cpu < args.cpu_seconds and n < 64) or n < 2:
            t1 = time.perf_counter()
            O.kosmos_forward(cpu_weights, ctok, cimg, ocfg)
            t_cpu += time.perf_counter() - t1
            n += 1
        # parity of every precision mode against that same CPU forward, measured here and now (sample 0 of the shard):
        # max|logit difference| / rms(logits), the figure the tests bound (1e-5 class fp32, 1e-3 bf16x3, 6e-2 bf16)
        ref_logits = O.kosmos_forward(cpu_weights, ctok, cimg, ocfg)
        parity = {}
        for mode in ("bf16", "mixed", "f16c", "bf16x3", "fp32"):
            model.precision = mode
            with torch.no_grad():                     # sample 0 of the WHOLE shard's forward: the benchmarked kernel path
                got = model(tok, img)[:1].float().cpu()
            parity[mode] = float((got - ref_logits).abs().max() / ref_logits.pow(2).mean().sqrt())
            model.invalidate_packed()                 # drop this mode's operand copies (3-10 GB each)
        model.precision = args.precision
        parity_all = dict(parity)
        parity_all["_logit_rms"] = float(ref_logits.pow(2).mean().sqrt())
        # The yardstick for the fp32 tolerance (north star: 1e-5): the SAME oracle evaluated in float64.  Two fp32
        # implementations of a 50-layer model differ by their summation orders; what each is away from the exact result
        # says whether the HIP fp32 path is any further from the truth than the CPU fp32 path it is compared with.
        with O.working_dtype(torch.float64):
            ref64 = O.kosmos_forward({k: (v.double() if v.is_floating_point() else v) for k, v in cpu_weights.items()},
                                     ctok, cimg.double(), ocfg)
        rms64 = ref64.pow(2).mean().sqrt()
        model.precision = "fp32"
        with torch.no_grad():
            got32 = model(tok, img)[:1].double().cpu()
        model.invalidate_packed()
        model.precision = args.precision
        fp32_vs_64 = {"hip_fp32": float(f"{float((got32 - ref64).abs().max() / rms64):.3e}"),
                      "cpu_fp32_oracle": float(f"{float((ref_logits.double() - ref64).abs().max() / rms64):.3e}"),
                      "note": "max|d|/rms against the float64 evaluation of the same oracle (sample 0)"}
        # The CPU at ITS best batch: a batch-1 latency figure beside a batch-32 GPU throughput figure
        # understates the host.  B = 8 at two thread counts, then B = 32 (the GPU's shard) at the better one; one forward
        # each (3.7 / 14.7 TFLOP) — `value` is the best samples/s the host reached, the batch-1 figure stays beside it.
        b1_rate, b1_threads = n / t_cpu, best_n
        batched = []
        if B >= 8:
            c8t, c8i = tok[:8].cpu(), img[:8].cpu()
            for nthr in sorted({ncpu, min(ncpu, 64)}, reverse=True):
                torch.set_num_threads(nthr)
                t1 = time.perf_counter()
                O.kosmos_forward(cpu_weights, c8t, c8i, ocfg)
                batched.append({"batch": 8, "threads": nthr, "samples_per_s": round(8 / (time.perf_counter() - t1), 4)})
            nthr = max(batched, key=lambda r: r["samples_per_s"])["threads"]
            if B >= 32:
                torch.set_num_threads(nthr)
                t1 = time.perf_counter()
                O.kosmos_forward(cpu_weights, tok[:32].cpu(), img[:32].cpu(), ocfg)
                batched.append({"batch": 32, "threads": nthr, "samples_per_s": round(32 / (time.perf_counter() - t1), 4)})
        torch.set_num_threads(best_n)
        top = max(batched, key=lambda r: r["samples_per_s"]) if batched else None
        use_batched = top is not None and top["samples_per_s"] > b1_rate
        cpu_baseline = {"value": round(top["samples_per_s"] if use_batched else b1_rate, 4), "unit": "samples/s",
                        "cores": top["threads"] if use_batched else b1_threads,
                        "batch": top["batch"] if use_batched else 1,
                        "batch1": {"samples_per_s": round(b1_rate, 4), "cores": b1_threads,
                                   "sample": f"{n} x batch-1 forward, {t_cpu:.1f} s"},
                        "batched": batched,
                        "logit_rms": float(f"{float(ref_logits.pow(2).mean().sqrt()):.4f}"),
                        "parity_max_abs_over_rms": {k: float(f"{v:.3e}") for k, v in parity.items()},
                        "fp32_vs_float64": fp32_vs_64,
                        "host_threads_available": ncpu, "host": hinfo, "kind": "port",
                        "sample": (f"fp32 torch CPU oracle (oracle/kosmos_oracle.py) forward of (1 image + {Tt} tokens) samples: "
                                   f"{n} x batch 1 ({t_cpu:.1f} s) and one forward each at " +
                                   ", ".join(f"batch {r['batch']} / {r['threads']} threads" for r in batched) +
                                   "; value = the fastest of them")}

    # decode block: parity of every timed step against the oracle's full forward, headline = fastest mode inside 1e-3
    if decode_check is not None and decode_check[0] is not None and "modes" in (decode or {}):
        from oracle import kosmos_oracle as O
        lm_cpu, dtok_cpu, kept, first = decode_check
        ref = O.kosmos_language_forward(lm_cpu, dtok_cpu, O.DecoderCfg(vocab=cfg.vocab))[0, first:]
        rms = float(ref.pow(2).mean().sqrt())
        for mode, got in kept.items():
            e = float((got - ref).abs().max() / rms)
            tol = 1e-5 if mode == "fp32" else 1e-3
            decode["modes"][mode]["parity"] = {"max_abs_over_rms": float(f"{e:.3e}"), "logit_rms": float(f"{rms:.4f}"),
                                               "tolerance": tol, "meets": bool(e < tol),
                                               "meets_1e-3": bool(e < 1e-3),
                                               "against": f"fp32 CPU oracle full forward, positions {first}..{first + ref.shape[0] - 1}"}
        ok = [m_ for m_ in decode["modes"] if decode["modes"][m_]["parity"]["meets_1e-3"]]
        if ok:
            best = min(ok, key=lambda m_: decode["modes"][m_]["ms_per_token"])
            decode.update({"fastest_meeting_tolerance": best, **{k: decode["modes"][best][k] for k in
                                                                  ("ms_per_token", "tokens_per_s", "roofline", "parity")}})
        del lm_cpu, ref
    elif decode is not None and "modes" in decode:
        decode["note"] = "parity not measured in this run (--no-cpu-baseline); headline left to the caller"
    if rank == 0:
        from kosmosx.accounting import flops_per_sample
        fl = flops_per_sample(cfg, Tt)
        total = world * B * args.steps
        line = {
            "metric": "multimodal forward samples/sec (224x224 img + 50 tok) @ 24L/2048d",
            "value": round(total / elapsed, 3), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": DTYPE_NAMES[args.precision], "data": "synthetic",
            "full": bool(args.full),
            "config": {"workload": f"{B} samples/GPU/step, each 1x3x224x224 image + {Tt} text tokens -> logits "
                                   f"[{Tt + cfg.perceiver.latents},{cfg.vocab}]; CLIP ViT-L/14 + Perceiver(257->64) + "
                                   "24L/2048d sub-LN XPos decoder, random-init weights (BASELINE.json configs[3] per-GPU share)",
                       "batch_per_gpu": B, "global_batch": world * B, "seq_len": Tt + cfg.perceiver.latents,
                       "text_len": Tt, "parallelism": f"dp{world}",
                       "logits_gather": (None if gatherer is None else f"RCCL {gatherer.last_algo} (requested: {args.gather_algo}), bf16 logits straight from the GEMM epilogue, "
                                                               "issued on a side stream (overlaps the next step)"),
                       # rounds 1-4 shipped --gather-algo auto (= direct above two ranks for this message size); since
                       # round 5 the default is all_gather, the only schedule that has run on more than one GPU-backed rank
                       "logits_gather_note": (None if gatherer is None else
                                              f"default schedule is all_gather since round 5; `auto` would pick "
                                              f"{'direct' if world > 2 else 'all_gather'} at {world} ranks for this shard (pass --gather-algo auto)"),
                       "micro_batch_streams": S, "pipelined_steps": P, "hip_graph": bool(args.graph),
                       "schedule_objective": (f"{objective} (kx_set_tuning key 18 = {1 if objective == 'throughput' else 0}: " +
                                              ("steps in flight on separate streams -> launches chosen for the fewest CU-microseconds "
                                               "(256-row tiles where 192-row ones only saved padding); bit-identical results; "
                                               "+2.7 % against the latency objective with two steps in flight, -3 % with one: "
                                               "profiles/r06_h_cutime_ab*.log)" if objective == "throughput" else
                                               "one step at a time -> launches chosen to finish soonest alone on the chip)"))},
            "algorithmic_gflop_per_sample": round(fl["total"] / 1e9, 2),
            "model_tflops": round(fl["total"] * total / elapsed / 1e12, 2),
            "mfma_peak_frac_end_to_end": round(fl["total"] * total / elapsed / 1e12 / (PEAK_BF16_TFLOPS * world), 4),
            "parity": parity_block(args.precision, parity_all),
            "roofline": roofline, "cpu_baseline": cpu_baseline,
            "precision_modes": modes_block(args.precision, round(total / elapsed, 3), elapsed / args.steps, other_modes,
                                           parity_all, fl["total"], B),
            "c3": c3, "batch1": batch1, "decode": decode, "training_step": training,
            "kernel_breakdown": breakdown,
            "gemm_shapes": gemm_shapes,
            "build_seconds": round(t_build, 1),
        }
        try:                                    # RCCL's banner sits in libc's stdout buffer: flush it BEFORE the JSON line
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(line), flush=True)
    if world > 1 or force_dist:
        dist.barrier()                      # rank 0 finishes its instrumented leg before anyone tears down
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
